/* Text cross-attention with V folded into the output projection (rtv_dit_step.ca_vo_ld, include/rtv_hip.h): the three entry points
 * the fold adds.  A header of its own, like rtv_hip_io.h / rtv_hip_jpeg.h / rtv_hip_lora.h: nothing here changes a signature of
 * rtv_hip.h (the trailing field ca_vo_ld of rtv_dit_step is ABI revision 104 there). */
#ifndef RTV_HIP_CROSS_FOLD_H
#define RTV_HIP_CROSS_FOLD_H
#include "rtv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The PROBABILITIES of rtv_attn_fwd_dup for a key window that fits in registers (Lkv <= 128), written out instead of being
 * multiplied by V (bf16 only):
 *   p[row, h * kh + t] = bf16(softmax_t(scale q_h . k_{h,t} + log(count_t)))     t < Lkv, count = dup_count at dup_key, else 1
 * A plain (not online) softmax, normalised in fp32 before the rounding.  Every other column of [0, p_cols) - t in [Lkv, kh) of
 * a head and the tail [H * kh, p_cols) - is written as zero, so `p` is the A operand of a GEMM against a weight laid out the
 * same way (rtv_cross_fold_weight).  kh % 8 == 0, Lkv <= kh, H * kh <= p_cols <= p_row_stride, p_cols % 8 == 0, 16-byte rows.
 * dup_count == 1: a plain window. */
int rtv_attn_probs_dup(const void* q, const void* k, void* p, int Lq, int Lkv, int H, int D,
                       int64_t q_row_stride, int64_t k_row_stride, int64_t p_row_stride, int kh, int p_cols,
                       float scale, int dup_key, int dup_count, rtv_stream_t stream);

/* Column layout of the folded cross-attention: kh = round_up(text_rows + 1, 8) columns per head (the real keys, the counted
 * padding key, zero padding), k_fold = round_up(num_heads * kh, 64) columns in all (the GEMM's K).  Returns 1 when the fold
 * applies to this prompt length, else 0; kh / k_fold (may be NULL) are filled either way.  It applies up to
 * kh = RTV_CROSS_FOLD_KH_MAX, the widest layout measured: at 14B width the folded pair (probabilities + GEMM) is 111 / 89 / 67 /
 * 34 / 12 us per layer faster than the unfolded one at kh = 40 / 72 / 88 / 104 / 120, repeat spread under 1 us
 * (profiles/cross_fold_kh_sweep.txt); kh = 128 (extrapolated: about break-even) was not measured and stays unfolded. */
#define RTV_CROSS_FOLD_KH_MAX 120
int rtv_cross_fold_dims(int num_heads, int text_rows, int* kh, int* k_fold);
/* vo[n, h*kh + t] = bf16(sum_d' co_w[n, h*128 + d'] * v[t, h*128 + d']) for t < rows (fp32 accumulation), zeros in the other
 * columns of [0, k_fold): the folded weight of one layer.  co_w [dim][ldw], v [rows][ldv], vo [dim][ldvo]; dim = num_heads * 128. */
int rtv_cross_fold_weight(const void* co_w, int64_t ldw, const void* v, int64_t ldv, void* vo, int64_t ldvo,
                          int num_heads, int rows, int kh, int k_fold, rtv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
