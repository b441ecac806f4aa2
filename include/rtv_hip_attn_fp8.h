/* fp8 self-attention side of librtv_hip.so: attention on an OCP e4m3 shadow of the bf16 KV cache (8-bit K . Q^T and fp8 P . V, the
 * precision of the reference's SageAttention backend, wan/modules/sage.py).  Same conventions as rtv_hip.h: device pointers unless
 * stated, 0 = success, non-zero = failure with the reason in rtv_last_error(), every launch goes to `stream`, no allocation and no
 * synchronisation inside.
 *
 * A header of its own for the reason rtv_hip_lora.h is one: the declarations were added without a new ABI revision - nothing here
 * changes a struct layout or a signature of rtv_hip.h (the DiT forward takes the shadows as an ARGUMENT of an entry point of its
 * own, rtv_dit_forward_attn_fp8, not as a field of rtv_dit_step) and RTV_ABI_VERSION stays as it is.
 *
 * The shadow of one layer's cache [cache_rows][H][128] is two byte arrays:
 *   k8   e4m3 [cache_rows][H][128], dense, row-major:  code = e4m3_rne(clamp(k / k_scale, -448, 448))  (OCP e4m3fn, saturating);
 *   v8t  the same codes of v with v_scale, stored TRANSPOSED per storage tile of 64 physical rows:
 *        [ceil(cache_rows / 64)][H][128 dims][64 key slots] bytes, tile index = physical row >> 6, and inside a tile
 *            key  32 kb + 8 i + 4 g + j   (kb, g in 0..1, i, j in 0..3)   lives in slot   32 g + 16 kb + 4 i + j.
 *        (RTV_ATTN_FP8_SLOT below.)  The kernel computes S^T = K . Q^T on 32x32x64 MFMAs, so a lane owns one query column and, of
 *        a 32-key block kb, the keys 8 i + 4 g + j in C/D register r = 4 i + j (g = lane >> 5); as the B operand of the P . V MFMA
 *        the same lane supplies the 32 consecutive k-bytes 32 g .. 32 g + 31.  With this slot order its 32 probabilities, in
 *        register order (kb, r), ARE those bytes: no cross-lane movement between the two products. */
#ifndef RTV_HIP_ATTN_FP8_H
#define RTV_HIP_ATTN_FP8_H
#include <stdint.h>

#include "rtv_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* slot of key `key` (0..63, = physical row & 63) inside its storage tile of v8t */
#define RTV_ATTN_FP8_SLOT(key) ((((key) >> 2) & 1) * 32 + ((key) >> 5) * 16 + (((key) >> 3) & 3) * 4 + ((key) & 3))

/* Bytes of the two shadow arrays of a cache of `cache_rows` rows and H heads. */
#define RTV_ATTN_FP8_K8_BYTES(cache_rows, H) ((size_t)(cache_rows) * (size_t)(H) * 128)
#define RTV_ATTN_FP8_V8T_BYTES(cache_rows, H) ((((size_t)(cache_rows) + 63) / 64) * (size_t)(H) * 8192)

/* What rtv_dit_forward_attn_fp8 takes (a HOST struct).  k8 / v8t / amax are HOST arrays of
 * num_layers device pointers: the shadow of layer l's cache and its float[2] running maxima (an entry of amax, or amax itself, may
 * be NULL).  Every layer's shadow has `cache_rows` rows = the rows of its bf16 cache. */
typedef struct {
  void* const* k8;
  void* const* v8t;
  int cache_rows;
  float k_scale;
  float v_scale;
  void* const* amax;
} rtv_attn_fp8_shadow;

/* Quantise the physical rows [row0, row0 + rows) of a bf16 KV cache [cache_rows][H][128] into its shadow.  k / v point at row 0,
 * head 0 of the K and of the V plane; both have the row stride `row_stride` in elements (>= H * 128, a multiple of 8; K and V may be
 * the two planes of one interleaved arena).  A row range that ends inside a storage tile writes only its own rows' bytes of v8t:
 * neighbouring slots keep their contents, so quantising [a, b) and then [b, c) equals quantising [a, c).
 * amax: optional device float[2] = running maxima of |k| and |v| over everything quantised so far (raw bf16 values, before the
 * division; NaNs are ignored), updated with an atomic maximum on the bit patterns of the non-negative floats; NULL switches it off.
 * With scale 1 a value above 448 saturates - amax is how the host sees that.
 * Refused before any launch: a null k / v / k8 / v8t, a pointer that is not 16-byte aligned (amax: 4-byte), non-positive rows, H or
 * cache_rows, a range outside [0, cache_rows), a row stride below H * 128 or not a multiple of 8, a non-finite or non-positive
 * scale. */
int rtv_attn_quantize_kv(const void* k, const void* v, int64_t row_stride, int row0, int rows, int H, void* k8, void* v8t,
                         int cache_rows, float k_scale, float v_scale, void* amax, rtv_stream_t stream);

/* o = softmax(scale * q k^T) v for B = 1, head dimension 128, on the shadow.  q bf16 [Lq][H][128] (row stride q_row_stride
 * elements), o bf16 likewise.  The key window is the physical rows [row0, row0 + n0) followed by [row1, row1 + n1) (as
 * rtv_attn_fwd_win: key j of the first range is row row0 + j); causal_block > 0 needs n1 == 0 and is the prefix rule of rtv_attn_fwd:
 * query row i sees the keys j < min(n0, ((q_offset + i) / causal_block + 1) * causal_block).
 * Arithmetic: q is quantised inside the kernel with one scale per (row, head), s_q = max(max |q|, 1e-12) * fp32(1 / 448),
 * code = e4m3_rne(clamp(q / s_q, -448, 448)); both products run on v_mfma_f32_32x32x64_f8f6f4 with fp32 accumulation; the scores
 * are multiplied by s_q * k_scale * scale * log2(e) in fp32; online softmax in the exp2 domain with a reference point at most 2^8
 * below the row maximum (P <= 256 < 448: no P scale); the row sum l comes from the unrounded fp32 P; P is rounded once to e4m3;
 * O * (v_scale / l) is rounded once to bf16.  The kernel walks 64-row storage tiles: keys of a tile that lie outside the window or
 * beyond a row's causal limit get the score -inf, and the V bytes of keys outside the window are replaced by zero (such rows may
 * hold anything, NaN codes included).
 * Refused before any launch: a null pointer, a pointer that is not 16-byte aligned, a row stride below H * 128 or not a multiple of
 * 8, non-positive Lq, H, n0 or cache_rows, negative n1, causal_block or q_offset, a range outside [0, cache_rows),
 * causal_block > 0 together with n1 > 0, a non-finite or non-positive scale / k_scale / v_scale. */
int rtv_attn_fwd_fp8(const void* q, const void* k8, const void* v8t, void* o, int Lq, int H, int cache_rows, int row0, int n0,
                     int row1, int n1, int64_t q_row_stride, int64_t o_row_stride, float scale, float k_scale, float v_scale,
                     int causal_block, int q_offset, rtv_stream_t stream);

/* rtv_dit_forward (rtv_hip.h) with the self-attention of every layer in fp8: each layer quantises exactly the physical rows the call
 * writes into its cache - behind the RoPE / cache kernel and the direct V GEMM, by the ring mapping of the write (two ranges when it
 * wraps), in the kv_only pass too - into shadow->k8[l] / v8t[l], then attends the key window of the step with rtv_attn_fwd_fp8.
 * Cross-attention and everything else are rtv_dit_forward's launches; rtv_dit_forward itself issues exactly what it issued before.
 * A step with row_count < M or attn_kv_splits > 1 is an error here that says so, never a bf16 run: sharded and split steps go
 * through the phases of rtv_hip_attn_fp8_cp.h. */
int rtv_dit_forward_attn_fp8(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* step,
                             const rtv_attn_fp8_shadow* shadow, void* workspace, size_t workspace_bytes, rtv_stream_t stream);

/* Test hook (not part of the drop-in boundary): while q_copy is non-NULL, every self-attention of an unsharded layer
 * (rtv_dit_forward, rtv_dit_layer_rest), in either precision, copies its query rows and - when o_copy is non-NULL - its output,
 * [M][dim] bf16 each, into them on the call's stream (the last layer that runs wins): what a test needs to repeat one attention launch
 * of a forward through rtv_attn_fwd_fp8 / rtv_attn_fwd_win.  NULL, NULL switches it off. */
int rtv_dit_lab_capture_self_attn(void* q_copy, void* o_copy);

#ifdef __cplusplus
}
#endif
#endif
