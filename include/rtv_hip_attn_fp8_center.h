/* K smoothing for the fp8 self-attention of rtv_hip_attn_fp8.h: the e4m3 shadow of K holds the codes of k - c, with one fp32 centre
 * c[h][d] per head and channel, instead of the codes of k.  Opt-in.  Same conventions as rtv_hip.h: device pointers unless stated,
 * 0 = success, non-zero = failure with the reason in rtv_last_error(), every launch goes to `stream`, no allocation and no
 * synchronisation inside.
 *
 * Why it is exact: with k' = k - c every score of a query moves by the same q . c, and softmax is invariant under a constant added
 * to a row - with the quantised q^ as well, because one q^ multiplies every key.  rtv_attn_fwd_fp8 therefore runs unchanged on a
 * centred shadow, for ANY fixed vector c; what c buys is that keys with a per-channel offset (RMSNorm weights, slowly rotating RoPE
 * pairs) spend the three mantissa bits of e4m3 on k - c, not on the offset.  The natural c is the column mean of the cached keys
 * (what SageAttention subtracts), which rtv_attn_kv_center computes.
 *
 * A header of its own, like rtv_hip_mx_rotate.h: nothing here changes a signature or a layout of rtv_hip.h or of
 * rtv_hip_attn_fp8.h, and RTV_ABI_VERSION stays as it is.
 *
 * ARITHMETIC of the centred K codes (part of the ABI; tests/attn_fp8_center_cases.py is the restatement):
 *   1. t = fp32(k) - c[h][d]          one fp32 subtraction, round to nearest even
 *   2. code = e4m3_rne(clamp(t / k_scale, -448, 448))      the fp32 division, clamp and conversion of rtv_attn_quantize_kv
 * c = 0 gives the bytes of rtv_attn_quantize_kv (x - 0 is exact).  V is not touched. */
#ifndef RTV_HIP_ATTN_FP8_CENTER_H
#define RTV_HIP_ATTN_FP8_CENTER_H
#include <stddef.h>
#include <stdint.h>

#include "rtv_hip_attn_fp8.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Rows one first-stage workgroup of rtv_attn_kv_center sums. */
#define RTV_ATTN_CENTER_CHUNK 256

/* Bytes of workspace rtv_attn_kv_center needs for `rows` = n0 + n1 key rows of H heads (0 when either is not positive). */
size_t rtv_attn_kv_center_workspace_bytes(int rows, int H);

/* center[h][d] = fp32 mean over the key rows of k[row][h][d]: k points at row 0, head 0 of the bf16 K plane of a cache (row stride
 * `row_stride` elements, >= H * 128, a multiple of 8: the K plane of an interleaved K / V arena is fine), the rows are the physical
 * ranges [row0, row0 + n0) followed by [row1, row1 + n1) - the window shape of rtv_attn_fwd_fp8, so a wrapped ring is one call.
 * Two stages: every workgroup sums one chunk of RTV_ATTN_CENTER_CHUNK rows of one head in fp32 in a fixed order into `workspace`,
 * then one workgroup per head adds the chunks in order and divides by n0 + n1.  No atomics: the same input gives the same bits.
 * center: device float [H][128], 16-byte aligned.
 * Refused before any launch: a null k / center / workspace, a pointer that is not 16-byte aligned, non-positive n0 or H, negative
 * n1, a negative first row of a non-empty range, a row stride below H * 128 or not a multiple of 8, more than 65535 heads, a
 * workspace below rtv_attn_kv_center_workspace_bytes(n0 + n1, H). */
int rtv_attn_kv_center(const void* k, int64_t row_stride, int row0, int n0, int row1, int n1, int H, float* center, void* workspace,
                       size_t workspace_bytes, rtv_stream_t stream);

/* rtv_attn_quantize_kv (same arguments, same checks, same partial-tile rules: only the bytes of the rows in the range are written,
 * [a, b) then [b, c) equals [a, c)) with the K codes of k - center, as under ARITHMETIC.  center: device float [H][128], 16-byte
 * aligned, not null.  V codes are those of rtv_attn_quantize_kv.  amax[0] is the running maximum of |k - center| - the value that
 * saturates at 448 * k_scale -, amax[1] that of |v|. */
int rtv_attn_quantize_kv_centered(const void* k, const void* v, int64_t row_stride, int row0, int rows, int H, void* k8, void* v8t,
                                  int cache_rows, float k_scale, float v_scale, void* amax, const float* center,
                                  rtv_stream_t stream);

/* rtv_dit_forward_attn_fp8 with every quantisation of the rows the call writes (both ranges of a wrapped write, the kv_only pass
 * too) going through rtv_attn_quantize_kv_centered with the layer's centre: centers is a HOST array of num_layers device
 * float [H][128] pointers.  The attention launches are those of rtv_dit_forward_attn_fp8 - the centre does not enter them.  The
 * shadow's rows quantised earlier must hold codes under the same centre; keeping that true is the caller's business.
 * Refuses what rtv_dit_forward_attn_fp8 refuses (a sharded step, attn_kv_splits > 1, a missing shadow) and a null centre table or
 * a null entry of it.  rtv_dit_forward_attn_fp8 itself issues exactly what it issued before. */
int rtv_dit_forward_attn_fp8_centered(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* step,
                                      const rtv_attn_fp8_shadow* shadow, void* const* centers, void* workspace,
                                      size_t workspace_bytes, rtv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
