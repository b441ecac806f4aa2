/* K smoothing on the e4m3-ONLY KV cache of rtv_hip_attn_fp8_only.h: the compact cache holds the codes of k - c
 * (rtv_hip_attn_fp8_center.h) although no bf16 K row exists to take c from or to requantise.  Opt-in.  Same conventions as
 * rtv_hip.h: device pointers unless stated, 0 = success, non-zero = failure with the reason in rtv_last_error(), every launch goes
 * to `stream`, no allocation and no synchronisation inside.
 *
 * A header of its own for the reason its parents are: nothing here changes a struct layout or a signature, RTV_ABI_VERSION stays as
 * it is, and every existing entry point issues exactly what it issued before.
 *
 * What is covered now, of what rtv_hip_attn_fp8_only.h lists as out of scope:
 *   K smoothing            a fresh K row is bf16 in registers inside the cache-write kernel: rtv_qk_norm_rope_k8_centered subtracts
 *                          the centre there.  The centre comes from the codes themselves (rtv_attn_k8_center), and the rows already
 *                          in the cache move to it in place (rtv_attn_k8_recenter).
 *   converting a live bf16 cache into a compact one   needs no kernel of its own: a shadow of rtv_hip_attn_fp8.h IS a compact cache
 *                          (the Python side drops the bf16 tensors, realtime_video_amd.CausalWanModel.convert_kv_cache_to_fp8).
 * Still out of scope: context parallelism on a compact cache, any change to the attention kernel, Q or V smoothing, recentring
 * inside a forward.
 *
 * What a recentre costs in accuracy: a row written before it keeps the error of its first rounding and takes a second one (at most
 * the same step, so at most a factor sqrt(2) in quadrature); every row written afterwards is rounded once, under the new centre.
 *
 * ARITHMETIC of rtv_attn_k8_recenter (part of the ABI; tests/attn_fp8_only_center_cases.py is the restatement), per code:
 *   1. delta = c_old[h][d] - c_new[h][d]       one fp32 subtraction
 *   2. x = fp32(code) * k_scale                one fp32 multiplication
 *   3. t = x + delta                           one fp32 addition, NOT contracted with step 2
 *   4. code' = e4m3_rne(clamp(t / k_scale, -448, 448))     the fp32 division, clamp and conversion of rtv_attn_quantize_kv
 * Consequences: with delta = 0 every non-NaN code is kept, except that 0x80 (-0) becomes 0x00 (-0 + 0 = +0); the result lies within
 * e4m3's half step at |t| / k_scale of x + delta.
 * NaN codes (0x7F, 0xFF) do not occur in a cache the quantisers wrote (they clamp).  One that is there anyway: rtv_attn_k8_recenter
 * keeps its byte and ignores it in amax; rtv_attn_k8_center makes the mean of its (head, channel) column NaN, and only that
 * column's. */
#ifndef RTV_HIP_ATTN_FP8_ONLY_CENTER_H
#define RTV_HIP_ATTN_FP8_ONLY_CENTER_H
#include <stddef.h>
#include <stdint.h>

#include "rtv_hip_attn_fp8_center.h"
#include "rtv_hip_attn_fp8_only.h"
#ifdef __cplusplus
extern "C" {
#endif

/* rtv_qk_norm_rope_k8 (same arguments, same checks, same messages) with the K codes of k - center: the K role is unchanged up to
 * the bf16 packing of the rotated row; the unpacked bf16 value then goes through the ARITHMETIC of rtv_hip_attn_fp8_center.h,
 * t = fp32(k) - center[h][d], code = e4m3_rne(clamp(t / k_scale, -448, 448)).  amax[0] follows |k - center|.  The q role is
 * unchanged.  The codes equal, bit for bit, those of rtv_qk_norm_rope_cache_ring followed by rtv_attn_quantize_kv_centered on the
 * rows written; center = 0 gives the bytes of rtv_qk_norm_rope_k8.
 * center: device float [num_heads][128], 16-byte aligned, not null (refused before any launch otherwise). */
int rtv_qk_norm_rope_k8_centered(const void* qkv, void* q_out, void* k8, int cache_rows, float k_scale, void* amax, int cache_row0,
                                 int M, int d, int num_heads, float eps, const void* wq, const void* wk, const void* rope_cs, int F,
                                 int gh, int gw, int start_frame, int row_offset, int ring_lo, int ring_size, int ring_shift,
                                 const float* center, rtv_stream_t stream);

/* Column means of the DEQUANTISED keys of a compact cache: center_new[h][d] = c_old[h][d] + mean over the rows of
 * fp32(code) * k_scale - the mean of the keys as the cache knows them, when its codes stand under c_old.  k8
 * [cache_rows][H][128] e4m3 codes; the rows are the physical ranges [row0, row0 + n0) followed by [row1, row1 + n1), as in
 * rtv_attn_kv_center.  The same two-stage scheme without atomics (chunks of RTV_ATTN_CENTER_CHUNK rows summed in fp32 in a fixed
 * order into `workspace`, then one workgroup per head adds the chunks in order, divides by n0 + n1 and adds c_old): the same input
 * gives the same bits.  workspace: rtv_attn_kv_center_workspace_bytes(n0 + n1, H) bytes.  center_new may be c_old.
 * Refused before any launch: a null k8 / c_old / center_new / workspace, a pointer that is not 16-byte aligned, non-positive n0, H
 * or cache_rows, negative n1, a non-empty range outside [0, cache_rows), a non-finite or non-positive k_scale, more than 65535
 * heads, a workspace below rtv_attn_kv_center_workspace_bytes(n0 + n1, H). */
int rtv_attn_k8_center(const void* k8, int cache_rows, int row0, int n0, int row1, int n1, int H, float k_scale, const float* c_old,
                       float* center_new, void* workspace, size_t workspace_bytes, rtv_stream_t stream);

/* Move the rows [row0, row0 + rows) of k8 [cache_rows][H][128] from centre c_old to centre c_new, in place, by the ARITHMETIC
 * above.  Only the bytes of the rows given are written: [a, b) followed by [b, c) equals [a, c).
 * amax: optional device float[2]; amax[0] is raised to max |t| (NaNs ignored) with at most one atomic maximum per workgroup;
 * amax[1] is not touched.  NULL switches it off.
 * Refused before any launch: a null k8 / c_old / c_new, a k8 / c_old / c_new that is not 16-byte aligned (amax: 4-byte),
 * non-positive rows, H or cache_rows, a range outside [0, cache_rows), a non-finite or non-positive k_scale, more than 65535
 * heads. */
int rtv_attn_k8_recenter(void* k8, int cache_rows, int row0, int rows, int H, float k_scale, const float* c_old, const float* c_new,
                         void* amax, rtv_stream_t stream);

/* rtv_dit_forward_attn_fp8_only with every K row the call writes going through rtv_qk_norm_rope_k8_centered with the layer's
 * centre: centers is a HOST array of num_layers device float [H][128] pointers, as in rtv_dit_forward_attn_fp8_centered.  V and the
 * attention launches are those of rtv_dit_forward_attn_fp8_only.  The rows already in the cache must hold codes under the same
 * centre; keeping that true is the caller's business (rtv_attn_k8_recenter).  Every output, code and maximum equals
 * rtv_dit_forward_attn_fp8_centered's bit for bit.
 * Refuses what both parents refuse, with their messages, before any launch. */
int rtv_dit_forward_attn_fp8_only_centered(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* step,
                                           const rtv_attn_fp8_shadow* shadow, void* const* centers, void* workspace,
                                           size_t workspace_bytes, rtv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
