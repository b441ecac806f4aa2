/* fp8 self-attention on an e4m3-ONLY KV cache: the mode of rtv_hip_attn_fp8.h without the bf16 cache beside the shadow.  Same
 * conventions as rtv_hip.h: device pointers unless stated, 0 = success, non-zero = failure with the reason in rtv_last_error(),
 * every launch goes to `stream`, no allocation and no synchronisation inside.
 *
 * A header of its own for the reason rtv_hip_attn_fp8.h is one: nothing here changes a struct layout or a signature, and
 * RTV_ABI_VERSION stays as it is.  The forward takes the same rtv_attn_fp8_shadow, whose k8 / v8t now ARE the cache.
 *
 * What the mode keeps per layer is the two byte arrays of rtv_hip_attn_fp8.h, in exactly that layout (k8 dense, v8t transposed
 * per 64-row storage tile, RTV_ATTN_FP8_SLOT): 10 240 bytes per row at 14B width instead of the 30 720 of the shadow mode (bf16 K
 * and V plus the shadow).  No bf16 K or V row of the cache exists anywhere: a block's K and V are bf16 only in the projection
 * buffer [M][3 d] the forward has anyway.  The codes are those of the shadow mode bit for bit, because the kernels here take the
 * shadow mode's two roundings in registers: K is rounded to bf16 as the cache write rounds it, and that bf16 value is quantised;
 * V is quantised from the bf16 projection output, which is what the shadow mode's V cache rows hold.
 *
 * The dict contract of the Python side (realtime_video_amd.CausalWanModel.enable_fp8_attention(bf16_cache=False)): the KV cache of
 * a layer is {"k8", "v8t", "rows", "global_end_index", "local_end_index"} (model.new_fp8_kv_cache(rows, device)), with no "k" /
 * "v" entry.  Refused there, never run in another precision: smooth_k=True (recentring reads the bf16 K cache),
 * context_parallel=True or a model with context_parallel set when the call does not ask for context_parallel="codes", a dict with
 * "k" / "v" handed to a model in the mode, a compact dict handed to a model that is not, and a change of k_scale / v_scale on a
 * cache that holds rows (the codes cannot be derived again: reset the cache).
 *
 * Out of scope here: K smoothing and converting a live bf16 cache into a compact one (rtv_hip_attn_fp8_only_center.h), context
 * parallelism on a compact cache (rtv_hip_attn_fp8_only_cp.h: the row exchange, carrying the codes; the head exchange stays
 * refused), and any change to the attention kernel, which is rtv_attn_fwd_fp8 as it is. */
#ifndef RTV_HIP_ATTN_FP8_ONLY_H
#define RTV_HIP_ATTN_FP8_ONLY_H
#include <stdint.h>

#include "rtv_hip_attn_fp8.h"
#ifdef __cplusplus
extern "C" {
#endif

/* rtv_qk_norm_rope_cache_ring (rtv_hip.h) with the K rows stored as e4m3 codes and no V role: one pass over the Q and K thirds of
 * qkv [M][3 d]:
 *   q = rope(rmsnorm(q) * wq) -> q_out [M][d] bf16, as rtv_qk_norm_rope_cache_ring writes it (q_out NULL: the q role is skipped -
 *       the kv_only pass);
 *   k = rope(rmsnorm(k) * wk), rounded to bf16 exactly as the cache write rounds it, then
 *       code = e4m3_rne(clamp(k / k_scale, -448, 448)) -> k8 [cache_rows][num_heads][128], physical row by the ring mapping of
 *       rtv_qk_norm_rope_cache_ring (logical row cache_row0 + row_offset + m).
 * amax: optional device float[2]; amax[0] = running maximum of |k| (the bf16 values, NaNs ignored), raised with at most one atomic
 * maximum per workgroup as rtv_attn_quantize_kv does; amax[1] is not touched.  NULL switches it off.
 * Refused before any launch: everything rtv_qk_norm_rope_cache_ring refuses (with its messages), a head dimension other than 128,
 * a null qkv / k8 / wq / wk / rope_cs, a qkv / q_out / k8 / wq / wk that is not 16-byte aligned (amax: 4-byte), non-positive
 * cache_rows, a physical row outside [0, cache_rows) (no ring: cache_row0 + row_offset + M > cache_rows; ring: ring_lo + ring_size
 * > cache_rows), a non-finite or non-positive k_scale. */
int rtv_qk_norm_rope_k8(const void* qkv, void* q_out, void* k8, int cache_rows, float k_scale, void* amax, int cache_row0, int M,
                        int d, int num_heads, float eps, const void* wq, const void* wk, const void* rope_cs, int F, int gh, int gw,
                        int start_frame, int row_offset, int ring_lo, int ring_size, int ring_shift, rtv_stream_t stream);

/* Quantise `rows` bf16 rows of a staging matrix into v8t: source row i (v_src + i * src_row_stride elements, H * 128 values) goes
 * to the physical row dst_row0 + i, code = e4m3_rne(clamp(v / v_scale, -448, 448)), transposed per storage tile as
 * rtv_attn_quantize_kv stores it.  In the forward v_src is the V third of the projection buffer, src_row_stride = 3 d.  Only the
 * bytes of the rows given are written: neighbouring slots of a partly covered tile keep their contents, so quantising [a, b) and
 * then [b, c) equals quantising [a, c).
 * amax: optional device float[2]; amax[1] = running maximum of |v|, as rtv_attn_quantize_kv; amax[0] is not touched.
 * Refused before any launch: a null v_src / v8t, a pointer that is not 16-byte aligned (amax: 4-byte), non-positive rows, H or
 * cache_rows, a range outside [0, cache_rows), a row stride below H * 128 or not a multiple of 8, a non-finite or non-positive
 * scale, more than 65535 heads. */
int rtv_attn_quantize_v_rows(const void* v_src, int64_t src_row_stride, int rows, int H, void* v8t, int cache_rows, int dst_row0,
                             float v_scale, void* amax, rtv_stream_t stream);

/* rtv_dit_forward_attn_fp8 on a cache that is only shadow->k8 / v8t: step->kv_k / kv_v / kv_row_stride are never read (kv_k and
 * kv_v may be NULL).  Every layer projects Q | K | V into the projection buffer in one GEMM (no direct V GEMM: there is no V cache
 * row to write), runs rtv_qk_norm_rope_k8, then rtv_attn_quantize_v_rows once per physical segment of the rows the call writes
 * (sink rows, ring rows, the wrapped rest - each with its source rows), then rtv_attn_fwd_fp8 on the key window; the kv_only pass
 * likewise.  Every output, code and maximum equals rtv_dit_forward_attn_fp8's bit for bit.
 * Refused before any launch: what rtv_dit_forward_attn_fp8 refuses, with its messages - a null shadow, k8 / v8t table or
 * cache_rows <= 0, a step with row_count < M or attn_kv_splits > 1 - and a layer without k8 / v8t, a k8 / v8t that is not 16-byte
 * aligned (amax: 4-byte), non-finite or non-positive scales, written rows or a key window outside [0, cache_rows). */
int rtv_dit_forward_attn_fp8_only(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* step,
                                  const rtv_attn_fp8_shadow* shadow, void* workspace, size_t workspace_bytes, rtv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
