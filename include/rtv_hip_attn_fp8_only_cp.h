/* The e4m3-only KV cache of rtv_hip_attn_fp8_only.h under the ROW exchange of context parallelism, with the exchange carrying the
 * e4m3 CODES instead of bf16 rows.  Opt-in.  Same conventions as rtv_hip.h: device pointers unless stated, 0 = success, non-zero =
 * failure with the reason in rtv_last_error(), every launch goes to `stream`, no allocation and no synchronisation inside.
 *
 * A header of its own, like its siblings: nothing here changes a signature or a layout of rtv_hip.h, rtv_hip_attn_fp8.h,
 * rtv_hip_attn_fp8_cp.h or rtv_hip_attn_fp8_only.h (rtv_dit_step, rtv_dit_config and rtv_attn_fp8_shadow are what they were: the
 * staging pointer is an argument), RTV_ABI_VERSION stays as it is, and every older entry point issues exactly what it issued before.
 *
 * k_scale / v_scale are two scalars of the mode and a row's codes depend on that row alone, so a rank quantises only the rows it
 * projected (STAGE), one in-place all-gather per layer moves every rank's codes to every rank, and each rank places the M gathered
 * rows into the layer's k8 / v8t (COMMIT).  No bf16 cache row exists anywhere; the codes, the maxima and every output are bit for
 * bit those of rtv_dit_forward_attn_fp8_only on the unsharded block.
 *
 * THE STAGING LAYOUT (part of the ABI; tests/attn_fp8_only_cp_cases.py is the restatement).
 *   kv8: a caller-owned uint8 [world][2][M / world][H * 128] buffer, 16-byte aligned, M = F * gh * gw rows of the block.
 *   Rank-major: rank r's segment is its M / world rows of K codes, then its M / world rows of V codes, both row-major (a row = H
 *   heads of 128 codes, the row layout of k8).  A rank's segment is one contiguous message, so the exchange of a layer is ONE
 *   in-place all-gather along the first axis.  One buffer per (M, device) serves all layers: layer l's codes are committed before
 *   layer l + 1 stages.
 *
 * Out of scope, and refused by the Python side: the head exchange (it keeps 1 / world of the cache per rank already), K smoothing
 * and converting a live bf16 cache under context parallelism. */
#ifndef RTV_HIP_ATTN_FP8_ONLY_CP_H
#define RTV_HIP_ATTN_FP8_ONLY_CP_H
#include <stddef.h>
#include <stdint.h>

#include "rtv_hip_attn_fp8.h"
#ifdef __cplusplus
extern "C" {
#endif

/* STAGE: the codes of the logical rows [row_begin, row_begin + row_count) of a block of M = F * gh * gw rows into kv8.  qkv is the
 * projection buffer [row_count][3 d] bf16 of those rows (row i = logical row row_begin + i, the row_offset convention of
 * rtv_qk_norm_rope_k8); its Q third is not read.
 *   K codes: what rtv_qk_norm_rope_k8 writes for the row - k = rope(rmsnorm(k) * wk) at the row's true position (start_frame, the
 *       row's place in the F x gh x gw grid), rounded to bf16 as the cache write rounds it, code = e4m3_rne(clamp(k / k_scale,
 *       -448, 448)); written by that kernel itself, with the K rows of the segment as its k8.
 *   V codes: code = e4m3_rne(clamp(v / v_scale, -448, 448)) of the bf16 V third, the rounding of rtv_attn_quantize_v_rows, stored
 *       row-major (16-byte loads, 16-byte stores).
 * amax: optional device float[2]; amax[0] / amax[1] = running maxima of |k| / |v| over the rows this call wrote, raised as
 * rtv_qk_norm_rope_k8 and rtv_attn_quantize_v_rows raise them.  NULL switches it off.
 * Refused before any launch: a null qkv / kv8 / wk / rope_cs, a qkv / kv8 / wk that is not 16-byte aligned (rope_cs: 8-byte, amax:
 * 4-byte), world <= 0, M % world != 0, rows outside [0, M) or in more than one rank's segment, a head dimension other than 128,
 * non-finite or non-positive scales, and everything rtv_qk_norm_rope_k8 refuses, with its messages. */
int rtv_attn_fp8_stage_kv8(const void* qkv, void* kv8, int world, int row_begin, int row_count, float k_scale, float v_scale,
                           void* amax, int d, int num_heads, float eps, const void* wk, const void* rope_cs, int F, int gh, int gw,
                           int start_frame, rtv_stream_t stream);

/* COMMIT: the M rows of a gathered kv8 (H heads) into k8 / v8t of one layer, a cache of cache_rows rows.  Logical row cache_row0 +
 * m goes to its physical row by the ring mapping of rtv_dit_step: sink rows in place, ring rows rotated by ring_shift, at most one
 * wrap (ring_size == 0: physical = logical).
 *   K rows are copied byte for byte.
 *   V rows go through the tile packer of rtv_attn_quantize_v_rows (LDS transpose, RTV_ATTN_FP8_SLOT): whole 64-row storage tiles
 *       leave as 16-byte pieces, a partly covered tile writes only the bytes of its own rows - neighbouring slots keep their
 *       contents.
 * A byte mover: no arithmetic on the codes.  H and the row counts are arguments, so that a head-exchange form can use it with H =
 * num_heads / world.
 * Refused before any launch: a null kv8 / k8 / v8t, a pointer that is not 16-byte aligned, world <= 0, M <= 0, M % world != 0, H
 * outside 1..65535, non-positive cache_rows, a negative cache_row0, bad ring fields (0 <= ring_shift < ring_size, ring_lo >= 0),
 * rows outside [0, cache_rows) (no ring: cache_row0 + M > cache_rows; ring: ring_lo + ring_size > cache_rows or cache_row0 + M >
 * ring_lo + ring_size). */
int rtv_attn_fp8_commit_kv8(const void* kv8, int world, int M, int H, void* k8, void* v8t, int cache_rows, int cache_row0,
                            int ring_lo, int ring_size, int ring_shift, rtv_stream_t stream);

/* rtv_dit_layer_proj (rtv_hip.h) for this mode: parts of RTV_PROJ_LN | RTV_PROJ_Q | RTV_PROJ_KV.  RTV_PROJ_Q projects, normalises
 * and rotates the local query rows as rtv_dit_layer_proj does.  RTV_PROJ_KV projects K | V of the local rows [row_begin, row_begin
 * + row_count) into the projection buffer and STAGES their codes into kv8 (world ranks; maxima into shadow->amax[layer]).
 * step->kv_k / kv_v / kv_row_stride are never read (kv_k and kv_v may be NULL); the cache is not written.
 * Refused before any launch: what rtv_dit_layer_proj refuses, a null shadow or one without its arrays or cache_rows, non-finite or
 * non-positive scales, a null or misaligned kv8, world <= 0, M % world != 0, local rows that are not inside one rank's segment. */
int rtv_dit_layer_proj_attn_fp8_only(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* step, int layer,
                                     int parts, int world, void* kv8, const rtv_attn_fp8_shadow* shadow, void* workspace,
                                     size_t workspace_bytes, rtv_stream_t stream);

/* COMMIT of a gathered kv8 into shadow->k8[layer] / v8t[layer] with the row and ring fields of the step: what a rank runs where a
 * pass stops behind the exchange (the last layer of a kv_only pass), as rtv_dit_quantize_block_attn_fp8 is for the shadow mode.
 * Refused before any launch: a null argument or shadow, a layer out of range, a layer without k8 / v8t, an empty token grid, and
 * what rtv_attn_fp8_commit_kv8 refuses. */
int rtv_dit_commit_block_attn_fp8_only(const rtv_dit_config* cfg, const rtv_dit_step* step, int layer, int world, const void* kv8,
                                       const rtv_attn_fp8_shadow* shadow, rtv_stream_t stream);

/* rtv_dit_layer_rest_attn_fp8 (rtv_hip_attn_fp8_cp.h) for this mode: commits the gathered kv8 as above, attends the local rows
 * with rtv_attn_fwd_fp8 - or, when step->attn_kv_splits > 1, with rtv_attn_fwd_fp8_split on the partial buffer of the workspace,
 * under the same bounds check (attn_kv_splits <= rtv_dit_config.max_attn_kv_splits) - and runs the rest of the layer.
 * step->kv_k / kv_v are never read.
 * Refused before any launch: what rtv_dit_layer_rest refuses, what the commit refuses, an attention window outside [0,
 * cache_rows), and a step whose attn_kv_splits the workspace was not planned for - never a bf16 or an unsplit run in its place. */
int rtv_dit_layer_rest_attn_fp8_only(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* step, int layer,
                                     int world, const void* kv8, const rtv_attn_fp8_shadow* shadow, void* workspace,
                                     size_t workspace_bytes, rtv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
