/* The fp8 self-attention of rtv_hip_attn_fp8.h for context-parallel ranks: a KV split of the attention kernel, for launches whose
 * query grid cannot fill the chip (a rank's 5 heads x 19 query tiles), and fp8 forms of the sharded phases of rtv_hip.h that keep
 * the e4m3 shadow current behind the exchanges.  Opt-in.  Same conventions as rtv_hip.h: device pointers unless stated, 0 = success,
 * non-zero = failure with the reason in rtv_last_error(), every launch goes to `stream`, no allocation and no synchronisation
 * inside.
 *
 * A header of its own, like rtv_hip_attn_fp8_center.h: nothing here changes a signature or a layout of rtv_hip.h or of
 * rtv_hip_attn_fp8.h (rtv_dit_step, rtv_dit_config and rtv_attn_fp8_shadow are what they were), RTV_ABI_VERSION stays as it is,
 * and every older entry point issues exactly what it issued before.
 *
 * THE SPLIT (part of the ABI; tests/attn_fp8_split_cases.py is the restatement).
 *   Tile list of a workgroup (one head, 256 query rows): the 64-row STORAGE tiles of the window's first range, cut behind the
 *   workgroup's largest block-causal key limit, then those of the second range; ntiles of them, as rtv_attn_fwd_fp8 walks them.
 *   Range s of S works on the tiles j in [ntiles * s / S, ntiles * (s + 1) / S) of that list (integer division; the rule of the
 *   bf16 split, applied to storage tiles).  An empty range - more ranges than tiles, or a block-causal workgroup with few tiles -
 *   reads nothing and leaves (m, l, O) = (-1e30, 0, 0); so does a row whose keys in a range are all masked.
 *   Per range the arithmetic is that of rtv_attn_fwd_fp8: Q quantised per (row, head), scores times c = s_q * k_scale * scale *
 *   log2(e) in fp32, a reference point m at most 2^8 below the range's row maximum, l from the unrounded P, P rounded once to e4m3.
 *   A range leaves its UNNORMALISED fp32 O (without v_scale), m and l; m is in the row's scaled log2 domain, which is one domain
 *   for all ranges because c belongs to the row.
 *   Merge (a second kernel, ranges in ascending order, no atomics: the same input gives the same bits):
 *       m = max_s m_s,   w_s = 2^(m_s - m),   O = v_scale * sum_s w_s O_s / sum_s w_s l_s,   rounded once to bf16. */
#ifndef RTV_HIP_ATTN_FP8_CP_H
#define RTV_HIP_ATTN_FP8_CP_H
#include <stddef.h>
#include <stdint.h>

#include "rtv_hip_attn_fp8.h"
#ifdef __cplusplus
extern "C" {
#endif

/* rtv_attn_fwd_fp8 (same leading arguments, same checks) with the key window cut into kv_splits ranges as under THE SPLIT:
 * grid = rtv_attn_fwd_fp8's workgroups x kv_splits, then the merge.  kv_splits (1..16) is clamped to the number of storage tiles
 * the window touches; after clamping, 1 is the plain launch of rtv_attn_fwd_fp8, bit for bit, and needs no workspace.
 * workspace: rtv_attn_split_workspace_bytes(1, Lq, H, kv_splits) bytes (rtv_hip.h; the layout of the bf16 split:
 * float [S][H][Lq][128] then float [S][H][Lq][2]), 16-byte aligned.
 * Refused before any launch: everything rtv_attn_fwd_fp8 refuses, kv_splits outside 1..16, and - while the clamped kv_splits is
 * above 1 - a workspace that is missing, misaligned or too small. */
int rtv_attn_fwd_fp8_split(const void* q, const void* k8, const void* v8t, void* o, int Lq, int H, int cache_rows, int row0, int n0,
                           int row1, int n1, int64_t q_row_stride, int64_t o_row_stride, float scale, float k_scale, float v_scale,
                           int causal_block, int q_offset, int kv_splits, void* workspace, size_t workspace_bytes,
                           rtv_stream_t stream);

/* Quantise the physical rows of the LOGICAL block [cache_row0, cache_row0 + M) of step->kv_k[layer] / kv_v[layer] (`heads` heads,
 * row stride step->kv_row_stride; M = F * gh * gw, the whole block, whatever row range the step shards) into shadow->k8[layer] /
 * v8t[layer], whose shadow is dense over `heads` heads.  Honours the ring fields of the step (sink rows as they are, ring rows
 * rotated, at most one wrap).  What a rank runs once an exchange has delivered the other ranks' rows - rtv_dit_layer_rest_attn_fp8
 * and rtv_dit_layer_attn_hp_attn_fp8 do it themselves; the caller needs it where a pass stops behind the exchange (the last layer
 * of a kv_only pass).  Refused before any launch: a null argument or shadow, a layer or a head count (1..num_heads) out of range, an
 * empty token grid, bad ring fields. */
int rtv_dit_quantize_block_attn_fp8(const rtv_dit_config* cfg, const rtv_dit_step* step, int layer, int heads,
                                    const rtv_attn_fp8_shadow* shadow, rtv_stream_t stream);

/* rtv_dit_layer_rest for the row (all-gather) exchange with the self-attention in fp8: quantises the block's M rows of all
 * num_heads heads as above (every rank quantises the gathered rows itself), attends the local rows [row_begin, row_begin +
 * row_count) with rtv_attn_fwd_fp8 - or, when step->attn_kv_splits > 1, with rtv_attn_fwd_fp8_split on the partial buffer of the
 * workspace, under the bounds check of the bf16 split (attn_kv_splits <= rtv_dit_config.max_attn_kv_splits) - and runs the rest of
 * the layer.  rtv_dit_layer_proj, rtv_dit_begin, rtv_dit_head and rtv_dit_finish are used unchanged.
 * Refused before any launch: what rtv_dit_layer_rest refuses, a null shadow or one without its arrays or cache_rows, and a step
 * whose attn_kv_splits the workspace was not planned for - never a bf16 or an unsplit run in its place. */
int rtv_dit_layer_rest_attn_fp8(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* step, int layer,
                                const rtv_attn_fp8_shadow* shadow, void* workspace, size_t workspace_bytes, rtv_stream_t stream);

/* rtv_dit_layer_attn_hp for the head exchange with the self-attention in fp8: the same for the num_heads / world heads this rank
 * owns (step->kv_k / kv_v point at them); the shadow is dense over those heads.  rtv_dit_layer_rest_hp follows unchanged.  The
 * same refusals, and those of rtv_dit_layer_attn_hp. */
int rtv_dit_layer_attn_hp_attn_fp8(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* step, int layer,
                                   int world, const void* q_all, void* o_all, const rtv_attn_fp8_shadow* shadow, void* workspace,
                                   size_t workspace_bytes, rtv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
