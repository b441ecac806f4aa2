/* LoRA side of librtv_hip.so, second part: the two arithmetic forms rtv_lora_merge (rtv_hip_lora.h) cannot express - a dense
 * delta beside the low-rank pairs, and DoRA's row-normalised merge.  The conventions of rtv_hip_lora.h apply: device pointers
 * unless stated, 0 = success, non-zero = failure with the reason in rtv_last_error(), every refusal comes before any launch, no
 * allocation and no synchronisation inside, base == W is allowed (any other overlap is not), a row range of a wider matrix is the
 * same call with offset pointers.
 *
 * A header of its own for the reason rtv_hip_lora.h is one: the declarations were added without a new ABI revision, nothing here
 * changes rtv_lora_adapter or a struct layout of rtv_hip.h and RTV_ABI_VERSION stays as it is. */
#ifndef RTV_HIP_LORA_EXT_H
#define RTV_HIP_LORA_EXT_H
#include <stddef.h>
#include <stdint.h>

#include "rtv_hip.h"
#include "rtv_hip_lora.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One term of one matrix: a low-rank pair (A bf16 [rank][K] "down", dense, 16-byte aligned; B bf16 [N][rank] "up", dense; `scale`
 * holds alpha / rank and the user's strength), a dense delta (diff bf16 [N][K] with row stride ldd in elements, a multiple of 8
 * and >= K, 16-byte aligned; `diff_scale` the user's strength), or both.  A term with rank == 0 and A == B == NULL has a diff
 * only; a term with diff == NULL a pair only (ldd and diff_scale are then ignored). */
typedef struct {
  const void* A;
  const void* B;
  int rank;
  float scale;
  const void* diff;
  int ldd;
  float diff_scale;
} rtv_lora_term;

/* W[n][k] = bf16_rne( float(base[n][k]) + sum_t ( scale_t * sum_j float(B_t[n][j]) * float(A_t[j][k]) + diff_scale_t * float(diff_t[n][k]) ) )
 * for n < N, k < K, in ONE launch.  Each low-rank sum accumulates in fp32 on bf16 MFMAs in an accumulator of its own and is
 * scaled in fp32; the scaled sums are added in term order, then the scaled diffs in term order; the total is rounded to bf16
 * once.  An element whose total delta is exactly zero keeps the bits of base.  With low-rank terms only the result is that of
 * rtv_lora_merge on the same operands, bit for bit.  `diff` is read in the copy layout beside base.  N = 1 merges a vector (a
 * bias, a norm weight).  base / W / K / strides as in rtv_lora_merge.  `terms` is a HOST array of `count` entries (NULL when
 * count == 0), count in 0 .. RTV_LORA_MAX_ADAPTERS.
 * Refused before any launch: everything rtv_lora_merge refuses, a term with neither part (or half a pair), a diff that is
 * misaligned or has a stride that is short or no multiple of 8, a non-finite diff_scale. */
int rtv_lora_merge_ex(const void* base, int ldb, void* W, int ldw, int N, int K, const rtv_lora_term* terms, int count,
                      rtv_stream_t stream);

/* Bytes of workspace rtv_lora_merge_dora needs for an N x K range: one fp32 per (row, 128-column tile), rounded up to 16 bytes.
 * 0 when N or K is not positive. */
size_t rtv_lora_dora_workspace_bytes(int N, int K);

/* DoRA (weight-decomposed low-rank adaptation), PEFT's definition - the magnitude vector has one entry per OUTPUT row and the
 * norm runs over the input width K.  With every intermediate value in fp32:
 *   V[n][k] = base[n][k] + factor * (B A)[n][k]        nrm[n] = sqrt(sum_k V[n][k]^2)        g[n] = float(mag[n]) / nrm[n]
 *   W[n][k] = bf16_rne( base[n][k] + strength * (g[n] * V[n][k] - base[n][k]) )
 * `mag` is bf16 [N] (2-byte aligned), `factor` is alpha / rank, `strength` blends between the base (0) and the DoRA weight (1).
 * strength == 0 and rows with nrm == 0 keep the bits of base, as does every element whose delta is exactly zero.
 * Two launches: the first writes one partial sum of V^2 per (row, 128-column tile) into `workspace` (a tree over the tile's
 * columns, no atomics), the second adds a row's partials in a fixed order (four runs of consecutive tiles, each in tile order,
 * then the four sums in order), recomputes V and stores.  The same inputs give the same bits on every call.  A / B / rank /
 * base / W / K / strides as in rtv_lora_merge; `workspace` is 16-byte aligned device memory of at least
 * rtv_lora_dora_workspace_bytes(N, K) bytes and is overwritten.
 * Refused before any launch: everything rtv_lora_merge refuses of one adapter, a null or misaligned mag, a workspace that is
 * null, misaligned or too small, a non-finite factor or strength. */
int rtv_lora_merge_dora(const void* base, int ldb, void* W, int ldw, int N, int K, const void* A, const void* B, int rank,
                        float factor, const void* mag, float strength, void* workspace, size_t workspace_bytes, rtv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
