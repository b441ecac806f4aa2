/* LoRA side of librtv_hip.so: low-rank adapters merged into a weight matrix of the DiT in place.  Same conventions as rtv_hip.h:
 * device pointers unless stated, 0 = success, non-zero = failure with the reason in rtv_last_error(), every launch goes to
 * `stream`.
 *
 * A header of its own for the reason rtv_hip_io.h is one: the declarations were added without a new ABI revision, nothing here
 * changes a struct layout of rtv_hip.h and RTV_ABI_VERSION stays as it is. */
#ifndef RTV_HIP_LORA_H
#define RTV_HIP_LORA_H
#include <stdint.h>

#include "rtv_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Adapters one rtv_lora_merge call can take (the table travels by value with the launch) and the largest rank of one of them. */
#define RTV_LORA_MAX_ADAPTERS 4
#define RTV_LORA_MAX_RANK 256

/* One adapter of one matrix: A bf16 [rank][K] ("down", dense, 16-byte aligned), B bf16 [N][rank] ("up", dense), `scale` already
 * holds alpha / rank and the user's strength. */
typedef struct {
  const void* A;
  const void* B;
  int rank;
  float scale;
} rtv_lora_adapter;

/* W[n][k] = bf16_rne( float(base[n][k]) + sum_a scale_a * sum_j float(B_a[n][j]) * float(A_a[j][k]) ),  n < N, k < K, in ONE launch.
 * The inner sums accumulate in fp32 on bf16 MFMAs, every adapter in an accumulator of its own; its scale is applied in fp32
 * before the adapters are added (no scale is folded into a bf16 operand); the sum is rounded to bf16 once.  An element whose
 * adapter sum is exactly zero (count == 0, scale == 0) keeps the bits of base.
 *
 * base / W: bf16 with row strides ldb / ldw in elements (>= K); K and both strides are multiples of 8 and both pointers 16-byte
 * aligned.  N is any positive number, a rank any value in 1 .. RTV_LORA_MAX_RANK (padded to the MFMA step with zeros inside).
 * base == W is allowed: every thread reads the elements it owns before it writes them; any other overlap is not.  A row range of
 * a wider matrix is the same call with offset pointers.  `adapters` is a HOST array of `count` entries (NULL when count == 0).
 * No allocation and no synchronisation inside.
 * Refused before any launch: a null pointer, non-positive N or K, a misaligned pointer or stride, a stride below K, count outside
 * 0 .. RTV_LORA_MAX_ADAPTERS, a rank outside 1 .. RTV_LORA_MAX_RANK, a non-finite scale. */
int rtv_lora_merge(const void* base, int ldb, void* W, int ldw, int N, int K, const rtv_lora_adapter* adapters, int count,
                   rtv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
