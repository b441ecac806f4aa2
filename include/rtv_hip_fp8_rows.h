/* fp8 Linears with PER-ROW scales (rtv_dit_config.use_fp8 == 2, rtv_dit_weights.fp8_row_scales; include/rtv_hip.h): the three
 * entry points the mode adds.  A header of its own, like rtv_hip_io.h / rtv_hip_lora.h / rtv_hip_cross_fold.h: nothing here
 * changes a signature of rtv_hip.h (the trailing field fp8_row_scales of rtv_dit_weights is ABI revision 105 there).
 *
 * Arithmetic: torchao's Float8DynamicActivationFloat8WeightConfig(granularity=PerRow()), restated from its published source with
 * the conventions of the per-tensor mode (rtv_quantize_fp8 / rtv_gemm_fp8).  For x [M, K] and W [N, K], both bf16:
 *   s_x[m] = max(max_k |x[m, k]|, 1e-12) * fp32(1 / 448),   s_w[n] the same over row n of W (one scale per output channel),
 *   q(t)   = e4m3fn(clamp(t / s, -448, 448)), round to nearest even, evaluated in fp32,
 *   y[m,n] = bf16(acc[m, n] * s_x[m] * s_w[n] + bias[n]) with fp32 accumulation (two fp32 multiplications, left to right),
 *            then rtv_gemm's bf16 epilogue.
 * A row's codes and scale depend on that row alone: a rank that holds a subset of the rows takes the decisions the unsharded
 * forward takes.  PARITY WITH torchao ITSELF IS UNPINNED, as for the per-tensor mode (no golden from it can be minted offline);
 * the pin is the restatement in tests/fp8_rows_oracle.py. */
#ifndef RTV_HIP_FP8_ROWS_H
#define RTV_HIP_FP8_ROWS_H
#include "rtv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* x [M, d] bf16 (row stride ld elements) -> q [M, d] e4m3 (row stride ldq bytes) and row_scales[m] = s_x[m] (device floats).
 * One pass: a row stays in registers between the |x| reduction and the conversion; no memset, no atomics, no scratch.
 * d % 16 == 0, d <= 14336, ld % 8 == 0, ldq % 8 == 0, 16-byte aligned x, 8-byte aligned q. */
int rtv_quantize_fp8_rows(const void* x, int64_t ld, int M, int d, void* q, int64_t ldq, float* row_scales, rtv_stream_t stream);

/* rtv_layernorm_modulate (same arguments, same rounding points) followed by rtv_quantize_fp8_rows on its bf16 result, in one
 * kernel and bit for bit: the normalised value is rounded to bf16 first and that bf16 value is quantised.  x [M, d] contiguous
 * rows; q / ldq / row_scales as above.  d % 16 == 0, d <= 8192. */
int rtv_layernorm_modulate_fp8_rows(const void* x, void* q, int64_t ldq, float* row_scales, int M, int d, float eps,
                                    const void* shift, const void* scale, int frame_stride, int rows_per_frame, int row_offset,
                                    const void* weight, const void* bias, rtv_stream_t stream);

/* C[M,N] bf16 = epilogue((A . W^T)[m, n] * a_row_scales[m] * w_row_scales[n]): rtv_gemm_fp8 with one scale per row of A and
 * per row of W (device floats, M and N of them; w_row_scales 16-byte aligned).  A launch over a row range of a weight passes the
 * matching slice of its scales.  Everything else - operands, K % 128 == 0, N % 8 == 0, epilogue arguments, split-K workspace -
 * is rtv_gemm_fp8's. */
int rtv_gemm_fp8_rows(const void* A, int lda, const void* W, int ldw, const float* a_row_scales, const float* w_row_scales,
                      void* C, int ldc, int M, int N, int K, const void* bias, int act, const void* gate, int gate_stride,
                      int rows_per_frame, int row_offset, const void* residual, int ldr, rtv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
