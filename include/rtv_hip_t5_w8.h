/* Text encoder with e4m3 WEIGHT STORAGE (opt-in; WanTextEncoder.enable_fp8_weights): a weight-only fp8 GEMM shaped for the 32 - 128
 * rows of a prompt, and the encoder entry that runs its five Linears per layer on it.  A header of its own, like rtv_hip_lora.h:
 * nothing here changes a signature or a struct of rtv_hip.h and RTV_ABI_VERSION stays as it is.  Same conventions as rtv_hip.h:
 * device pointers unless stated, 0 = success, non-zero = failure with the reason in rtv_last_error().
 *
 * Arithmetic.  For x [M, K] bf16 and W [N, K] bf16:
 *   s_w[n] = max(max_k |W[n, k]|, 1e-12) * fp32(1 / 448)         the per-row rule of rtv_quantize_fp8_rows (rtv_hip_fp8_rows.h),
 *   c[n,k] = e4m3fn(clamp(W[n, k] / s_w[n], -448, 448))          which is also the quantiser: the codes are made by it
 *   y[m,n] = bf16( fp32_acc( sum_k x[m, k] * value(c[n, k]) ) * s_w[n] )
 * value(c) is the exact e4m3 value held in bf16 (3 mantissa bits and e4m3's exponent range fit inside bf16: signed zeros and the
 * subnormal codes included), the products are bf16 x bf16 on the MFMA with fp32 accumulation, and there is one fp32 multiplication
 * by the scale and one rounding to bf16 - the rounding point of the bf16 path.  Activations are NOT quantised: the only error of the
 * mode is the rounding of the weights. */
#ifndef RTV_HIP_T5_W8_H
#define RTV_HIP_T5_W8_H
#include <stddef.h>

#include "rtv_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* C = bf16((A . value(Wq)^T)[m, n] * w_row_scales[n]).  A bf16 [M][K], row stride lda elements; Wq e4m3 codes [N][K], row stride
 * ldw BYTES; w_row_scales float [N]; C bf16, transpose_out == 0: C[m * ldc + n], transpose_out == 1: C[n * ldc + m] (the V^T
 * form the encoder's attention kernel reads).
 *
 * A workgroup owns 64 output channels for at most 128 rows and a segment of K; it streams its codes once, 16 bytes per lane
 * straight to registers, and takes the rows from LDS.  M > 128 runs as further row chunks (which read the codes again).  K is cut
 * into segments by a plan that is a function of (N, K) ONLY - not of M, not of the device: the segments' fp32 partial sums go
 * to slabs in `workspace` and a second kernel adds them in ascending segment order (no atomics).  Row m of the output therefore
 * depends on row m of A alone, and a row has the same bits in every launch that contains it.
 *
 * Refused before any launch: a null pointer; M <= 0 or M % 32; K <= 0 or K % 128; N <= 0 or N % 16; a stride below the row it
 * strides (lda < K, ldw < K, ldc < N or < M when transposed); lda % 8, ldw % 16, ldc % 4 (not transposed); A, Wq or workspace not
 * 16-byte aligned, C not 8-byte (transposed: 2-byte) aligned, scales not 16-byte aligned; transpose_out outside 0 / 1; a workspace
 * below rtv_gemm_w8_workspace_bytes(M, N, K) (0 where the plan does not cut K: workspace may then be NULL). */
size_t rtv_gemm_w8_workspace_bytes(int M, int N, int K);
int rtv_gemm_w8(const void* A, int lda, const void* Wq, int ldw, const float* w_row_scales, void* C, int ldc, int transpose_out,
                int M, int N, int K, void* workspace, size_t workspace_bytes, rtv_stream_t stream);
/* The plan: the number of K segments for (N, K), 0 for an N or K rtv_gemm_w8 refuses.  Segment s covers the 128-wide K steps
 * [s * steps / segments, (s + 1) * steps / segments), steps = K / 128. */
int rtv_gemm_w8_segments(int N, int K);

/* rtv_t5_layer_weights (rtv_hip.h) with the five matrices as e4m3 codes [N][K] (dense, row stride K bytes, 16-byte aligned) and
 * their float row scales [N]; the norm weights and pos_bias as there. */
typedef struct {
  const void* norm1_w;            /* bf16 [dim] */
  const void* qk_q;               /* e4m3 [2*dim_attn][dim]: attn.q.weight rows, then attn.k.weight rows */
  const void* qk_s;               /* float [2*dim_attn] */
  const void* v_q;                /* e4m3 [dim_attn][dim] */
  const void* v_s;                /* float [dim_attn] */
  const void* o_q;                /* e4m3 [dim][dim_attn] */
  const void* o_s;                /* float [dim] */
  const void* norm2_w;            /* bf16 [dim] */
  const void* gate_fc1_q;         /* e4m3 [2*dim_ffn][dim]: ffn.gate.0.weight rows, then ffn.fc1.weight rows */
  const void* gate_fc1_s;         /* float [2*dim_ffn] */
  const void* fc2_q;              /* e4m3 [dim][dim_ffn] */
  const void* fc2_s;              /* float [dim] */
  const void* pos_bias;           /* float32 [num_heads][2*max_len-1], as rtv_t5_layer_weights.pos_bias */
} rtv_t5_layer_weights_w8;
typedef struct {
  const void* token_embedding;    /* bf16 [vocab][dim]: the table stays bf16 */
  const void* final_norm_w;       /* bf16 [dim] */
  const rtv_t5_layer_weights_w8* layers;   /* host array [num_layers] */
  int max_len;
} rtv_t5_weights_w8;

/* rtv_t5_workspace_bytes / rtv_t5_encode (rtv_hip.h) on those weights: the same embedding, norm, attention, GEGLU and add kernels
 * and the same fp32 residual stream; the five Linears of a layer run on rtv_gemm_w8 (V^T with transpose_out = 1).  dim, dim_attn
 * and dim_ffn must be multiples of 128 here. */
size_t rtv_t5_w8_workspace_bytes(const rtv_t5_config* cfg, int seq_len);
int rtv_t5_encode_w8(const rtv_t5_config* cfg, const rtv_t5_weights_w8* w, const int* ids, int seq_len, int out_rows,
                     void* workspace, size_t workspace_bytes, void* out, rtv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
