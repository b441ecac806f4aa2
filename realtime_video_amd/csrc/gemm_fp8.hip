// FP8 (OCP e4m3) projection GEMM + dynamic per-tensor activation quantisation for gfx950.
//
// Mirrors the reference's optional fp8 weight path: release_server.py:179-182 runs
//   torchao.quantize_(transformer, Float8DynamicActivationFloat8WeightConfig(granularity=PerTensor()))
// i.e. every nn.Linear computes  y = bf16( (q(x) . q(W)^T) * s_x * s_w + bias )  with
//   s = max|t| / 448 (fp32, over the WHOLE tensor, clamped to >= 1e-12),  q(t) = e4m3( clamp(t / s, -448, 448) ),
// weights quantised once, activations per call ("dynamic"), products accumulated in fp32 (torch._scaled_mm).  torchao is
// a third-party dependency that is not part of the reference tree (unpinned in its pyproject): the algorithm above is
// restated from its published source; oracle/wan_oracle.py carries the same restatement (parity for this mode is
// pinned to that restatement only).
//
// The GEMM kernel is gemm_fp8_body.h (gemm8.hip's 256x256 ping-pong schedule on 128-byte K-tiles, shared with the per-row variant
// in gemm_fp8_rows.hip) with the scalar-product de-quantise step.
#include "fp8_quant.h"
#include "gemm_fp8_body.h"

namespace rtv {

namespace gf8 {
struct Fp8Args {
  const uint8_t* A;      // [M][lda] e4m3
  const uint8_t* W;      // [N][ldw] e4m3
  int lda, ldw;          // bytes
  const float* a_scale;  // device: s_x of this call (written by the quantisation kernel)
  float w_scale;         // s_w
};
}  // namespace gf8

__global__ __launch_bounds__(gf8::THREADS, 2) void gemm_fp8_kernel(GemmParams p, gf8::Fp8Args f, SplitArgs sp) {
  // de-quantise: (q(x) . q(W)^T) * s_x * s_w
  gf8::gemm_body(p, f, sp, [&](f32x16 (&acc)[4][2], int, int) {
    const float sc = f.a_scale[0] * f.w_scale;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] *= sc;
  });
}

// ------------------------------------------------------------------ dynamic per-tensor activation quantisation
// pass 1: amax_bits = max over the tensor of |x| (non-negative floats order like their bit patterns -> integer atomicMax).
// One workgroup per group of rows, 16-byte chunks strided over the threads (no integer division in the loop).
__global__ __launch_bounds__(256) void absmax_bf16_kernel(const uint16_t* __restrict__ x, int64_t ld, int M, int d,
                                                         unsigned* __restrict__ amax_bits) {
  const int cpr = d >> 3;  // 16-byte chunks per row
  float m = 0.f;
  for (int r = blockIdx.x; r < M; r += gridDim.x) {
    const uint16_t* xr = x + (int64_t)r * ld;
    for (int c = threadIdx.x; c < cpr; c += 256) {
      const u32x4 raw = *(const u32x4*)(xr + c * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t u = raw[j];
        m = fmaxf(m, fmaxf(fabsf(__builtin_bit_cast(float, u << 16)), fabsf(__builtin_bit_cast(float, u & 0xffff0000u))));
      }
    }
  }
  __shared__ float red[4];
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0)   // one same-address atomic per workgroup
    atomicMax(amax_bits, __builtin_bit_cast(unsigned, fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

// pass 2: scale = max(amax, 1e-12) / 448 ; q = e4m3(clamp(x / scale, -448, 448)) ; also publishes `scale`
__global__ __launch_bounds__(256) void quantize_fp8_kernel(const uint16_t* __restrict__ x, int64_t ld, int M, int d,
                                                          const unsigned* __restrict__ amax_bits, uint8_t* __restrict__ q,
                                                          int64_t ldq, float* __restrict__ scale_out) {
  const float scale = fp8_scale(__builtin_bit_cast(float, amax_bits[0]));
  if (blockIdx.x == 0 && threadIdx.x == 0) scale_out[0] = scale;
  const int cpr = d >> 3;
  for (int r = blockIdx.x; r < M; r += gridDim.x) {
    const uint16_t* xr = x + (int64_t)r * ld;
    uint8_t* qr = q + (int64_t)r * ldq;
    for (int c = threadIdx.x; c < cpr; c += 256) {
      const u32x4 raw = *(const u32x4*)(xr + c * 8);
      float v[8];
      unpack_bf16x8(raw, v);
      *(u32x2*)(qr + c * 8) = quantize8(v, scale);
    }
  }
}

int launch_quantize_fp8(const uint16_t* x, int64_t ld, int M, int d, uint8_t* q, int64_t ldq, float* scale_out,
                        unsigned* amax_scratch, hipStream_t stream) {
  if (M <= 0 || d <= 0) return set_error(-1, "quantize_fp8: empty tensor");
  if ((d & 15) || (ld & 7) || (ldq & 7)) return set_error(-1, "quantize_fp8: d must be a multiple of 16, strides of 8");
  if (hipMemsetAsync(amax_scratch, 0, sizeof(unsigned), stream) != hipSuccess) return set_error(-1, "quantize_fp8: memset failed");
  const int blocks = M < 1024 ? M : 1024;
  ProfScope prof(PROF_MISC, stream, 0.0);
  hipLaunchKernelGGL(absmax_bf16_kernel, dim3(blocks), dim3(256), 0, stream, x, ld, M, d, amax_scratch);
  hipLaunchKernelGGL(quantize_fp8_kernel, dim3(blocks), dim3(256), 0, stream, x, ld, M, d, amax_scratch, q, ldq, scale_out);
  return check_launch("quantize_fp8");
}

int launch_gemm_fp8(GemmParams p, const uint8_t* A, int lda, const uint8_t* W, int ldw, const float* a_scale, float w_scale,
                    hipStream_t stream) {
  if (int st = gf8::prepare_launch(p, lda, ldw, "gemm_fp8")) return st;
  static LdsAttr lds_attr;   // per device (a second GPU used from this process needs the attribute as well)
  if (int st = ensure_dynamic_lds((const void*)gemm_fp8_kernel, gf8::LDS_BYTES, &lds_attr, "gemm_fp8")) return st;
  SplitArgs sp;
  int grid = 0;
  if (int st = plan_split_k(p.tiles_m * p.tiles_n, p.K / gf8::BK, true, &sp, &grid, stream)) return st;
  gf8::Fp8Args f{A, W, lda, ldw, a_scale, w_scale};
  ProfScope prof(PROF_GEMM, stream, 2.0 * p.M * (double)p.N * p.K);
  note_kernel(DK_GEMM_FP8_256x256);
  hipLaunchKernelGGL(gemm_fp8_kernel, dim3(grid), dim3(gf8::THREADS), gf8::LDS_BYTES, stream, p, f, sp);
  return check_launch("gemm_fp8");
}

}  // namespace rtv

using namespace rtv;

extern "C" int rtv_quantize_fp8(const void* x, int64_t ld, int M, int d, void* q, int64_t ldq, float* scale_out,
                                void* amax_scratch, rtv_stream_t stream) {
  if (!x || !q || !scale_out || !amax_scratch) return set_error(-1, "quantize_fp8: null pointer");
  return launch_quantize_fp8((const uint16_t*)x, ld, M, d, (uint8_t*)q, ldq, scale_out, (unsigned*)amax_scratch,
                             (hipStream_t)stream);
}

extern "C" int rtv_gemm_fp8(const void* A, int lda, const void* W, int ldw, const float* a_scale, float w_scale, void* C,
                            int ldc, int M, int N, int K, const void* bias, int act, const void* gate, int gate_stride,
                            int rows_per_frame, int row_offset, const void* residual, int ldr, rtv_stream_t stream) {
  if (!A || !W || !C || !a_scale) return set_error(-1, "gemm_fp8: null pointer");
  const GemmParams p = gemm_params(nullptr, lda, nullptr, ldw, C, ldc, M, N, K, bias, act, gate, gate_stride, rows_per_frame, row_offset,
                                   residual, ldr);
  return launch_gemm_fp8(p, (const uint8_t*)A, lda, (const uint8_t*)W, ldw, a_scale, w_scale, (hipStream_t)stream);
}
