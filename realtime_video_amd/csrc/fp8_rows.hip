// Per-row dynamic e4m3 quantisation for the fp8 Linears with per-row scales (include/rtv_hip_fp8_rows.h; torchao's PerRow
// granularity restated, tests/fp8_rows_oracle.py):
//   s[m] = max(max_k |x[m, k]|, 1e-12) * fp32(1 / 448),   q[m, k] = e4m3(clamp(x[m, k] / s[m], -448, 448)).
// A row's scale needs that row alone, so the quantiser is ONE pass: the row is read once into registers, |x| is reduced over the
// lanes that share the row, and the same registers are converted and stored.  No memset, no atomics (the per-tensor quantiser of
// gemm_fp8.hip is a memset and two kernels, and reads the activations twice).  Two kernels here:
//   quantize_fp8_rows_kernel           x bf16 -> codes + scales; a wave per row up to 2048 columns, a workgroup per row above
//   layernorm_modulate_fp8_rows_kernel elementwise.hip's layernorm_modulate_kernel with this quantiser behind its bf16 rounding
// The GEMM that consumes the codes is gemm_fp8_rows.hip.
#include "fp8_quant.h"
#include "ln_row.h"
#include "rtv_common.h"
#include "rtv_internal.h"

namespace rtv {

namespace f8r {
constexpr int THREADS = EW_THREADS;

// max over the workgroup's 4 waves (`red`: 4 floats nothing else uses - each kernel calls this once)
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
}  // namespace f8r

// ------------------------------------------------------------------ row quantiser
// WAVE: a wave per row (4 rows per workgroup, no LDS, no barrier); else a workgroup per row.  The G lanes of a row take its 16-byte
// chunks G apart, MAXC of them each: rows of up to G * 8 * MAXC elements.
template <int MAXC, bool WAVE>
__global__ __launch_bounds__(f8r::THREADS) void quantize_fp8_rows_kernel(const uint16_t* __restrict__ x, int64_t ld, int M, int d,
                                                                        uint8_t* __restrict__ q, int64_t ldq,
                                                                        float* __restrict__ row_scales) {
  using namespace f8r;
  constexpr int G = WAVE ? 64 : THREADS;
  const int lane = WAVE ? (threadIdx.x & 63) : threadIdx.x;
  const int row = WAVE ? blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6) : blockIdx.x;
  if (row >= M) return;   // (WAVE only: whole waves leave, and that form has no barrier)
  const int nchunks = d >> 3;
  const uint16_t* xr = x + (int64_t)row * ld;
  u32x4 raw[MAXC];
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + i * G;
    if (c < nchunks) {
      raw[i] = *(const u32x4*)(xr + c * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t u = raw[i][j];
        m = fmaxf(m, fmaxf(fabsf(__uint_as_float(u << 16)), fabsf(__uint_as_float(u & 0xffff0000u))));
      }
    }
  }
  if constexpr (WAVE) {
    m = wave_max(m);
  } else {
    __shared__ float red[4];
    m = block_max(m, red);
  }
  const float scale = fp8_scale(m);
  if (lane == 0) row_scales[row] = scale;
  uint8_t* qr = q + (int64_t)row * ldq;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + i * G;
    if (c < nchunks) {
      float v[8];
      unpack_bf16x8(raw[i], v);
      *(u32x2*)(qr + c * 8) = quantize8(v, scale);
    }
  }
}

// ------------------------------------------------------------------ LayerNorm (+ modulation) + row quantiser, a workgroup per row
// layernorm_modulate_kernel's row (ln_row.h: same reductions, same rounding points) up to the value it would store; that value is
// rounded to bf16 as the store would round it, kept in registers, and quantised as quantize_fp8_rows_kernel quantises the stored row.
__global__ __launch_bounds__(f8r::THREADS) void layernorm_modulate_fp8_rows_kernel(
    const bf16_t* __restrict__ x, uint8_t* __restrict__ q, int64_t ldq, float* __restrict__ row_scales, int d, float eps,
    const bf16_t* __restrict__ shift, const bf16_t* __restrict__ scale, int frame_stride, int rows_per_frame, int row_offset,
    const bf16_t* __restrict__ weight, const bf16_t* __restrict__ bias) {
  using namespace f8r;
  __shared__ float red[8];
  __shared__ float redm[4];
  const int row = blockIdx.x;
  const int nchunks = d >> 3;
  float v[EW_MAXC][8];
  float m = 0.f;
  layernorm_row(x, d, eps, shift, scale, frame_stride, rows_per_frame, row_offset, weight, bias, red, [&](int i, int, const float* o) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[i][j] = round_bf16(o[j]);   // the bf16 value layernorm_modulate_kernel stores: what the Linear's input is
      m = fmaxf(m, fabsf(v[i][j]));
    }
  });
  const float qs = fp8_scale(block_max(m, redm));
  if (threadIdx.x == 0) row_scales[row] = qs;
  uint8_t* qr = q + (int64_t)row * ldq;
#pragma unroll
  for (int i = 0; i < EW_MAXC; ++i) {
    int c = threadIdx.x + i * THREADS;
    if (c < nchunks) *(u32x2*)(qr + c * 8) = quantize8(v[i], qs);
  }
}

}  // namespace rtv

using namespace rtv;

extern "C" int rtv_quantize_fp8_rows(const void* x, int64_t ld, int M, int d, void* q, int64_t ldq, float* row_scales,
                                     rtv_stream_t stream) {
  if (!x || !q || !row_scales) return set_error(-1, "quantize_fp8_rows: null pointer");
  if (M <= 0 || d <= 0) return set_error(-1, "quantize_fp8_rows: empty tensor");
  if ((d & 15) || (ld & 7) || (ldq & 7) || ld < d || ldq < d)
    return set_error(-1, "quantize_fp8_rows: d must be a multiple of 16, strides multiples of 8 and >= d");
  if (((uintptr_t)x & 15) || ((uintptr_t)q & 7)) return set_error(-1, "quantize_fp8_rows: x must be 16-byte aligned, q 8-byte aligned");
  if (d > f8r::THREADS * 8 * 7) return set_error(-1, "quantize_fp8_rows: d must be <= 14336");
  hipStream_t s = (hipStream_t)stream;
  const uint16_t* xp = (const uint16_t*)x;
  uint8_t* qp = (uint8_t*)q;
  ProfScope prof(PROF_MISC, s, 0.0);
  if (d <= 64 * 8 * 4)
    hipLaunchKernelGGL((quantize_fp8_rows_kernel<4, true>), dim3((M + 3) / 4), dim3(f8r::THREADS), 0, s, xp, ld, M, d, qp, ldq, row_scales);
  else if (d <= f8r::THREADS * 8 * 3)
    hipLaunchKernelGGL((quantize_fp8_rows_kernel<3, false>), dim3(M), dim3(f8r::THREADS), 0, s, xp, ld, M, d, qp, ldq, row_scales);
  else
    hipLaunchKernelGGL((quantize_fp8_rows_kernel<7, false>), dim3(M), dim3(f8r::THREADS), 0, s, xp, ld, M, d, qp, ldq, row_scales);
  return check_launch("quantize_fp8_rows");
}

extern "C" int rtv_layernorm_modulate_fp8_rows(const void* x, void* q, int64_t ldq, float* row_scales, int M, int d, float eps,
                                               const void* shift, const void* scale, int frame_stride, int rows_per_frame,
                                               int row_offset, const void* weight, const void* bias, rtv_stream_t stream) {
  if (M <= 0) return 0;
  if (!x || !q || !row_scales) return set_error(-1, "layernorm_modulate_fp8_rows: null pointer");
  if (d % 16 || d > f8r::THREADS * 8 * EW_MAXC) return set_error(-1, "layernorm_modulate_fp8_rows: d must be a multiple of 16 and <= 8192");
  if ((ldq & 7) || ldq < d || ((uintptr_t)x & 15) || ((uintptr_t)q & 7))
    return set_error(-1, "layernorm_modulate_fp8_rows: ldq must be a multiple of 8 and >= d, x 16-byte aligned, q 8-byte aligned");
  if ((shift == nullptr) != (scale == nullptr)) return set_error(-1, "layernorm_modulate_fp8_rows: shift and scale go together");
  if ((weight == nullptr) != (bias == nullptr)) return set_error(-1, "layernorm_modulate_fp8_rows: weight and bias go together");
  if (weight && scale) return set_error(-1, "layernorm_modulate_fp8_rows: affine and modulation are exclusive");
  if (scale && (rows_per_frame <= 0 || frame_stride % 8)) return set_error(-1, "layernorm_modulate_fp8_rows: bad frame geometry");
  ProfScope prof(PROF_LN, (hipStream_t)stream, M * (double)d * 3);
  hipLaunchKernelGGL(layernorm_modulate_fp8_rows_kernel, dim3(M), dim3(f8r::THREADS), 0, (hipStream_t)stream, (const bf16_t*)x,
                     (uint8_t*)q, ldq, row_scales, d, eps, (const bf16_t*)shift, (const bf16_t*)scale, frame_stride, rows_per_frame,
                     row_offset, (const bf16_t*)weight, (const bf16_t*)bias);
  return check_launch("layernorm_modulate_fp8_rows");
}
