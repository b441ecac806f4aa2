// The e4m3 conversion of the dynamic activation quantisers (torchao's Float8DynamicActivationFloat8WeightConfig restated):
//   s = max(max |x|, 1e-12) * fp32(1 / 448),   q = e4m3(clamp(x / s, -448, 448)),
// the maximum taken over the tensor (gemm_fp8.hip) or over a row (fp8_rows.hip).
#pragma once
#include "rtv_common.h"

namespace rtv {

constexpr float FP8_MAX = 448.f;

// scale from max |x|: torch evaluates `amax / 448.0` (tensor / Python scalar) on the GPU as a multiplication by the fp32 reciprocal
__device__ __forceinline__ float fp8_scale(float amax) { return fmaxf(amax, 1e-12f) * (1.0f / FP8_MAX); }

// 8 floats -> 8 e4m3 codes (round to nearest even), 8 bytes
__device__ __forceinline__ u32x2 quantize8(const float* x, float scale) {
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = fminf(fmaxf(x[j] / scale, -FP8_MAX), FP8_MAX);
  int w0 = 0, w1 = 0;
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], w0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], w0, true);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], w1, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], w1, true);
  return u32x2{(uint32_t)w0, (uint32_t)w1};
}

}  // namespace rtv
