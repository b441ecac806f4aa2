// The e4m3 conversion of the dynamic activation quantisers (torchao's Float8DynamicActivationFloat8WeightConfig restated):
//   s = max(max |x|, 1e-12) * fp32(1 / 448),   q = e4m3(clamp(x / s, -448, 448)),
// the maximum taken over the tensor (gemm_fp8.hip) or over a row (fp8_rows.hip).
#pragma once
#include <cmath>

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

// The running maximum of a 256-thread workgroup's |x| into a device float kept as its bits, in two steps around a __syncthreads()
// of the caller's: every wave leaves its maximum in s_max[4], then ONE thread folds the four and raises *amax.  Used by the e4m3 K
// writer (kv_fp8.hip) and the recentre kernel (kv_fp8_center.hip); the quantisers of attn_fp8.hip / kv_fp8.hip write the same tail
// out: on these helpers their launches measured slower (profiles/r26_kv_fp8_fold_ab.txt).
__device__ __forceinline__ void block_max_stage(float v, float* s_max) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = v;
}
__device__ __forceinline__ void block_max_commit(const float* s_max, unsigned* amax) {
  // non-negative floats order like their bit patterns; most workgroups find the maximum already there and only read
  const unsigned bits = __float_as_uint(fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3])));
  if (bits > __atomic_load_n(amax, __ATOMIC_RELAXED)) atomicMax(amax, bits);
}

// what every launcher asks of a quantisation scale
inline bool good_scale(float s) { return std::isfinite(s) && s > 0.f; }

}  // namespace rtv
