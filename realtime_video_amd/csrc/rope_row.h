// What the wave-per-row RoPE kernels share: qk_norm_rope_cache_kernel (elementwise.hip) and its e4m3 form
// qk_norm_rope_k8_kernel<CPL, CENTER> (kv_fp8.hip).  The row body itself is written out in both: see the header of kv_fp8.hip.
#pragma once
#include "rtv_common.h"

namespace rtv {

// Make the compiler forget what it knows about a register-resident chunk: the row kernels unpack their raw bf16 chunks once per
// pass; without this the unpacked floats of the first pass are kept (CSE) for the later ones - 8 registers per chunk instead of 4 -
// and the kernels spill or lose occupancy.
__device__ __forceinline__ void launder(u32x4& v) {
  uint32_t a = v[0], b = v[1], c = v[2], e = v[3];
  asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(e));
  v[0] = a;
  v[1] = b;
  v[2] = c;
  v[3] = e;
}

constexpr int ROWS_PER_WG = 4;

// rotate the 4 complex pairs of one 8-element chunk by the (cos, sin) values in w[0..4)
__device__ __forceinline__ void rope8(float* x, const float2* w) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const float a = x[2 * t], b = x[2 * t + 1];
    x[2 * t] = a * w[t].x - b * w[t].y;
    x[2 * t + 1] = a * w[t].y + b * w[t].x;
  }
}

// chunks per lane for a row of d elements: the smallest compiled CPL with d <= CPL * 512
#define RTV_ROW_DISPATCH(d, CALL)      \
  do {                                  \
    if ((d) <= 1024) { CALL(2); }       \
    else if ((d) <= 2048) { CALL(4); }  \
    else if ((d) <= 5120) { CALL(10); } \
    else { CALL(16); }                  \
  } while (0)

}  // namespace rtv
