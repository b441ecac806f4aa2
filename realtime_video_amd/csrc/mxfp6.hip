// MXFP6 quantisers (include/rtv_hip_mxfp6.h; the OCP Microscaling conversion with the floor rule, tests/mxfp6_oracle.py):
//   per 32-element block  E = max(biased exponent of max|x| - 2, 0),  code = e2m3(x * 2^(127 - E)), nearest even, saturating at 7.5.
// (E is the header's clamp(floor(log2 amax) - 2, -127, 127) + 127: the fp32 exponent field of a bf16 value is floor(log2) + 127 for
// normal numbers, subnormal and zero maxima clamp to E = 0, and the largest finite exponent field, 254, gives E = 252.)
// They are mxfp4.hip's kernels with another value table and another packer: a lane holds 8 consecutive elements (one 16-byte chunk),
// the 4 lanes of a quad hold a block, and the block maximum is two lane exchanges.  A lane's 8 codes are 48 bits, so the two lanes
// of a pair own three dwords of the block's six: the even lane stores the first two (its 48 bits and the partner's low 16, one more
// lane exchange), the odd lane the third - whole dwords, assembled in registers.  Two kernels:
//   quantize_mxfp6_kernel            x bf16 -> codes + scales; a wave per row up to 2048 columns, a workgroup per row above
//   layernorm_modulate_mxfp6_kernel  elementwise.hip's layernorm_modulate_kernel with this quantiser behind its bf16 rounding
// The GEMM that consumes the codes is gemm_mxfp6.hip.
#include <string>

#include "../../include/rtv_hip_mxfp6.h"
#include "ln_row.h"
#include "rtv_common.h"
#include "rtv_internal.h"

namespace rtv {

namespace mx6 {
constexpr int THREADS = EW_THREADS;

// e2m3 magnitude code (5 bits) of 0 <= t < 8, round to nearest even, saturating.  The 32 magnitudes in increasing order are the
// multiples of 1/8 below 2 (codes 0-16: the subnormals and the first binade share a spacing), of 1/4 in [2, 4) (16-24) and of 1/2
// in [4, 8) (24-31), so the code is the nearest integer of t over the spacing plus the offset of the range; rintf rounds ties to
// the even integer, which is the even code in every range (the offsets are even), i.e. the even mantissa.  t * 8 is exact.
__device__ __forceinline__ uint32_t e2m3_mag(float t) {
  const float r = t < 2.f ? rintf(t * 8.f) : t < 4.f ? rintf(t * 4.f) + 8.f : fminf(rintf(t * 2.f) + 16.f, 31.f);
  return (uint32_t)r;
}

// The 8 values of this lane (bf16 values in fp32) -> their 8 codes as 48 bits, element j at bits [6 j, 6 j + 6); *E = the scale byte
// of the block this lane's quad holds.  Every lane of a quad must call this together (lanes without data pass zeros).
__device__ __forceinline__ uint64_t quantize_chunk(const float* v, uint32_t* E) {
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(v[j]));
  m = fmaxf(m, __shfl_xor(m, 1, 64));
  m = fmaxf(m, __shfl_xor(m, 2, 64));
  const int ex = (int)((__float_as_uint(m) >> 23) & 0xffu);
  const int eb = max(ex - 2, 0);
  *E = (uint32_t)eb;
  uint64_t w = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float t = ldexpf(fabsf(v[j]), 127 - eb);   // exact: a power-of-two scaling of a bf16 value, below 8 by construction
    w |= (uint64_t)(e2m3_mag(t) | ((__float_as_uint(v[j]) >> 26) & 32u)) << (6 * j);
  }
  return w;
}

// chunk c of a row (elements 8 c .. + 8) with its 48 bits w: chunks 2 p and 2 p + 1 (a lane pair) own the dwords 3 p .. 3 p + 2 of
// the row's codes.  Every lane of a pair must call this together (the exchange); `live` = the chunk is inside the row.
__device__ __forceinline__ void store_chunk(uint8_t* codes_row, uint8_t* scales_row, int c, bool live, uint64_t w, uint32_t E) {
  const uint32_t lo = (uint32_t)w, hi = (uint32_t)(w >> 32);   // hi: 16 bits
  const uint32_t partner_lo = __shfl_xor(lo, 1, 64);
  if (!live) return;
  uint32_t* d = (uint32_t*)codes_row + (c >> 1) * 3;
  if (c & 1) {
    d[2] = (lo >> 16) | (hi << 16);
  } else {
    d[0] = lo;
    d[1] = hi | (partner_lo << 16);
  }
  if ((c & 3) == 0) scales_row[RTV_MXFP6_SCALE_POS(c >> 2)] = (uint8_t)E;
}
}  // namespace mx6

// ------------------------------------------------------------------ row quantiser
// WAVE: a wave per row (4 rows per workgroup); else a workgroup per row.  The G lanes of a row take its 16-byte chunks G apart,
// MAXC of them each: rows of up to G * 8 * MAXC elements.  d % 32 == 0, so a quad's 4 chunks are inside the row or outside together.
template <int MAXC, bool WAVE>
__global__ __launch_bounds__(mx6::THREADS) void quantize_mxfp6_kernel(const uint16_t* __restrict__ x, int64_t ld, int M, int d,
                                                                     uint8_t* __restrict__ codes, int64_t ld_codes,
                                                                     uint8_t* __restrict__ scales, int64_t ld_scales) {
  using namespace mx6;
  constexpr int G = WAVE ? 64 : THREADS;
  const int lane = WAVE ? (threadIdx.x & 63) : threadIdx.x;
  const int row = WAVE ? blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6) : blockIdx.x;
  if (row >= M) return;   // (WAVE only: whole waves leave)
  const int nchunks = d >> 3;
  const uint16_t* xr = x + (int64_t)row * ld;
  u32x4 raw[MAXC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + i * G;
    raw[i] = c < nchunks ? *(const u32x4*)(xr + c * 8) : u32x4{0, 0, 0, 0};
  }
  uint8_t* cr = codes + (int64_t)row * ld_codes;
  uint8_t* sr = scales + (int64_t)row * ld_scales;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + i * G;
    float v[8];
    unpack_bf16x8(raw[i], v);
    uint32_t E;
    const uint64_t w = quantize_chunk(v, &E);
    store_chunk(cr, sr, c, c < nchunks, w, E);
  }
}

// ------------------------------------------------------------------ LayerNorm (+ modulation) + quantiser, a workgroup per row
// layernorm_modulate_kernel's row (ln_row.h: same reductions, same rounding points) up to the value it would store; that value is
// rounded to bf16 as the store would round it, kept in registers, and quantised as quantize_mxfp6_kernel quantises the stored row.
__global__ __launch_bounds__(mx6::THREADS) void layernorm_modulate_mxfp6_kernel(
    const bf16_t* __restrict__ x, uint8_t* __restrict__ codes, int64_t ld_codes, uint8_t* __restrict__ scales, int64_t ld_scales, int d,
    float eps, const bf16_t* __restrict__ shift, const bf16_t* __restrict__ scale, int frame_stride, int rows_per_frame, int row_offset,
    const bf16_t* __restrict__ weight, const bf16_t* __restrict__ bias) {
  using namespace mx6;
  __shared__ float red[8];
  const int row = blockIdx.x;
  const int nchunks = d >> 3;
  float v[EW_MAXC][8];
#pragma unroll
  for (int i = 0; i < EW_MAXC; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
  layernorm_row(x, d, eps, shift, scale, frame_stride, rows_per_frame, row_offset, weight, bias, red, [&](int i, int, const float* o) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[i][j] = round_bf16(o[j]);   // the bf16 value layernorm_modulate_kernel stores: what the Linear's input is
  });
  uint8_t* cr = codes + (int64_t)row * ld_codes;
  uint8_t* sr = scales + (int64_t)row * ld_scales;
#pragma unroll
  for (int i = 0; i < EW_MAXC; ++i) {
    const int c = threadIdx.x + i * THREADS;
    uint32_t E;
    const uint64_t w = quantize_chunk(v[i], &E);
    store_chunk(cr, sr, c, c < nchunks, w, E);
  }
}

}  // namespace rtv

using namespace rtv;

static int mxfp6_check_out(const char* who, int d, const void* codes, int64_t ld_codes, int64_t ld_scales) {
  if ((ld_codes & 3) || ld_codes < RTV_MXFP6_CODE_BYTES(d) || ld_scales < RTV_MXFP6_SCALE_BYTES(d) || ((uintptr_t)codes & 3))
    return set_error(-1, (std::string(who) + ": ld_codes must be a multiple of 4 and >= 3 d / 4, ld_scales >= RTV_MXFP6_SCALE_BYTES(d), "
                                             "codes 4-byte aligned").c_str());
  return 0;
}

extern "C" int rtv_quantize_mxfp6(const void* x, int64_t ld, int M, int d, void* codes, int64_t ld_codes, void* scales,
                                  int64_t ld_scales, rtv_stream_t stream) {
  if (!x || !codes || !scales) return set_error(-1, "quantize_mxfp6: null pointer");
  if (M <= 0 || d <= 0) return set_error(-1, "quantize_mxfp6: empty tensor");
  if ((d & 31) || (ld & 7) || ld < d) return set_error(-1, "quantize_mxfp6: d must be a multiple of 32, ld a multiple of 8 and >= d");
  if ((uintptr_t)x & 15) return set_error(-1, "quantize_mxfp6: x must be 16-byte aligned");
  if (d > mx6::THREADS * 8 * 7) return set_error(-1, "quantize_mxfp6: d must be <= 14336");
  if (int st = mxfp6_check_out("quantize_mxfp6", d, codes, ld_codes, ld_scales)) return st;
  hipStream_t s = (hipStream_t)stream;
  const uint16_t* xp = (const uint16_t*)x;
  uint8_t *cp = (uint8_t*)codes, *sp = (uint8_t*)scales;
  ProfScope prof(PROF_MISC, s, 0.0);
  if (d <= 64 * 8 * 4)
    hipLaunchKernelGGL((quantize_mxfp6_kernel<4, true>), dim3((M + 3) / 4), dim3(mx6::THREADS), 0, s, xp, ld, M, d, cp, ld_codes, sp, ld_scales);
  else if (d <= mx6::THREADS * 8 * 3)
    hipLaunchKernelGGL((quantize_mxfp6_kernel<3, false>), dim3(M), dim3(mx6::THREADS), 0, s, xp, ld, M, d, cp, ld_codes, sp, ld_scales);
  else
    hipLaunchKernelGGL((quantize_mxfp6_kernel<7, false>), dim3(M), dim3(mx6::THREADS), 0, s, xp, ld, M, d, cp, ld_codes, sp, ld_scales);
  return check_launch("quantize_mxfp6");
}

extern "C" int rtv_layernorm_modulate_mxfp6(const void* x, void* codes, int64_t ld_codes, void* scales, int64_t ld_scales, int M, int d,
                                            float eps, const void* shift, const void* scale, int frame_stride, int rows_per_frame,
                                            int row_offset, const void* weight, const void* bias, rtv_stream_t stream) {
  if (M <= 0) return 0;
  if (!x || !codes || !scales) return set_error(-1, "layernorm_modulate_mxfp6: null pointer");
  if (d <= 0 || d % 32 || d > mx6::THREADS * 8 * EW_MAXC) return set_error(-1, "layernorm_modulate_mxfp6: d must be a multiple of 32 and <= 8192");
  if ((uintptr_t)x & 15) return set_error(-1, "layernorm_modulate_mxfp6: x must be 16-byte aligned");
  if (int st = mxfp6_check_out("layernorm_modulate_mxfp6", d, codes, ld_codes, ld_scales)) return st;
  if ((shift == nullptr) != (scale == nullptr)) return set_error(-1, "layernorm_modulate_mxfp6: shift and scale go together");
  if ((weight == nullptr) != (bias == nullptr)) return set_error(-1, "layernorm_modulate_mxfp6: weight and bias go together");
  if (weight && scale) return set_error(-1, "layernorm_modulate_mxfp6: affine and modulation are exclusive");
  if (scale && (rows_per_frame <= 0 || frame_stride % 8)) return set_error(-1, "layernorm_modulate_mxfp6: bad frame geometry");
  ProfScope prof(PROF_LN, (hipStream_t)stream, M * (double)d * 3);
  hipLaunchKernelGGL(layernorm_modulate_mxfp6_kernel, dim3(M), dim3(mx6::THREADS), 0, (hipStream_t)stream, (const bf16_t*)x, (uint8_t*)codes,
                     ld_codes, (uint8_t*)scales, ld_scales, d, eps, (const bf16_t*)shift, (const bf16_t*)scale, frame_stride, rows_per_frame,
                     row_offset, (const bf16_t*)weight, (const bf16_t*)bias);
  return check_launch("layernorm_modulate_mxfp6");
}
