// MXFP4 quantisers (include/rtv_hip_mxfp4.h; the OCP Microscaling conversion with the floor rule, tests/mxfp4_oracle.py):
//   per 32-element block  E = max(biased exponent of max|x| - 2, 0),  code = e2m1(x * 2^(127 - E)), nearest even, saturating at 6.
// (E is the header's clamp(floor(log2 amax) - 2, -127, 127) + 127: the fp32 exponent field of a bf16 value is floor(log2) + 127 for
// normal numbers, subnormal and zero maxima clamp to E = 0, and the largest finite exponent field, 254, gives E = 252.)
// A block needs nothing but itself, so there is no row reduction: a lane holds 8 consecutive elements (one 16-byte chunk), the 4 lanes
// of a quad hold a block, and the block maximum is two lane exchanges.  Two kernels, with the geometry of fp8_rows.hip:
//   quantize_mxfp4_kernel            x bf16 -> codes + scales; a wave per row up to 2048 columns, a workgroup per row above
//   layernorm_modulate_mxfp4_kernel  elementwise.hip's layernorm_modulate_kernel with this quantiser behind its bf16 rounding
// The GEMM that consumes the codes is gemm_mxfp4.hip.
#include <string>

#include "../../include/rtv_hip_mxfp4.h"
#include "ln_row.h"
#include "rtv_common.h"
#include "rtv_internal.h"

namespace rtv {

namespace mx4 {
constexpr int THREADS = EW_THREADS;

// e2m1 magnitude code of t >= 0, round to nearest even, saturating: the representable magnitudes are 0, 0.5, 1, 1.5, 2, 3, 4, 6, so
// the code is the number of rounding boundaries at or below t; a boundary (the midpoint of two neighbours) belongs to the neighbour
// with the even code, i.e. it is passed by `>` when the code below it is even and by `>=` when it is odd.
__device__ __forceinline__ uint32_t e2m1_mag(float t) {
  return (uint32_t)(t > 0.25f) + (uint32_t)(t >= 0.75f) + (uint32_t)(t > 1.25f) + (uint32_t)(t >= 1.75f) + (uint32_t)(t > 2.5f) +
         (uint32_t)(t >= 3.5f) + (uint32_t)(t > 5.0f);
}

// The 8 values of this lane (bf16 values in fp32) -> their 8 codes as one dword, element j in nibble j; *E = the scale byte of the
// block this lane's quad holds.  Every lane of a quad must call this together (lanes without data pass zeros).
__device__ __forceinline__ uint32_t quantize_chunk(const float* v, uint32_t* E) {
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(v[j]));
  m = fmaxf(m, __shfl_xor(m, 1, 64));
  m = fmaxf(m, __shfl_xor(m, 2, 64));
  const int ex = (int)((__float_as_uint(m) >> 23) & 0xffu);
  const int eb = max(ex - 2, 0);
  *E = (uint32_t)eb;
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float t = ldexpf(fabsf(v[j]), 127 - eb);   // exact: a power-of-two scaling of a bf16 value, below 8 by construction
    w |= (e2m1_mag(t) | ((__float_as_uint(v[j]) >> 28) & 8u)) << (4 * j);
  }
  return w;
}

// chunk c of a row (elements 8 c .. + 8) -> its dword of codes and, from the quad's first lane, the block's scale byte
__device__ __forceinline__ void store_chunk(uint8_t* codes_row, uint8_t* scales_row, int c, uint32_t w, uint32_t E) {
  *(uint32_t*)(codes_row + c * 4) = w;
  if ((c & 3) == 0) scales_row[RTV_MXFP4_SCALE_POS(c >> 2)] = (uint8_t)E;
}
}  // namespace mx4

// ------------------------------------------------------------------ row quantiser
// WAVE: a wave per row (4 rows per workgroup); else a workgroup per row.  The G lanes of a row take its 16-byte chunks G apart,
// MAXC of them each: rows of up to G * 8 * MAXC elements.  d % 32 == 0, so a quad's 4 chunks are inside the row or outside together.
template <int MAXC, bool WAVE>
__global__ __launch_bounds__(mx4::THREADS) void quantize_mxfp4_kernel(const uint16_t* __restrict__ x, int64_t ld, int M, int d,
                                                                     uint8_t* __restrict__ codes, int64_t ld_codes,
                                                                     uint8_t* __restrict__ scales, int64_t ld_scales) {
  using namespace mx4;
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
    const uint32_t w = quantize_chunk(v, &E);
    if (c < nchunks) store_chunk(cr, sr, c, w, E);
  }
}

// ------------------------------------------------------------------ LayerNorm (+ modulation) + quantiser, a workgroup per row
// layernorm_modulate_kernel's row (ln_row.h: same reductions, same rounding points) up to the value it would store; that value is
// rounded to bf16 as the store would round it, kept in registers, and quantised as quantize_mxfp4_kernel quantises the stored row.
__global__ __launch_bounds__(mx4::THREADS) void layernorm_modulate_mxfp4_kernel(
    const bf16_t* __restrict__ x, uint8_t* __restrict__ codes, int64_t ld_codes, uint8_t* __restrict__ scales, int64_t ld_scales, int d,
    float eps, const bf16_t* __restrict__ shift, const bf16_t* __restrict__ scale, int frame_stride, int rows_per_frame, int row_offset,
    const bf16_t* __restrict__ weight, const bf16_t* __restrict__ bias) {
  using namespace mx4;
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
    const uint32_t w = quantize_chunk(v[i], &E);
    if (c < nchunks) store_chunk(cr, sr, c, w, E);
  }
}

}  // namespace rtv

using namespace rtv;

static int mxfp4_check_out(const char* who, int d, const void* codes, int64_t ld_codes, int64_t ld_scales) {
  if ((ld_codes & 3) || ld_codes < d / 2 || ld_scales < RTV_MXFP4_SCALE_BYTES(d) || ((uintptr_t)codes & 3))
    return set_error(-1, (std::string(who) + ": ld_codes must be a multiple of 4 and >= d / 2, ld_scales >= RTV_MXFP4_SCALE_BYTES(d), "
                                             "codes 4-byte aligned").c_str());
  return 0;
}

extern "C" int rtv_quantize_mxfp4(const void* x, int64_t ld, int M, int d, void* codes, int64_t ld_codes, void* scales,
                                  int64_t ld_scales, rtv_stream_t stream) {
  if (!x || !codes || !scales) return set_error(-1, "quantize_mxfp4: null pointer");
  if (M <= 0 || d <= 0) return set_error(-1, "quantize_mxfp4: empty tensor");
  if ((d & 31) || (ld & 7) || ld < d) return set_error(-1, "quantize_mxfp4: d must be a multiple of 32, ld a multiple of 8 and >= d");
  if ((uintptr_t)x & 15) return set_error(-1, "quantize_mxfp4: x must be 16-byte aligned");
  if (d > mx4::THREADS * 8 * 7) return set_error(-1, "quantize_mxfp4: d must be <= 14336");
  if (int st = mxfp4_check_out("quantize_mxfp4", d, codes, ld_codes, ld_scales)) return st;
  hipStream_t s = (hipStream_t)stream;
  const uint16_t* xp = (const uint16_t*)x;
  uint8_t *cp = (uint8_t*)codes, *sp = (uint8_t*)scales;
  ProfScope prof(PROF_MISC, s, 0.0);
  if (d <= 64 * 8 * 4)
    hipLaunchKernelGGL((quantize_mxfp4_kernel<4, true>), dim3((M + 3) / 4), dim3(mx4::THREADS), 0, s, xp, ld, M, d, cp, ld_codes, sp, ld_scales);
  else if (d <= mx4::THREADS * 8 * 3)
    hipLaunchKernelGGL((quantize_mxfp4_kernel<3, false>), dim3(M), dim3(mx4::THREADS), 0, s, xp, ld, M, d, cp, ld_codes, sp, ld_scales);
  else
    hipLaunchKernelGGL((quantize_mxfp4_kernel<7, false>), dim3(M), dim3(mx4::THREADS), 0, s, xp, ld, M, d, cp, ld_codes, sp, ld_scales);
  return check_launch("quantize_mxfp4");
}

extern "C" int rtv_layernorm_modulate_mxfp4(const void* x, void* codes, int64_t ld_codes, void* scales, int64_t ld_scales, int M, int d,
                                            float eps, const void* shift, const void* scale, int frame_stride, int rows_per_frame,
                                            int row_offset, const void* weight, const void* bias, rtv_stream_t stream) {
  if (M <= 0) return 0;
  if (!x || !codes || !scales) return set_error(-1, "layernorm_modulate_mxfp4: null pointer");
  if (d <= 0 || d % 32 || d > mx4::THREADS * 8 * EW_MAXC) return set_error(-1, "layernorm_modulate_mxfp4: d must be a multiple of 32 and <= 8192");
  if ((uintptr_t)x & 15) return set_error(-1, "layernorm_modulate_mxfp4: x must be 16-byte aligned");
  if (int st = mxfp4_check_out("layernorm_modulate_mxfp4", d, codes, ld_codes, ld_scales)) return st;
  if ((shift == nullptr) != (scale == nullptr)) return set_error(-1, "layernorm_modulate_mxfp4: shift and scale go together");
  if ((weight == nullptr) != (bias == nullptr)) return set_error(-1, "layernorm_modulate_mxfp4: weight and bias go together");
  if (weight && scale) return set_error(-1, "layernorm_modulate_mxfp4: affine and modulation are exclusive");
  if (scale && (rows_per_frame <= 0 || frame_stride % 8)) return set_error(-1, "layernorm_modulate_mxfp4: bad frame geometry");
  ProfScope prof(PROF_LN, (hipStream_t)stream, M * (double)d * 3);
  hipLaunchKernelGGL(layernorm_modulate_mxfp4_kernel, dim3(M), dim3(mx4::THREADS), 0, (hipStream_t)stream, (const bf16_t*)x, (uint8_t*)codes,
                     ld_codes, (uint8_t*)scales, ld_scales, d, eps, (const bf16_t*)shift, (const bf16_t*)scale, frame_stride, rows_per_frame,
                     row_offset, (const bf16_t*)weight, (const bf16_t*)bias);
  return check_launch("layernorm_modulate_mxfp4");
}
