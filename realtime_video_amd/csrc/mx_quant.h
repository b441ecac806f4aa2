// The block-scaled (OCP Microscaling) quantisers, once: mxfp4.hip and mxfp6.hip are this text under a format trait, as fp8_rows.hip
// and elementwise.hip are ln_row.h's.  The conversion is the floor rule of the public headers and of tests/mx_oracle.py:
//   per 32-element block  E = max(biased exponent of max|x| - 2, 0),  code = F::mag(x * 2^(127 - E)), nearest even, saturating.
// (E is the headers' clamp(floor(log2 amax) - 2, -127, 127) + 127: the fp32 exponent field of a bf16 value is floor(log2) + 127 for
// normal numbers, subnormal and zero maxima clamp to E = 0, and the largest finite exponent field, 254, gives E = 252.)
// A block needs nothing but itself, so there is no row reduction: a lane holds 8 consecutive elements (one 16-byte chunk), the 4 lanes
// of a quad hold a block, and the block maximum is two lane exchanges.  Two bodies, with the geometry of fp8_rows.hip:
//   quantize_rows          x bf16 -> codes + scales; a wave per row up to 2048 columns, a workgroup per row above
//   layernorm_modulate_mx  elementwise.hip's layernorm_modulate_kernel with this quantiser behind its bf16 rounding
// and the host functions behind the units' extern "C" entries, every check included.
//
// ROT (include/rtv_hip_mx_rotate.h; instantiated in mx_rotate.hip): both bodies with the 32-point Sylvester Hadamard transform of each
// block in front of quantize_chunk - rotate_chunk below.  A template parameter: the ROT = false bodies are the text they were.
//
// A format trait F supplies
//   BITS                          width of a code, sign on top; word_t = an unsigned type that holds a lane's 8 codes
//   mag(t)                        __device__: the magnitude code of 0 <= t < 8, round to nearest even, saturating
//   store_chunk(codes_row, scales_row, c, live, w, E)
//                                 __device__: chunk c of a row (elements 8 c .. + 8) with its codes w, element j at bits [BITS j,
//                                 BITS j + BITS), and from the quad's first lane the block's scale byte E.  Every lane calls it
//                                 (a packer may exchange between lanes); `live` = the chunk is inside the row.
//   code_bytes(d), scale_bytes(d) the public header's macros
//   QUANTIZE, LAYERNORM, MIN_CODES, SCALE_BYTES_NAME
//                                 the names the error strings use
#pragma once
#include <string>

#include "../../include/rtv_hip_mx_rotate.h"
#include "ln_row.h"
#include "rtv_common.h"
#include "rtv_internal.h"

namespace rtv {
namespace mxq {
constexpr int THREADS = EW_THREADS;

// The 8 values of this lane (bf16 values in fp32) -> their 8 codes; *E = the scale byte of the block this lane's quad holds.  Every
// lane of a quad must call this together (lanes without data pass zeros).
template <class F>
__device__ __forceinline__ typename F::word_t quantize_chunk(const float* v, uint32_t* E) {
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(v[j]));
  m = fmaxf(m, __shfl_xor(m, 1, 64));
  m = fmaxf(m, __shfl_xor(m, 2, 64));
  const int ex = (int)((__float_as_uint(m) >> 23) & 0xffu);
  const int eb = max(ex - 2, 0);
  *E = (uint32_t)eb;
  typename F::word_t w = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float t = ldexpf(fabsf(v[j]), 127 - eb);   // exact: a power-of-two scaling of a bf16 value (ROT: of an fp32 value), below 8 by construction
    w |= (typename F::word_t)(F::mag(t) | ((__float_as_uint(v[j]) >> (32 - F::BITS)) & (1u << (F::BITS - 1)))) << (F::BITS * j);
  }
  return w;
}

// ------------------------------------------------------------------ block rotation
// The lane xor 1 / xor 2 partner's value as a DPP quad_perm move: one VALU move inside the quad (a row of 4 lanes), no LDS crossbar
// (__shfl_xor is ds_bpermute_b32).  Every lane of the quad must be active.
template <int XOR>
__device__ __forceinline__ float quad_partner(float x) {
  static_assert(XOR == 1 || XOR == 2, "inside a quad");
  constexpr int QUAD_PERM = XOR == 1 ? 0xB1 : 0x4E;   // quad_perm:[1,0,3,2] / [2,3,0,1]
  return __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), QUAD_PERM, 0xF, 0xF, false));
}

// v (this lane's 8 of its quad's 32 values, element k = 8 * (lane & 3) + j of the block) -> (v H) * scale with H the Sylvester
// Hadamard matrix of order 32, by the butterflies of rtv_hip_mx_rotate.h: stage b = 0..4 in this order, (u, v) -> (u + v, u - v) on
// the pairs (k, k | 1 << b), fp32 adds and subtracts (nothing to fuse: there is no multiplication), then the exact power of two
// `scale`.  Stages 0-2 are inside the lane; stages 3 and 4 pair it with lane ^ 1 and lane ^ 2: the lane with the bit clear keeps
// own + partner, the lane with the bit set partner - own = partner + (-own), the same fp32 sum with the sign bit of `own` flipped.
__device__ __forceinline__ void rotate_chunk(float* v, float scale) {
#pragma unroll
  for (int b = 1; b < 8; b <<= 1)
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (!(j & b)) {
        const float u = v[j], w = v[j | b];
        v[j] = u + w;
        v[j | b] = u - w;
      }
  const uint32_t neg1 = (threadIdx.x & 1u) << 31, neg2 = (threadIdx.x & 2u) << 30;   // (chunk c = lane + i * G, G % 4 == 0: c & 3 = lane & 3)
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = quad_partner<1>(v[j]) + __uint_as_float(__float_as_uint(v[j]) ^ neg1);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (quad_partner<2>(v[j]) + __uint_as_float(__float_as_uint(v[j]) ^ neg2)) * scale;
}

// ------------------------------------------------------------------ row quantiser
// WAVE: a wave per row (4 rows per workgroup); else a workgroup per row.  The G lanes of a row take its 16-byte chunks G apart,
// MAXC of them each: rows of up to G * 8 * MAXC elements.  d % 32 == 0, so a quad's 4 chunks are inside the row or outside together.
// ROT: each block is rotated and scaled by rot_scale = 2^-shift in front of the conversion (rotate_chunk).
template <class F, int MAXC, bool WAVE, bool ROT = false>
__device__ __forceinline__ void quantize_rows(const uint16_t* __restrict__ x, int64_t ld, int M, int d, uint8_t* __restrict__ codes,
                                              int64_t ld_codes, uint8_t* __restrict__ scales, int64_t ld_scales, float rot_scale = 1.f) {
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
    if constexpr (ROT) rotate_chunk(v, rot_scale);
    uint32_t E;
    const typename F::word_t w = quantize_chunk<F>(v, &E);
    F::store_chunk(cr, sr, c, c < nchunks, w, E);
  }
}

// ------------------------------------------------------------------ LayerNorm (+ modulation) + quantiser, a workgroup per row
// layernorm_modulate_kernel's row (ln_row.h: same reductions, same rounding points) up to the value it would store; that value is
// rounded to bf16 as the store would round it, kept in registers, and quantised as quantize_rows quantises the stored row.
// ROT: the kept values are rotated in place, block by block, at the activation shift.
template <class F, bool ROT = false>
__device__ __forceinline__ void layernorm_modulate_mx(const bf16_t* __restrict__ x, uint8_t* __restrict__ codes, int64_t ld_codes,
                                                      uint8_t* __restrict__ scales, int64_t ld_scales, int d, float eps,
                                                      const bf16_t* __restrict__ shift, const bf16_t* __restrict__ scale, int frame_stride,
                                                      int rows_per_frame, int row_offset, const bf16_t* __restrict__ weight,
                                                      const bf16_t* __restrict__ bias) {
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
    if constexpr (ROT) rotate_chunk(v[i], 1.f / (1 << RTV_MX_ROT_ACT_SHIFT));
    uint32_t E;
    const typename F::word_t w = quantize_chunk<F>(v[i], &E);
    F::store_chunk(cr, sr, c, c < nchunks, w, E);
  }
}

// ------------------------------------------------------------------ host
typedef void (*QuantizeKernel)(const uint16_t*, int64_t, int, int, uint8_t*, int64_t, uint8_t*, int64_t);
typedef void (*LayerNormKernel)(const bf16_t*, uint8_t*, int64_t, uint8_t*, int64_t, int, float, const bf16_t*, const bf16_t*, int, int, int,
                                const bf16_t*, const bf16_t*);

inline int fail(const char* who, const std::string& what) { return set_error(-1, (std::string(who) + ": " + what).c_str()); }

template <class F>
int check_out(const char* who, int d, const void* codes, int64_t ld_codes, int64_t ld_scales) {
  if ((ld_codes & 3) || ld_codes < F::code_bytes(d) || ld_scales < F::scale_bytes(d) || ((uintptr_t)codes & 3))
    return fail(who, std::string("ld_codes must be a multiple of 4 and >= ") + F::MIN_CODES + ", ld_scales >= " + F::SCALE_BYTES_NAME +
                         ", codes 4-byte aligned");
  return 0;
}

// wave4 / block3 / block7: the unit's quantize kernel as <4, true>, <3, false> and <7, false>; `extra`: what a kernel takes behind
// ld_scales (the rotated kernels: rot_scale)
template <class F, class Kernel = QuantizeKernel, class... Extra>
int quantize(Kernel wave4, Kernel block3, Kernel block7, const void* x, int64_t ld, int M, int d, void* codes, int64_t ld_codes,
             void* scales, int64_t ld_scales, rtv_stream_t stream, Extra... extra) {
  const char* who = F::QUANTIZE;
  if (!x || !codes || !scales) return fail(who, "null pointer");
  if (M <= 0 || d <= 0) return fail(who, "empty tensor");
  if ((d & 31) || (ld & 7) || ld < d) return fail(who, "d must be a multiple of 32, ld a multiple of 8 and >= d");
  if ((uintptr_t)x & 15) return fail(who, "x must be 16-byte aligned");
  if (d > THREADS * 8 * 7) return fail(who, "d must be <= 14336");
  if (int st = check_out<F>(who, d, codes, ld_codes, ld_scales)) return st;
  hipStream_t s = (hipStream_t)stream;
  const bool wave = d <= 64 * 8 * 4;
  const Kernel kernel = wave ? wave4 : d <= THREADS * 8 * 3 ? block3 : block7;
  ProfScope prof(PROF_MISC, s, 0.0);
  hipLaunchKernelGGL(kernel, dim3(wave ? (M + 3) / 4 : M), dim3(THREADS), 0, s, (const uint16_t*)x, ld, M, d, (uint8_t*)codes, ld_codes,
                     (uint8_t*)scales, ld_scales, extra...);
  return check_launch(who);
}

template <class F>
int layernorm_modulate(LayerNormKernel kernel, const void* x, void* codes, int64_t ld_codes, void* scales, int64_t ld_scales, int M, int d,
                       float eps, const void* shift, const void* scale, int frame_stride, int rows_per_frame, int row_offset,
                       const void* weight, const void* bias, rtv_stream_t stream) {
  const char* who = F::LAYERNORM;
  if (M <= 0) return 0;
  if (!x || !codes || !scales) return fail(who, "null pointer");
  if (d <= 0 || d % 32 || d > THREADS * 8 * EW_MAXC) return fail(who, "d must be a multiple of 32 and <= 8192");
  if ((uintptr_t)x & 15) return fail(who, "x must be 16-byte aligned");
  if (int st = check_out<F>(who, d, codes, ld_codes, ld_scales)) return st;
  if ((shift == nullptr) != (scale == nullptr)) return fail(who, "shift and scale go together");
  if ((weight == nullptr) != (bias == nullptr)) return fail(who, "weight and bias go together");
  if (weight && scale) return fail(who, "affine and modulation are exclusive");
  if (scale && (rows_per_frame <= 0 || frame_stride % 8)) return fail(who, "bad frame geometry");
  ProfScope prof(PROF_LN, (hipStream_t)stream, M * (double)d * 3);
  hipLaunchKernelGGL(kernel, dim3(M), dim3(THREADS), 0, (hipStream_t)stream, (const bf16_t*)x, (uint8_t*)codes, ld_codes, (uint8_t*)scales,
                     ld_scales, d, eps, (const bf16_t*)shift, (const bf16_t*)scale, frame_stride, rows_per_frame, row_offset,
                     (const bf16_t*)weight, (const bf16_t*)bias);
  return check_launch(who);
}

}  // namespace mxq
}  // namespace rtv
