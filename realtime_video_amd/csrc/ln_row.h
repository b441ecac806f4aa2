// Row kernels of the DiT block, one 256-thread workgroup per token row: their common geometry and reduction, and the LayerNorm
// (+ AdaLN modulation, or affine) of a row up to the fp32 values in front of its final bf16 rounding.  layernorm_modulate_kernel
// (elementwise.hip) stores those values; layernorm_modulate_fp8_rows_kernel (fp8_rows.hip) quantises them: one text, same bits.
#pragma once
#include "rtv_common.h"

namespace rtv {

constexpr int EW_THREADS = 256;
constexpr int EW_MAXC = 4;  // rows of up to EW_THREADS * 8 * EW_MAXC = 8192 elements (16 chunks per lane of the row's wave)

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();  // protect `red` from the previous use
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// LayerNorm of row blockIdx.x of x [rows][d]: emit(i, c, o) receives, for this thread's i-th 16-byte chunk c (elements
// c * 8 .. + 8), the eight results in fp32; the caller rounds them to bf16.  `red`: 4 floats of LDS.
template <class Emit>
__device__ __forceinline__ void layernorm_row(const bf16_t* __restrict__ x, int d, float eps, const bf16_t* __restrict__ shift,
                                              const bf16_t* __restrict__ scale, int frame_stride, int rows_per_frame, int row_offset,
                                              const bf16_t* __restrict__ weight, const bf16_t* __restrict__ bias, float* red, Emit emit) {
  const int row = blockIdx.x;
  const int nchunks = d >> 3;
  const bf16_t* xr = x + (size_t)row * d;
  float v[EW_MAXC][8];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < EW_MAXC; ++i) {
    int c = threadIdx.x + i * EW_THREADS;
    if (c < nchunks) {
      u32x4 raw = *(const u32x4*)(xr + c * 8);
      unpack_bf16x8(raw, v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[i][j];
    }
  }
  const float mean = block_sum(s, red) / (float)d;
  float s2 = 0.f;
#pragma unroll
  for (int i = 0; i < EW_MAXC; ++i) {
    int c = threadIdx.x + i * EW_THREADS;
    if (c < nchunks) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float t = v[i][j] - mean;
        s2 += t * t;
      }
    }
  }
  const float var = block_sum(s2, red) / (float)d;
  const float rstd = rsqrtf(var + eps);
  const int f = rows_per_frame > 0 ? (row_offset + row) / rows_per_frame : 0;
  const bf16_t* sh = shift ? shift + (size_t)f * frame_stride : nullptr;
  const bf16_t* sc = scale ? scale + (size_t)f * frame_stride : nullptr;
#pragma unroll
  for (int i = 0; i < EW_MAXC; ++i) {
    int c = threadIdx.x + i * EW_THREADS;
    if (c < nchunks) {
      float o[8];
      if (weight) {  // affine LayerNorm: one rounding at the output (torch kernel computes in f32)
        float w8[8], b8[8];
        unpack_bf16x8(*(const u32x4*)(weight + c * 8), w8);
        unpack_bf16x8(*(const u32x4*)(bias + c * 8), b8);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (v[i][j] - mean) * rstd * w8[j] + b8[j];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (v[i][j] - mean) * rstd;
        if (sc) {  // bf16(bf16(bf16(ln) * bf16(1 + scale)) + shift)
          float sc8[8], sh8[8];
          unpack_bf16x8(*(const u32x4*)(sc + c * 8), sc8);
          unpack_bf16x8(*(const u32x4*)(sh + c * 8), sh8);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float n = round_bf16(o[j]);
            float a = round_bf16(1.0f + sc8[j]);
            float p = round_bf16(n * a);
            o[j] = p + sh8[j];
          }
        }
      }
      emit(i, c, o);
    }
  }
}

}  // namespace rtv
