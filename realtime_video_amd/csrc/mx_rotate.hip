// The rotated MXFP4 / MXFP6 quantisers (include/rtv_hip_mx_rotate.h): mx_quant.h's two bodies with ROT = true under both format
// traits - the 32-point Hadamard butterflies of each block in front of the unchanged conversion (mx_quant.h: rotate_chunk).
//   quantize_mx_rot_kernel            x bf16 -> rotate, scale by 2^-shift -> codes + scales; geometry of the unrotated kernels
//   layernorm_modulate_mx_rot_kernel  the LayerNorm-fused quantiser, rotating the bf16-rounded values it keeps, at the activation shift
// A unit of its own: mxfp4.hip and mxfp6.hip hold the unrotated kernels and nothing else.
#include "../../include/rtv_hip_mx_rotate.h"
#include "mxfp4_format.h"
#include "mxfp6_format.h"

namespace rtv {

template <class F, int MAXC, bool WAVE>
__global__ __launch_bounds__(mxq::THREADS) void quantize_mx_rot_kernel(const uint16_t* __restrict__ x, int64_t ld, int M, int d,
                                                                       uint8_t* __restrict__ codes, int64_t ld_codes,
                                                                       uint8_t* __restrict__ scales, int64_t ld_scales, float rot_scale) {
  mxq::quantize_rows<F, MAXC, WAVE, true>(x, ld, M, d, codes, ld_codes, scales, ld_scales, rot_scale);
}

template <class F>
__global__ __launch_bounds__(mxq::THREADS) void layernorm_modulate_mx_rot_kernel(
    const bf16_t* __restrict__ x, uint8_t* __restrict__ codes, int64_t ld_codes, uint8_t* __restrict__ scales, int64_t ld_scales, int d,
    float eps, const bf16_t* __restrict__ shift, const bf16_t* __restrict__ scale, int frame_stride, int rows_per_frame, int row_offset,
    const bf16_t* __restrict__ weight, const bf16_t* __restrict__ bias) {
  mxq::layernorm_modulate_mx<F, true>(x, codes, ld_codes, scales, ld_scales, d, eps, shift, scale, frame_stride, rows_per_frame, row_offset,
                                      weight, bias);
}

typedef void (*QuantizeRotKernel)(const uint16_t*, int64_t, int, int, uint8_t*, int64_t, uint8_t*, int64_t, float);

template <class F>
static int quantize_rot(const void* x, int64_t ld, int M, int d, void* codes, int64_t ld_codes, void* scales, int64_t ld_scales, int shift,
                        rtv_stream_t stream) {
  if (shift < 0 || shift > RTV_MX_ROT_MAX_SHIFT) return mxq::fail(F::QUANTIZE, "shift must be in 0 .. 5");
  return mxq::quantize<F, QuantizeRotKernel>(quantize_mx_rot_kernel<F, 4, true>, quantize_mx_rot_kernel<F, 3, false>,
                                             quantize_mx_rot_kernel<F, 7, false>, x, ld, M, d, codes, ld_codes, scales, ld_scales, stream,
                                             1.f / (float)(1 << shift));
}

}  // namespace rtv

using namespace rtv;

extern "C" int rtv_quantize_mxfp4_rot(const void* x, int64_t ld, int M, int d, void* codes, int64_t ld_codes, void* scales,
                                      int64_t ld_scales, int shift, rtv_stream_t stream) {
  return quantize_rot<Mxfp4>(x, ld, M, d, codes, ld_codes, scales, ld_scales, shift, stream);
}

extern "C" int rtv_quantize_mxfp6_rot(const void* x, int64_t ld, int M, int d, void* codes, int64_t ld_codes, void* scales,
                                      int64_t ld_scales, int shift, rtv_stream_t stream) {
  return quantize_rot<Mxfp6>(x, ld, M, d, codes, ld_codes, scales, ld_scales, shift, stream);
}

extern "C" int rtv_layernorm_modulate_mxfp4_rot(const void* x, void* codes, int64_t ld_codes, void* scales, int64_t ld_scales, int M, int d,
                                                float eps, const void* shift, const void* scale, int frame_stride, int rows_per_frame,
                                                int row_offset, const void* weight, const void* bias, rtv_stream_t stream) {
  return mxq::layernorm_modulate<Mxfp4>(layernorm_modulate_mx_rot_kernel<Mxfp4>, x, codes, ld_codes, scales, ld_scales, M, d, eps, shift,
                                        scale, frame_stride, rows_per_frame, row_offset, weight, bias, stream);
}

extern "C" int rtv_layernorm_modulate_mxfp6_rot(const void* x, void* codes, int64_t ld_codes, void* scales, int64_t ld_scales, int M, int d,
                                                float eps, const void* shift, const void* scale, int frame_stride, int rows_per_frame,
                                                int row_offset, const void* weight, const void* bias, rtv_stream_t stream) {
  return mxq::layernorm_modulate<Mxfp6>(layernorm_modulate_mx_rot_kernel<Mxfp6>, x, codes, ld_codes, scales, ld_scales, M, d, eps, shift,
                                        scale, frame_stride, rows_per_frame, row_offset, weight, bias, stream);
}
