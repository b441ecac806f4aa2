// MXFP6 quantisers (include/rtv_hip_mxfp6.h): mx_quant.h's bodies with the e2m3 value table, saturating at 7.5, and a 6-bit packer
// (mxfp6_format.h).  The rotated forms of both kernels are in mx_rotate.hip.
//   quantize_mxfp6_kernel           x bf16 -> codes + scales; a wave per row up to 2048 columns, a workgroup per row above
//   layernorm_modulate_mxfp6_kernel  elementwise.hip's layernorm_modulate_kernel with this quantiser behind its bf16 rounding
// The GEMM that consumes the codes is gemm_mxfp6.hip.
#include "mxfp6_format.h"

namespace rtv {

template <int MAXC, bool WAVE>
__global__ __launch_bounds__(mxq::THREADS) void quantize_mxfp6_kernel(const uint16_t* __restrict__ x, int64_t ld, int M, int d,
                                                                      uint8_t* __restrict__ codes, int64_t ld_codes,
                                                                      uint8_t* __restrict__ scales, int64_t ld_scales) {
  mxq::quantize_rows<Mxfp6, MAXC, WAVE>(x, ld, M, d, codes, ld_codes, scales, ld_scales);
}

__global__ __launch_bounds__(mxq::THREADS) void layernorm_modulate_mxfp6_kernel(
    const bf16_t* __restrict__ x, uint8_t* __restrict__ codes, int64_t ld_codes, uint8_t* __restrict__ scales, int64_t ld_scales, int d,
    float eps, const bf16_t* __restrict__ shift, const bf16_t* __restrict__ scale, int frame_stride, int rows_per_frame, int row_offset,
    const bf16_t* __restrict__ weight, const bf16_t* __restrict__ bias) {
  mxq::layernorm_modulate_mx<Mxfp6>(x, codes, ld_codes, scales, ld_scales, d, eps, shift, scale, frame_stride, rows_per_frame, row_offset,
                                    weight, bias);
}

}  // namespace rtv

using namespace rtv;

extern "C" int rtv_quantize_mxfp6(const void* x, int64_t ld, int M, int d, void* codes, int64_t ld_codes, void* scales,
                                  int64_t ld_scales, rtv_stream_t stream) {
  return mxq::quantize<Mxfp6>(quantize_mxfp6_kernel<4, true>, quantize_mxfp6_kernel<3, false>, quantize_mxfp6_kernel<7, false>, x, ld, M, d,
                              codes, ld_codes, scales, ld_scales, stream);
}

extern "C" int rtv_layernorm_modulate_mxfp6(const void* x, void* codes, int64_t ld_codes, void* scales, int64_t ld_scales, int M, int d,
                                            float eps, const void* shift, const void* scale, int frame_stride, int rows_per_frame,
                                            int row_offset, const void* weight, const void* bias, rtv_stream_t stream) {
  return mxq::layernorm_modulate<Mxfp6>(layernorm_modulate_mxfp6_kernel, x, codes, ld_codes, scales, ld_scales, M, d, eps, shift, scale,
                                        frame_stride, rows_per_frame, row_offset, weight, bias, stream);
}
