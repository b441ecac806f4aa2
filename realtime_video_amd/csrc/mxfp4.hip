// MXFP4 quantisers (include/rtv_hip_mxfp4.h): mx_quant.h's bodies with the e2m1 value table, saturating at 6, and a nibble packer
// (mxfp4_format.h).  The rotated forms of both kernels are in mx_rotate.hip.
//   quantize_mxfp4_kernel           x bf16 -> codes + scales; a wave per row up to 2048 columns, a workgroup per row above
//   layernorm_modulate_mxfp4_kernel  elementwise.hip's layernorm_modulate_kernel with this quantiser behind its bf16 rounding
// The GEMM that consumes the codes is gemm_mxfp4.hip.
#include "mxfp4_format.h"

namespace rtv {

template <int MAXC, bool WAVE>
__global__ __launch_bounds__(mxq::THREADS) void quantize_mxfp4_kernel(const uint16_t* __restrict__ x, int64_t ld, int M, int d,
                                                                      uint8_t* __restrict__ codes, int64_t ld_codes,
                                                                      uint8_t* __restrict__ scales, int64_t ld_scales) {
  mxq::quantize_rows<Mxfp4, MAXC, WAVE>(x, ld, M, d, codes, ld_codes, scales, ld_scales);
}

__global__ __launch_bounds__(mxq::THREADS) void layernorm_modulate_mxfp4_kernel(
    const bf16_t* __restrict__ x, uint8_t* __restrict__ codes, int64_t ld_codes, uint8_t* __restrict__ scales, int64_t ld_scales, int d,
    float eps, const bf16_t* __restrict__ shift, const bf16_t* __restrict__ scale, int frame_stride, int rows_per_frame, int row_offset,
    const bf16_t* __restrict__ weight, const bf16_t* __restrict__ bias) {
  mxq::layernorm_modulate_mx<Mxfp4>(x, codes, ld_codes, scales, ld_scales, d, eps, shift, scale, frame_stride, rows_per_frame, row_offset,
                                    weight, bias);
}

}  // namespace rtv

using namespace rtv;

extern "C" int rtv_quantize_mxfp4(const void* x, int64_t ld, int M, int d, void* codes, int64_t ld_codes, void* scales,
                                  int64_t ld_scales, rtv_stream_t stream) {
  return mxq::quantize<Mxfp4>(quantize_mxfp4_kernel<4, true>, quantize_mxfp4_kernel<3, false>, quantize_mxfp4_kernel<7, false>, x, ld, M, d,
                              codes, ld_codes, scales, ld_scales, stream);
}

extern "C" int rtv_layernorm_modulate_mxfp4(const void* x, void* codes, int64_t ld_codes, void* scales, int64_t ld_scales, int M, int d,
                                            float eps, const void* shift, const void* scale, int frame_stride, int rows_per_frame,
                                            int row_offset, const void* weight, const void* bias, rtv_stream_t stream) {
  return mxq::layernorm_modulate<Mxfp4>(layernorm_modulate_mxfp4_kernel, x, codes, ld_codes, scales, ld_scales, M, d, eps, shift, scale,
                                        frame_stride, rows_per_frame, row_offset, weight, bias, stream);
}
