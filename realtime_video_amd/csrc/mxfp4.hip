// MXFP4 quantisers (include/rtv_hip_mxfp4.h): mx_quant.h's bodies with the e2m1 value table, saturating at 6, and a nibble packer.
//   quantize_mxfp4_kernel            x bf16 -> codes + scales; a wave per row up to 2048 columns, a workgroup per row above
//   layernorm_modulate_mxfp4_kernel  elementwise.hip's layernorm_modulate_kernel with this quantiser behind its bf16 rounding
// The GEMM that consumes the codes is gemm_mxfp4.hip.
#include "../../include/rtv_hip_mxfp4.h"
#include "mx_quant.h"

namespace rtv {

struct Mxfp4 {
  static constexpr int BITS = 4;
  typedef uint32_t word_t;   // a lane's 8 codes: one dword, element j in nibble j
  static constexpr const char *QUANTIZE = "quantize_mxfp4", *LAYERNORM = "layernorm_modulate_mxfp4", *MIN_CODES = "d / 2",
                              *SCALE_BYTES_NAME = "RTV_MXFP4_SCALE_BYTES(d)";
  static constexpr int64_t code_bytes(int d) { return d / 2; }
  static constexpr int64_t scale_bytes(int d) { return RTV_MXFP4_SCALE_BYTES(d); }

  // e2m1 magnitude code of t >= 0, round to nearest even, saturating: the representable magnitudes are 0, 0.5, 1, 1.5, 2, 3, 4, 6, so
  // the code is the number of rounding boundaries at or below t; a boundary (the midpoint of two neighbours) belongs to the neighbour
  // with the even code, i.e. it is passed by `>` when the code below it is even and by `>=` when it is odd.
  static __device__ __forceinline__ uint32_t mag(float t) {
    return (uint32_t)(t > 0.25f) + (uint32_t)(t >= 0.75f) + (uint32_t)(t > 1.25f) + (uint32_t)(t >= 1.75f) + (uint32_t)(t > 2.5f) +
           (uint32_t)(t >= 3.5f) + (uint32_t)(t > 5.0f);
  }

  // chunk c of a row (elements 8 c .. + 8) -> its dword of codes and, from the quad's first lane, the block's scale byte
  static __device__ __forceinline__ void store_chunk(uint8_t* codes_row, uint8_t* scales_row, int c, bool live, uint32_t w, uint32_t E) {
    if (!live) return;
    *(uint32_t*)(codes_row + c * 4) = w;
    if ((c & 3) == 0) scales_row[RTV_MXFP4_SCALE_POS(c >> 2)] = (uint8_t)E;
  }
};

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
