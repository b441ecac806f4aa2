// The MXFP4 format trait of mx_quant.h (include/rtv_hip_mxfp4.h): the e2m1 value table, saturating at 6, and a nibble packer.  A
// header because two units instantiate the quantiser bodies under it: mxfp4.hip and mx_rotate.hip.
#pragma once
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

}  // namespace rtv
