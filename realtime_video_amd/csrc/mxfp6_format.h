// The MXFP6 format trait of mx_quant.h (include/rtv_hip_mxfp6.h): the e2m3 value table, saturating at 7.5, and a 6-bit packer.
// A lane's 8 codes are 48 bits, so the two lanes of a pair own three dwords of the block's six: the even lane stores the first two
// (its 48 bits and the partner's low 16, one more lane exchange), the odd lane the third - whole dwords, assembled in registers.
// A header because two units instantiate the quantiser bodies under it: mxfp6.hip and mx_rotate.hip.
#pragma once
#include "../../include/rtv_hip_mxfp6.h"
#include "mx_quant.h"

namespace rtv {

struct Mxfp6 {
  static constexpr int BITS = 6;
  typedef uint64_t word_t;   // a lane's 8 codes: 48 bits, element j at bits [6 j, 6 j + 6)
  static constexpr const char *QUANTIZE = "quantize_mxfp6", *LAYERNORM = "layernorm_modulate_mxfp6", *MIN_CODES = "3 d / 4",
                              *SCALE_BYTES_NAME = "RTV_MXFP6_SCALE_BYTES(d)";
  static constexpr int64_t code_bytes(int d) { return RTV_MXFP6_CODE_BYTES(d); }
  static constexpr int64_t scale_bytes(int d) { return RTV_MXFP6_SCALE_BYTES(d); }

  // e2m3 magnitude code (5 bits) of 0 <= t < 8, round to nearest even, saturating.  The 32 magnitudes in increasing order are the
  // multiples of 1/8 below 2 (codes 0-16: the subnormals and the first binade share a spacing), of 1/4 in [2, 4) (16-24) and of 1/2
  // in [4, 8) (24-31), so the code is the nearest integer of t over the spacing plus the offset of the range; rintf rounds ties to
  // the even integer, which is the even code in every range (the offsets are even), i.e. the even mantissa.  t * 8 is exact.
  static __device__ __forceinline__ uint32_t mag(float t) {
    const float r = t < 2.f ? rintf(t * 8.f) : t < 4.f ? rintf(t * 4.f) + 8.f : fminf(rintf(t * 2.f) + 16.f, 31.f);
    return (uint32_t)r;
  }

  // chunk c of a row (elements 8 c .. + 8) with its 48 bits w: chunks 2 p and 2 p + 1 (a lane pair) own the dwords 3 p .. 3 p + 2 of
  // the row's codes.  Every lane of a pair must call this together (the exchange); `live` = the chunk is inside the row.
  static __device__ __forceinline__ void store_chunk(uint8_t* codes_row, uint8_t* scales_row, int c, bool live, uint64_t w, uint32_t E) {
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
};

}  // namespace rtv
