// Frame delivery side: decoder pixels -> complete baseline JPEG files on the device (include/rtv_hip_jpeg.h states the stream
// format).  Three launches per call:
//
//   transform  one workgroup = 4 horizontally adjacent MCUs (64 x 16 pixels) of one frame.  A thread loads 4 pixels of one row
//              (fp32 planes -> the byte rtv_pixels_to_rgb8 makes, or rgb8 as it is), writes their level-shifted Y into the four
//              luma blocks and, after one cross-lane add with the row below, the two 2x2 chroma means into the chroma blocks, all
//              in LDS (rows of 9 floats, blocks of 72: both DCT passes read conflict-free).  192 threads then run the 8-point DCT
//              down one column each, in place, and along one row each; the row's 8 coefficients are scaled by the reciprocal
//              quantiser step, rounded half away from zero and put at their zigzag position of an int16 staging tile, which
//              leaves as contiguous words: arena coefficients [T][mcu_rows][mcus][6][64].  Luma blocks wholly outside the
//              picture (H or W = 8 mod 16) become dummy blocks: the previous block's DC, no AC.
//   entropy    one workgroup = one (frame, MCU row) = one restart interval.  A thread owns a run of consecutive blocks: it
//              measures their Huffman-coded length, the lengths are scanned across the workgroup, the segment's words are zeroed,
//              and the thread codes its blocks again, ORing 32-bit words into the segment at its bit offset (atomics: the first
//              and last word of a run are shared with the neighbours).  The last byte is padded with 1 bits; the 0xFF bytes are
//              counted, so that the segment's stuffed length is known: seginfo [T][mcu_rows] = (bytes, bytes after stuffing).
//   assemble   one workgroup = one segment again: sums the stuffed lengths in front of it, and writes header (first row of a
//              frame), RSTn (other rows), the segment with a 0x00 behind every 0xFF, EOI (last row) and the frame offsets.  Every
//              byte store is guarded by out_cap; the offsets are the true ones whether the files fit or not.
//
// The segment scratch is sized by the bound, not by the data: a block takes at most 20 bits of DC (9-bit code + 11) and 63 x 26
// bits of AC (16-bit code + 10) = 1658 bits, 208 bytes.
#include "rtv_common.h"
#include "rtv_internal.h"
#include "../../include/rtv_hip_jpeg.h"

namespace rtv {
namespace {

constexpr int JPEG_HEADER_BYTES = 629;
constexpr int JPEG_BLOCK_BOUND_BYTES = 208;      // ceil(1658 / 8) rounded up to whole words
constexpr int JPEG_MAX_SIDE = 65528;             // the largest multiple of 8 SOF0's 16-bit fields hold

// ---------------------------------------------------------------------------------------------------------- tables (T.81 Annex K)
const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};   // zigzag index -> natural
const uint8_t kQuantBase[2][64] = {   // K.1 luminance, K.2 chrominance, natural order
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// K.3 - K.6 as (BITS[16], HUFFVAL): DC luminance, AC luminance, DC chrominance, AC chrominance
const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// what the kernels take by value with the launch: nothing of a call lives in device memory but the arena
struct QuantArg {
  float rq[2][64];        // 1 / step, natural order: luma, chroma
  uint8_t zz[64];         // natural index -> zigzag index
};
struct HuffArg {          // (code << 8) | length, indexed by the symbol; length 0 = the table has no such symbol
  uint32_t dc[2][12];
  uint32_t ac[2][256];
};
struct HeaderArg {
  int len;
  uint8_t bytes[640];
};

void quant_steps(int quality, int comp, uint8_t* steps /* natural order */) {   // libjpeg jpeg_quality_scaling + jpeg_add_quant_table
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; ++i) {
    int v = (kQuantBase[comp][i] * scale + 50) / 100;
    steps[i] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
  }
}

void huff_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* table) {   // T.81 Annex C: codes in order of length, then value
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i) table[vals[k++]] = (code++ << 8) | (uint32_t)len;
    code <<= 1;
  }
}

const HuffArg& huff_tables() {
  static const HuffArg h = [] {
    HuffArg t = {};
    for (int c = 0; c < 2; ++c) {
      huff_codes(kDcBits[c], kDcVals, t.dc[c]);
      huff_codes(kAcBits[c], kAcVals[c], t.ac[c]);
    }
    return t;
  }();
  return h;
}

size_t write_header(int quality, int H, int W, uint8_t* b) {
  size_t n = 0;
  auto put = [&](std::initializer_list<int> v) { for (int x : v) b[n++] = (uint8_t)x; };
  put({0xFF, 0xD8});                                                                             // SOI
  put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});                    // APP0: JFIF 1.01, aspect 1:1, no thumbnail
  for (int c = 0; c < 2; ++c) {                                                                  // DQT: 8-bit table c, zigzag order
    uint8_t steps[64];
    quant_steps(quality, c, steps);
    put({0xFF, 0xDB, 0, 67, c});
    for (int i = 0; i < 64; ++i) b[n++] = steps[kZigzag[i]];
  }
  put({0xFF, 0xC0, 0, 17, 8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});   // SOF0
  for (int c = 0; c < 2; ++c) {                                                                  // DHT: class << 4 | id
    put({0xFF, 0xC4, 0, 2 + 1 + 16 + 12, c});
    for (int i = 0; i < 16; ++i) b[n++] = kDcBits[c][i];
    for (int i = 0; i < 12; ++i) b[n++] = kDcVals[i];
    put({0xFF, 0xC4, 0, 2 + 1 + 16 + 162, 0x10 | c});
    for (int i = 0; i < 16; ++i) b[n++] = kAcBits[c][i];
    for (int i = 0; i < 162; ++i) b[n++] = kAcVals[c][i];
  }
  const int ri = (W + 15) / 16;
  put({0xFF, 0xDD, 0, 4, ri >> 8, ri & 255});                                                    // DRI: one MCU row
  put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});                              // SOS
  return n;
}

// ---------------------------------------------------------------------------------------------------------------- device helpers
// exclusive scan of one int per thread over a 256-thread workgroup; lds: 4 ints, reusable straight after
__device__ __forceinline__ int block_scan_exclusive(int v, int* lds, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int s = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(s, d);
    if (lane >= d) s += o;
  }
  __syncthreads();                  // the previous call's readers are done with lds
  if (lane == 63) lds[wave] = s;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int x = lds[w];
    base += w < wave ? x : 0;
    tot += x;
  }
  *total = tot;
  return base + s - v;
}

// 0.5 * cos((2n + 1) k pi / 16), scaled by 1 / sqrt(2) for k = 0: F = C f C^T is the T.81 A.3.3 forward DCT
__device__ __forceinline__ constexpr float dct_coef(int k, int n) {
  constexpr float h[9] = {0.5f, 0.49039264020161522f, 0.46193976625564337f, 0.41573480615127262f, 0.35355339059327379f,
                          0.27778511650980114f, 0.19134171618254492f, 0.097545161008064166f, 0.0f};   // 0.5 cos(j pi / 16)
  if (k == 0) return 0.35355339059327379f;
  int m = ((2 * n + 1) * k) & 31;
  if (m > 16) m = 32 - m;
  return m > 8 ? -h[16 - m] : h[m];
}

__device__ __forceinline__ void dct8(const float* in, float* out) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float s = 0.0f;
#pragma unroll
    for (int n = 0; n < 8; ++n) s = fmaf(dct_coef(k, n), in[n], s);
    out[k] = s;
  }
}

__device__ __forceinline__ int pixel_byte(float x) {   // rtv_pixels_to_rgb8's arithmetic (elementwise.hip), NaN -> 0
  float y = __fmul_rn(__fadd_rn(x, 1.0f), 0.5f);
  y = fminf(fmaxf(y, 0.0f), 1.0f);
  return (int)(uint8_t)(int)__fmul_rn(y, 255.0f);
}

// ---------------------------------------------------------------------------------------------------------------------- transform
constexpr int TR_MCUS = 4;                   // MCUs of one workgroup
constexpr int TR_BLOCKS = TR_MCUS * 6;
constexpr int TR_ROW = 9, TR_BLK = 72;       // floats per block row / per block in LDS

// luma block k (Y00 Y01 Y10 Y11) of MCU (mx, my) lies wholly outside the picture: H or W is 8 mod 16 and this is the far half of an
// edge MCU.  A decoder drops its pixels, so it is coded the cheapest way, as libjpeg codes its dummy blocks: no AC, and the DC of
// the block coded before it (difference 0).  Chroma blocks are never outside.
__device__ __forceinline__ bool outside(int mx, int my, int k, int H, int W) {
  return k < 4 && (mx * 2 + (k & 1) >= (W >> 3) || my * 2 + (k >> 1) >= (H >> 3));
}

template <bool RGB8>
__global__ void __launch_bounds__(256) jpeg_transform_kernel(const void* __restrict__ px, int16_t* __restrict__ coef, int H, int W, int mcus,
                                                             const QuantArg q) {
  __shared__ float S[TR_BLOCKS * TR_BLK];
  __shared__ __attribute__((aligned(16))) int16_t staged[TR_BLOCKS * 64];
  __shared__ float rq[128];
  __shared__ uint8_t zz[64];
  const int tid = threadIdx.x;
  if (tid < 128) rq[tid] = q.rq[tid >> 6][tid & 63];
  if (tid < 64) zz[tid] = q.zz[tid];
  const int mcu0 = blockIdx.x * TR_MCUS, my = blockIdx.y, t = blockIdx.z;
  const int row = tid >> 4, xq = tid & 15;
  const int y = min(my * 16 + row, H - 1);                 // the bottom half of an edge MCU replicates the last row
  const int x = mcu0 * 16 + xq * 4;
  const bool inside = x < W;                               // W % 4 == 0: a thread's 4 pixels are all inside or all outside
  const int xc = inside ? x : W - 1;                       // ... and outside they replicate the last column
  int r[4], g[4], b[4];
  if (RGB8) {
    const uint8_t* p = (const uint8_t*)px + (((size_t)t * H + y) * W + xc) * 3;
    if (inside) {
      uint32_t w[3];
      if (((uintptr_t)p & 3) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = ((const uint32_t*)p)[k];
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        r[k] = (w[(3 * k) >> 2] >> (8 * ((3 * k) & 3))) & 255u;
        g[k] = (w[(3 * k + 1) >> 2] >> (8 * ((3 * k + 1) & 3))) & 255u;
        b[k] = (w[(3 * k + 2) >> 2] >> (8 * ((3 * k + 2) & 3))) & 255u;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = p[0], g[k] = p[1], b[k] = p[2];
    }
  } else {
    const size_t hw = (size_t)H * W;
    const float* p = (const float*)px + (size_t)t * 3 * hw + (size_t)y * W + xc;
    float v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (inside) {
        const float4 f = *(const float4*)(p + c * hw);
        v[c][0] = f.x, v[c][1] = f.y, v[c][2] = f.z, v[c][3] = f.w;
      } else {
        v[c][0] = v[c][1] = v[c][2] = v[c][3] = p[c * hw];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = pixel_byte(v[0][k]), g[k] = pixel_byte(v[1][k]), b[k] = pixel_byte(v[2][k]);
  }

  // every product and sum below is spelled out (fmaf / __fmul_rn): the two instantiations must round alike
  const int m = xq >> 2, xl = (xq & 3) * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float yv = fmaf(0.114f, (float)b[k], fmaf(0.587f, (float)g[k], fmaf(0.299f, (float)r[k], -128.0f)));
    const int xx = xl + k;
    S[(m * 6 + (row >> 3) * 2 + (xx >> 3)) * TR_BLK + (row & 7) * TR_ROW + (xx & 7)] = yv;
  }
  // chroma: the sums of the 2x2 blocks are exact integers; rows 2j and 2j + 1 are lanes l and l ^ 16 of one wave
  int sr[2] = {r[0] + r[1], r[2] + r[3]}, sg[2] = {g[0] + g[1], g[2] + g[3]}, sb[2] = {b[0] + b[1], b[2] + b[3]};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    sr[j] += __shfl_xor(sr[j], 16);
    sg[j] += __shfl_xor(sg[j], 16);
    sb[j] += __shfl_xor(sb[j], 16);
  }
  if (!(row & 1)) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float R = (float)sr[j], G = (float)sg[j], B = (float)sb[j];
      const float cb = __fmul_rn(0.25f, fmaf(0.5f, B, fmaf(-0.331264f, G, __fmul_rn(-0.168736f, R))));   // + 128 - 128
      const float cr = __fmul_rn(0.25f, fmaf(-0.081312f, B, fmaf(-0.418688f, G, __fmul_rn(0.5f, R))));
      const int at = (row >> 1) * TR_ROW + (xq & 3) * 2 + j;
      S[(m * 6 + 4) * TR_BLK + at] = cb;
      S[(m * 6 + 5) * TR_BLK + at] = cr;
    }
  }
  __syncthreads();

  const int blk = tid >> 3, line = tid & 7;                // threads 0 .. 191: block, and its column (pass 1) or row (pass 2)
  float in[8], out[8];
  if (blk < TR_BLOCKS) {                                   // G[v][x] = sum_y C[v][y] f[y][x], in place: the column is this thread's
    float* col = S + blk * TR_BLK + line;
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = col[k * TR_ROW];
    dct8(in, out);
#pragma unroll
    for (int k = 0; k < 8; ++k) col[k * TR_ROW] = out[k];
  }
  __syncthreads();
  if (blk < TR_BLOCKS) {                                   // F[v][u] = sum_x C[u][x] G[v][x]
    const float* rowp = S + blk * TR_BLK + line * TR_ROW;
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = rowp[k];
    dct8(in, out);
    const float* step = rq + ((blk % 6) >= 4 ? 64 : 0) + line * 8;
    const bool dummy = outside(mcu0 + blk / 6, my, blk % 6, H, W);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float c = __fmul_rn(out[u], step[u]);
      const int a = (int)floorf(__fadd_rn(fabsf(c), 0.5f));   // half away from zero
      // what the Huffman tables can code (AC of 10 bits, DC differences of 11); the DCT of 8-bit samples stays inside anyway
      const int v = min(max(c < 0.0f ? -a : a, line + u ? -1023 : -1024), 1023);
      staged[blk * 64 + zz[line * 8 + u]] = dummy ? (int16_t)0 : (int16_t)v;
    }
  }
  __syncthreads();
  if (tid < TR_MCUS) {                                     // dummy luma blocks repeat the DC of the block coded before them
    for (int k = 1; k < 4; ++k)
      if (outside(mcu0 + tid, my, k, H, W)) staged[(tid * 6 + k) * 64] = staged[(tid * 6 + k - 1) * 64];
  }
  __syncthreads();
  const int nv = min(TR_MCUS, mcus - mcu0);                // MCUs of this workgroup inside the frame
  uint32_t* dst = (uint32_t*)(coef + (((size_t)t * gridDim.y + my) * mcus + mcu0) * 384);
  for (int i = tid; i < nv * 192; i += 256) dst[i] = ((const uint32_t*)staged)[i];
}

// ------------------------------------------------------------------------------------------------------------------------ entropy
struct BitWriter {        // MSB-first bit string in 32-bit words: bit p of the string is bit 31 - p % 32 of word p / 32
  uint32_t* word;
  uint64_t acc;
  int held;
  __device__ __forceinline__ BitWriter(uint32_t* seg, int bit) : word(seg + (bit >> 5)), acc(0), held(bit & 31) {}
  __device__ __forceinline__ void put(uint32_t v, int len) {          // len <= 26
    acc = (acc << len) | v;
    held += len;
    if (held >= 32) {
      atomicOr(word++, (uint32_t)(acc >> (held - 32)));
      held -= 32;
    }
  }
  __device__ __forceinline__ void flush() {
    if (held) atomicOr(word, (uint32_t)(acc << (32 - held)));
  }
};

struct BitCounter {
  int bits = 0;
  __device__ __forceinline__ void put(uint32_t, int len) { bits += len; }
};

// the block's predecessor of the same component inside the segment (MCU = Y00 Y01 Y10 Y11 Cb Cr), -1 at the restart
__device__ __forceinline__ int dc_predecessor(int b) {
  const int m = b / 6, k = b - m * 6;
  if (k >= 1 && k <= 3) return b - 1;
  if (m == 0) return -1;
  return k == 0 ? b - 3 : b - 6;
}

template <class Sink>
__device__ __forceinline__ void code_value(int v, uint32_t entry, int s, Sink& sink) {   // Huffman code of the symbol, then s value bits
  const uint32_t bits = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u);
  sink.put(((entry >> 8) << s) | bits, (int)(entry & 255u) + s);
}

template <class Sink>
__device__ __forceinline__ void code_block(const int16_t* blk, int pred, const uint32_t* dcT, const uint32_t* acT, Sink& sink) {
  const u32x4* p = (const u32x4*)blk;
  int run = 0;
#pragma unroll 1
  for (int q8 = 0; q8 < 8; ++q8) {
    const u32x4 v = p[q8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = (int)(int16_t)(uint16_t)(v[j >> 1] >> (16 * (j & 1)));
      if (q8 == 0 && j == 0) {                             // DC: the difference to the predecessor, size category 0 .. 11
        const int d = c - pred;
        const int s = 32 - __clz(abs(d));
        code_value(d, dcT[s], s, sink);
      } else if (c == 0) {
        ++run;
      } else {
        while (run >= 16) {                                // ZRL
          sink.put(acT[0xF0] >> 8, (int)(acT[0xF0] & 255u));
          run -= 16;
        }
        const int s = 32 - __clz(abs(c));
        code_value(c, acT[(run << 4) | s], s, sink);
        run = 0;
      }
    }
  }
  if (run) sink.put(acT[0] >> 8, (int)(acT[0] & 255u));   // EOB
}

__global__ void __launch_bounds__(256) jpeg_entropy_kernel(const int16_t* __restrict__ coef, uint32_t* __restrict__ raw, int* __restrict__ seginfo,
                                                           int mcus, int raw_words, const HuffArg h) {
  __shared__ uint32_t dcT[2][12], acT[2][256];
  __shared__ int scan[4];
  const int tid = threadIdx.x, seg = blockIdx.x;
  if (tid < 24) dcT[tid / 12][tid % 12] = h.dc[tid / 12][tid % 12];
  for (int i = tid; i < 512; i += 256) acT[i >> 8][i & 255] = h.ac[i >> 8][i & 255];
  __syncthreads();

  const int nblocks = mcus * 6, per = (nblocks + 255) / 256;
  const int b0 = min(tid * per, nblocks), b1 = min(b0 + per, nblocks);
  const int16_t* segc = coef + (size_t)seg * nblocks * 64;
  uint32_t* segraw = raw + (size_t)seg * raw_words;

  BitCounter counter;
  for (int b = b0; b < b1; ++b) {
    const int pb = dc_predecessor(b), comp = (b % 6) >= 4;
    code_block(segc + (size_t)b * 64, pb < 0 ? 0 : (int)segc[(size_t)pb * 64], dcT[comp], acT[comp], counter);
  }
  int total_bits;
  const int bit0 = block_scan_exclusive(counter.bits, scan, &total_bits);
  const int nbytes = (total_bits + 7) >> 3, nwords = min((nbytes + 3) >> 2, raw_words);   // nblocks * 1658 bits at most: inside raw_words
  for (int i = tid; i < nwords; i += 256) segraw[i] = 0u;
  __threadfence();                                         // the zeros are in place before any lane ORs into them
  __syncthreads();

  BitWriter writer(segraw, bit0);
  for (int b = b0; b < b1; ++b) {
    const int pb = dc_predecessor(b), comp = (b % 6) >= 4;
    code_block(segc + (size_t)b * 64, pb < 0 ? 0 : (int)segc[(size_t)pb * 64], dcT[comp], acT[comp], writer);
  }
  writer.flush();
  if (tid == 0 && (total_bits & 7)) {                      // pad the last byte with 1 bits
    const int pad = 8 - (total_bits & 7);
    BitWriter tail(segraw, total_bits);
    tail.put((1u << pad) - 1u, pad);
    tail.flush();
  }
  __threadfence();
  __syncthreads();

  int ff = 0;                                              // the words were built by atomics in L2: read them there
  for (int i = tid; i < nwords; i += 256) {
    const uint32_t w = __hip_atomic_load(segraw + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int k = 0; k < 4; ++k) ff += ((w >> (8 * k)) & 255u) == 255u;   // bytes behind nbytes are zero
  }
  int total_ff;
  block_scan_exclusive(ff, scan, &total_ff);
  if (tid == 0) {
    seginfo[2 * seg] = nbytes;
    seginfo[2 * seg + 1] = nbytes + total_ff;
  }
}

// ----------------------------------------------------------------------------------------------------------------------- assemble
__global__ void __launch_bounds__(256) jpeg_assemble_kernel(const uint32_t* __restrict__ raw, const int* __restrict__ seginfo, int raw_words,
                                                            uint8_t* __restrict__ out, size_t out_cap, int64_t* __restrict__ offsets,
                                                            const HeaderArg hdr) {
  __shared__ unsigned long long before;
  __shared__ int scan[4];
  const int tid = threadIdx.x, r = blockIdx.x, t = blockIdx.y, rows = gridDim.x, T = gridDim.y;
  const int seg = t * rows + r;
  if (tid == 0) before = 0ull;
  __syncthreads();
  unsigned long long mine = 0ull;
  for (int i = tid; i < seg; i += 256) mine += (unsigned long long)seginfo[2 * i + 1];
  if (mine) atomicAdd(&before, mine);
  __syncthreads();
  // a frame = header, segments with RSTn between them, EOI
  const int64_t frame_fixed = (int64_t)hdr.len + 2 * (rows - 1) + 2;
  const int64_t start = (int64_t)before + t * frame_fixed + hdr.len + 2 * r;       // of this segment's first byte
  auto store = [&](int64_t at, uint32_t v) {
    if ((uint64_t)at < (uint64_t)out_cap) out[at] = (uint8_t)v;
  };
  if (r == 0) {
    for (int i = tid; i < hdr.len; i += 256) store(start - hdr.len + i, hdr.bytes[i]);
    if (tid == 0) offsets[t] = start - hdr.len;
  } else if (tid < 2) {
    store(start - 2 + tid, tid ? 0xD0u + ((r - 1) & 7) : 0xFFu);
  }
  const int nbytes = seginfo[2 * seg];
  const uint32_t* segraw = raw + (size_t)seg * raw_words;
  int64_t at = start;                                      // of the round's first byte
  for (int w0 = 0; w0 * 4 < nbytes; w0 += 256) {           // rounds of 256 words: a lane's word, and where the 0xFF before it push it
    const int w = w0 + tid, have = min(max(nbytes - w * 4, 0), 4);
    const uint32_t word = have ? segraw[w] : 0u;
    int ff = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) ff += k < have && ((word >> (24 - 8 * k)) & 255u) == 255u;
    int round_ff;
    int64_t o = at + tid * 4 + block_scan_exclusive(ff, scan, &round_ff);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < have) {
        const uint32_t byte = (word >> (24 - 8 * k)) & 255u;
        store(o++, byte);
        if (byte == 255u) store(o++, 0u);
      }
    }
    at += 1024 + round_ff;
  }
  if (r == rows - 1) {
    const int64_t end = start + seginfo[2 * seg + 1];
    if (tid < 2) store(end + tid, tid ? 0xD9u : 0xFFu);    // EOI
    if (tid == 0 && t == T - 1) offsets[T] = end + 2;
  }
}

// --------------------------------------------------------------------------------------------------------------------------- host
struct JpegPlan {
  int mcus, rows;
  int raw_words;                     // per segment
  size_t coef_bytes, raw_bytes, info_bytes;
  size_t arena_bytes() const { return coef_bytes + raw_bytes + info_bytes; }
};

const char* plan(int T, int H, int W, JpegPlan* p) {   // null = fine, else why not
  if (T <= 0 || H <= 0 || W <= 0) return "sizes must be positive";
  if (H % 8 || W % 8) return "H and W must be multiples of 8";
  if (H > JPEG_MAX_SIDE || W > JPEG_MAX_SIDE) return "H and W must be multiples of 8 up to 65528";
  if (T > RTV_FRAMES_MAX) return "T above RTV_FRAMES_MAX (16) frames per call";
  p->mcus = (W + 15) / 16;
  p->rows = (H + 15) / 16;
  p->raw_words = p->mcus * 6 * (JPEG_BLOCK_BOUND_BYTES / 4);
  const size_t segs = (size_t)T * p->rows;
  p->coef_bytes = segs * p->mcus * 6 * 64 * sizeof(int16_t);        // a multiple of 256
  p->raw_bytes = segs * p->raw_words * 4;                            // a multiple of 16
  p->info_bytes = segs * 2 * sizeof(int);
  return nullptr;
}

int fail(const char* fn, const char* why) {
  char msg[192];
  snprintf(msg, sizeof(msg), "%s: %s", fn, why);
  return set_error(-1, msg);
}

int check_call(const char* fn, const void* pixels, int rgb8, int T, int H, int W, int quality, const void* arena, size_t arena_bytes,
               const void* out, const void* offsets, JpegPlan* p) {
  if (!pixels || !arena || !out || !offsets) return fail(fn, "null argument");
  if (const char* why = plan(T, H, W, p)) return fail(fn, why);
  if (quality < 1 || quality > 100) return fail(fn, "quality must be in 1..100");
  if (arena_bytes < p->arena_bytes()) return fail(fn, "arena smaller than rtv_jpeg_arena_bytes(T, H, W)");
  if ((uintptr_t)arena & 15) return fail(fn, "arena must be 16-byte aligned");
  if (!rgb8 && ((uintptr_t)pixels & 15)) return fail(fn, "float pixels must be 16-byte aligned");
  return 0;
}

int launch_transform(const char* fn, const void* pixels, int rgb8, int T, int H, int W, int quality, void* arena, const JpegPlan& p,
                     hipStream_t stream) {
  QuantArg q;
  for (int c = 0; c < 2; ++c) {
    uint8_t steps[64];
    quant_steps(quality, c, steps);
    for (int i = 0; i < 64; ++i) q.rq[c][i] = 1.0f / (float)steps[i];
  }
  for (int i = 0; i < 64; ++i) q.zz[kZigzag[i]] = (uint8_t)i;
  const dim3 grid((p.mcus + TR_MCUS - 1) / TR_MCUS, p.rows, T);
  ProfScope prof(PROF_MISC, stream, (double)T * H * W * (rgb8 ? 3.0 : 12.0) + (double)p.coef_bytes);
  if (rgb8)
    hipLaunchKernelGGL(jpeg_transform_kernel<true>, grid, dim3(256), 0, stream, pixels, (int16_t*)arena, H, W, p.mcus, q);
  else
    hipLaunchKernelGGL(jpeg_transform_kernel<false>, grid, dim3(256), 0, stream, pixels, (int16_t*)arena, H, W, p.mcus, q);
  return check_launch(fn);
}

}  // namespace
}  // namespace rtv

using namespace rtv;

extern "C" {

size_t rtv_jpeg_header(int quality, int H, int W, void* host_buf, size_t cap) {
  const char* why = nullptr;
  JpegPlan p;
  if (!host_buf) why = "null argument";
  else if ((why = plan(1, H, W, &p))) {}
  else if (quality < 1 || quality > 100) why = "quality must be in 1..100";
  else if (cap < (size_t)JPEG_HEADER_BYTES) why = "cap below the header's 629 bytes";
  if (why) {
    fail("jpeg_header", why);
    return 0;
  }
  return write_header(quality, H, W, (uint8_t*)host_buf);
}

size_t rtv_jpeg_arena_bytes(int T, int H, int W) {
  JpegPlan p;
  return plan(T, H, W, &p) ? 0 : p.arena_bytes();
}

size_t rtv_jpeg_out_bound(int T, int H, int W) {
  JpegPlan p;
  if (plan(T, H, W, &p)) return 0;
  // per frame: header, EOI, and per MCU row a marker (the first row has none) and the segment bound with every byte stuffed
  return (size_t)T * (JPEG_HEADER_BYTES + 2 + (size_t)p.rows * (2 + 2 * (size_t)p.raw_words * 4));
}

int rtv_jpeg_encode(const void* pixels, int pixels_are_rgb8, int T, int H, int W, int quality, void* arena, size_t arena_bytes,
                    void* out, size_t out_cap, void* offsets, rtv_stream_t stream) {
  if (T == 0) return 0;
  JpegPlan p;
  if (int e = check_call("jpeg_encode", pixels, pixels_are_rgb8, T, H, W, quality, arena, arena_bytes, out, offsets, &p)) return e;
  hipStream_t s = (hipStream_t)stream;
  if (int e = launch_transform("jpeg_encode (transform)", pixels, pixels_are_rgb8, T, H, W, quality, arena, p, s)) return e;
  int16_t* coef = (int16_t*)arena;
  uint32_t* raw = (uint32_t*)((char*)arena + p.coef_bytes);
  int* seginfo = (int*)((char*)arena + p.coef_bytes + p.raw_bytes);
  {
    ProfScope prof(PROF_MISC, s, 2.0 * (double)p.coef_bytes);
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(T * p.rows), dim3(256), 0, s, coef, raw, seginfo, p.mcus, p.raw_words, huff_tables());
    if (int e = check_launch("jpeg_encode (entropy)")) return e;
  }
  HeaderArg hdr = {};
  hdr.len = (int)write_header(quality, H, W, hdr.bytes);
  ProfScope prof(PROF_MISC, s, (double)T * H * W * 0.5);
  hipLaunchKernelGGL(jpeg_assemble_kernel, dim3(p.rows, T), dim3(256), 0, s, raw, seginfo, p.raw_words, (uint8_t*)out, out_cap,
                     (int64_t*)offsets, hdr);
  return check_launch("jpeg_encode (assemble)");
}

int rtv_jpeg_coefficients(const void* pixels, int pixels_are_rgb8, int T, int H, int W, int quality, void* arena,
                          size_t arena_bytes, void* coefficients, rtv_stream_t stream) {
  if (T == 0) return 0;
  JpegPlan p;
  if (int e = check_call("jpeg_coefficients", pixels, pixels_are_rgb8, T, H, W, quality, arena, arena_bytes, coefficients, coefficients, &p))
    return e;
  if (int e = launch_transform("jpeg_coefficients", pixels, pixels_are_rgb8, T, H, W, quality, arena, p, (hipStream_t)stream)) return e;
  if (hipMemcpyAsync(coefficients, arena, p.coef_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
    return fail("jpeg_coefficients", "copying the coefficients failed");
  return 0;
}

}  // extern "C"
