// Pixel input side: rgb8 camera frames [T][Hin][Win][3] -> the VAE encoder's input, fp16 [3][T][H][W] in [-1, 1], one launch per
// block of frames (include/rtv_hip_io.h).  The arithmetic is the reference's, restated:
//
//   decode  release_server.py:479  TF.to_tensor(image).to(dtype=torch.float16)   x = fp16(float(u) / 255.0f)
//           release_server.py:481  tensor.to(gpu).sub_(0.5).mul_(2.0)            y = fp16(fp16(float(x) - 0.5f) * 2.0f)
//           (half arithmetic in torch = fp32 operation, one rounding per op).  A byte has 256 values: every workgroup builds the
//           256-entry table of y in LDS once, which is exact by construction and keeps the divide out of the tap loop.
//   resize  v2v.py:153  F.interpolate(frames, size=(h, w), mode='bicubic')       align_corners=False, A = -0.75, no antialiasing:
//           source coordinate s = scale * (dst + 0.5) - 0.5 with scale = in / out in fp32, i = floor(s), t = s - i, taps i-1 .. i+2
//           clamped to the border, weights W(t+1), w(t), w(1-t), W(2-t) with w(x) = ((A+2)x - (A+3))x^2 + 1 and
//           W(x) = ((Ax - 5A)x + 8A)x - 4A; every source row is interpolated along x, then the four rows along y, all in fp32
//           (torch's order), and the sum is rounded once to fp16.  Nothing is clamped: overshoot to about +-1.35 and the aliasing of
//           a downscale are the reference's behaviour.
//   layout  v2v.py:153  .transpose(0, 1)                                         out[c][t][y][x]
//
// Resize kernel: one workgroup = one tile of (8 * tw8) x th output pixels of one frame.  The decoded source footprint of the tile
// goes through LDS (aligned 4-byte global loads wherever a word lies inside the footprint's row segment, single bytes at its two
// ends: 3 * Win is no multiple of 4 for most widths), the tap offsets and weights of the tile's columns and rows are computed once
// per tile, and every thread produces 8 consecutive columns of one row for the three planes: three 16-byte stores.
#include "rtv_common.h"
#include "rtv_internal.h"
#include "../../include/rtv_hip_io.h"

namespace rtv {
namespace {

struct FrameSlots {
  int idx[RTV_FRAMES_MAX];
};

constexpr int FI_LDS_LIMIT = 64 * 1024;   // static + dynamic LDS of one workgroup without a function attribute

__device__ __forceinline__ void build_decode_table(f16_t* tab) {
  for (int u = threadIdx.x; u < 256; u += blockDim.x) {
    const _Float16 x = (_Float16)__fdiv_rn((float)u, 255.0f);
    const _Float16 y = (_Float16)__fsub_rn((float)x, 0.5f);
    const _Float16 z = (_Float16)__fmul_rn((float)y, 2.0f);
    f16_t r;
    __builtin_memcpy(&r, &z, 2);
    tab[u] = r;
  }
}

// torch area_pixel_compute_source_index(scale, dst, align_corners=false, cubic=true), then floor / fraction
__device__ __forceinline__ int source_index(float scale, int dst, float* t) {
  const float s = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f);
  const float fl = floorf(s);
  *t = __fsub_rn(s, fl);
  return (int)fl;
}

__device__ __forceinline__ void cubic_weights(float t, float* w) {   // torch get_cubic_upsample_coefficients, A = -0.75
  const float A = -0.75f;
  float x = t + 1.0f;
  w[0] = ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
  x = t;
  w[1] = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
  x = 1.0f - t;
  w[2] = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
  x = 2.0f - t;
  w[3] = ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct ResizeArgs {
  const uint8_t* rgb8;
  f16_t* out;
  FrameSlots slots;
  int64_t slot_stride;
  int Hin, Win, H, W, out_T, out_t0;
  float sy, sx;
  int tw8, th;       // tile: 8 * tw8 columns x th rows, tw8 * th threads
  int nc_max, nr_max;   // LDS footprint: nr_max rows of nc_max pixels (3 fp16 each)
};

// dynamic LDS: f16 tab[256] | float wx[TW][4] | int cx[TW][4] | float wy[th][4] | int ry[th][4] | f16 src[nr_max][3 * nc_max]
__global__ void __launch_bounds__(256) frames_resize_kernel(const ResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fi_smem[];
  const int TW = a.tw8 * 8, th = a.th, nthr = a.tw8 * a.th;
  f16_t* tab = (f16_t*)fi_smem;
  float* wx = (float*)(fi_smem + 512);
  int* cx = (int*)(wx + TW * 4);
  float* wy = (float*)(cx + TW * 4);
  int* ry = (int*)(wy + th * 4);
  f16_t* src = (f16_t*)(ry + th * 4);
  const int pitch = 3 * a.nc_max;                 // fp16 elements per footprint row

  const int tid = threadIdx.x;
  const int ox0 = blockIdx.x * TW, oy0 = blockIdx.y * th, t = blockIdx.z;
  const int ox1 = min(ox0 + TW, a.W) - 1, oy1 = min(oy0 + th, a.H) - 1;
  float frac;
  // the footprint: source_index is monotonic in dst, so every clamped tap of the tile lies in [xlo, xhi] x [ylo, yhi]
  const int xlo = clampi(source_index(a.sx, ox0, &frac) - 1, 0, a.Win - 1);
  const int xhi = clampi(source_index(a.sx, ox1, &frac) + 2, 0, a.Win - 1);
  const int ylo = clampi(source_index(a.sy, oy0, &frac) - 1, 0, a.Hin - 1);
  const int yhi = clampi(source_index(a.sy, oy1, &frac) + 2, 0, a.Hin - 1);
  const int nc = min(xhi - xlo + 1, a.nc_max), nr = min(yhi - ylo + 1, a.nr_max);   // the host's bounds hold; never write past them

  build_decode_table(tab);
  for (int i = tid; i < TW + th; i += nthr) {     // tap offsets (in fp16 elements of the footprint) and weights, once per tile
    const bool col = i < TW;
    const int j = col ? i : i - TW;
    float w[4];
    const int s = source_index(col ? a.sx : a.sy, (col ? ox0 : oy0) + j, &frac);
    cubic_weights(frac, w);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col) {
        wx[j * 4 + k] = w[k];
        cx[j * 4 + k] = 3 * clampi(clampi(s - 1 + k, 0, a.Win - 1) - xlo, 0, nc - 1);
      } else {
        wy[j * 4 + k] = w[k];
        ry[j * 4 + k] = pitch * clampi(clampi(s - 1 + k, 0, a.Hin - 1) - ylo, 0, nr - 1);
      }
    }
  }
  __syncthreads();                                 // the table is read below

  // stage the footprint: row r = source row ylo + r, bytes [3 * xlo, 3 * (xlo + nc)) of it, as aligned words where they fit
  const uint8_t* frame = a.rgb8 + (size_t)a.slots.idx[t] * (size_t)a.slot_stride;
  const int row_bytes = 3 * nc;
  const int nw = (row_bytes + 3) / 4 + 1;         // aligned words that can touch one row segment
  for (int i = tid; i < nr * nw; i += nthr) {
    const int r = i / nw, wi = i - r * nw;
    const uint8_t* g0 = frame + ((size_t)(ylo + r) * a.Win + xlo) * 3;
    const uint8_t* p = (const uint8_t*)((uintptr_t)g0 & ~(uintptr_t)3) + 4 * wi;
    const int rel = (int)(p - g0);                // -3 .. row_bytes + 3
    f16_t* dst = src + r * pitch;
    if (rel >= 0 && rel + 4 <= row_bytes) {
      const uint32_t v = *(const uint32_t*)p;
#pragma unroll
      for (int b = 0; b < 4; ++b) dst[rel + b] = tab[(v >> (8 * b)) & 255u];
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (rel + b >= 0 && rel + b < row_bytes) dst[rel + b] = tab[p[b]];
    }
  }
  __syncthreads();

  const int tx = tid % a.tw8, ty = tid / a.tw8;
  const int ox = ox0 + tx * 8, oy = oy0 + ty;
  if (ox >= a.W || oy >= a.H) return;             // W is a multiple of 8: a thread's 8 columns are all inside or all outside
  float wr[4];
  const f16_t* rows[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    wr[k] = wy[ty * 4 + k];
    rows[k] = src + ry[ty * 4 + k];
  }
  // two columns per trip (rolled: the 96 taps of a trip are what the registers hold at once), a trip's word goes into place by select
  u32x4 v[3] = {};
#pragma unroll 1
  for (int q = 0; q < 4; ++q) {
    float acc[3][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = tx * 8 + 2 * q + j;
      const f32x4 wc = *(const f32x4*)(wx + col * 4);
      int off[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) off[k] = cx[col * 4 + k];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float s = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const f16_t* row = rows[r] + c;
          const float h = f16_to_f32(row[off[0]]) * wc[0] + f16_to_f32(row[off[1]]) * wc[1] + f16_to_f32(row[off[2]]) * wc[2] +
                          f16_to_f32(row[off[3]]) * wc[3];
          s += h * wr[r];
        }
        acc[c][j] = s;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t w = pack_f16x2(acc[c][0], acc[c][1]);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[c][k] = k == q ? w : v[c][k];
    }
  }
  const size_t plane = (size_t)a.H * a.W;
  f16_t* o = a.out + ((size_t)(a.out_t0 + t)) * plane + (size_t)oy * a.W + ox;
#pragma unroll
  for (int c = 0; c < 3; ++c) *(u32x4*)(o + (size_t)c * a.out_T * plane) = v[c];
}

// (Hin, Win) == (H, W): the table value, bit for bit.  One thread = 8 pixels = 24 source bytes (W % 8 == 0: never across frames).
__global__ void __launch_bounds__(256) frames_decode_kernel(const uint8_t* __restrict__ rgb8, const FrameSlots slots, int64_t slot_stride, int T,
                                     size_t hw, f16_t* __restrict__ out, int out_T, int out_t0) {
  __shared__ f16_t tab[256];
  build_decode_table(tab);
  __syncthreads();
  const size_t groups = hw >> 3, total = (size_t)T * groups;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t t = i / groups, q = i - t * groups;
    const uint8_t* p = rgb8 + (size_t)slots.idx[t] * (size_t)slot_stride + q * 24;
    uint32_t w[6];
    if (((uintptr_t)p & 3) == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) w[k] = ((const uint32_t*)p)[k];
    } else {
#pragma unroll
      for (int k = 0; k < 6; ++k)
        w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
    }
    f16_t* o = out + ((size_t)out_t0 + t) * hw + q * 8;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      u32x4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int b0 = 3 * (2 * k) + c, b1 = 3 * (2 * k + 1) + c;        // byte of pixel 2k / 2k+1, channel c
        const uint32_t lo = tab[(w[b0 >> 2] >> (8 * (b0 & 3))) & 255u], hi = tab[(w[b1 >> 2] >> (8 * (b1 & 3))) & 255u];
        v[k] = lo | (hi << 16);
      }
      *(u32x4*)(o + (size_t)c * out_T * hw) = v;
    }
  }
}

// LDS bytes of the resize kernel for a tile shape, and the footprint bounds the kernel is given.  A tile's taps span at most
// scale * (n - 1) + 4 source pixels (+ 1 for the fp32 coordinate rounding): floor(scale * (n - 1)) + 6 bounds the count.
size_t resize_lds(int tw8, int th, float sx, float sy, int Hin, int Win, int* nc_max, int* nr_max) {
  const int TW = tw8 * 8;
  const double nc = floor((double)sx * (TW - 1)) + 6.0, nr = floor((double)sy * (th - 1)) + 6.0;
  *nc_max = (int)fmin(nc, (double)Win);
  *nr_max = (int)fmin(nr, (double)Hin);
  return 512 + (size_t)(TW + th) * 32 + (size_t)*nr_max * *nc_max * 6;
}

}  // namespace
}  // namespace rtv

using namespace rtv;

extern "C" {

int rtv_frames_from_rgb8(const void* rgb8, const int* slots, int64_t slot_stride, int T, int Hin, int Win, void* out, int out_T,
                         int out_t0, int H, int W, rtv_stream_t stream) {
  if (T == 0) return 0;
  if (!rgb8 || !out) return set_error(-1, "frames_from_rgb8: null argument");
  if (T < 0 || Hin <= 0 || Win <= 0 || H <= 0 || W <= 0 || out_T <= 0)
    return set_error(-1, "frames_from_rgb8: sizes must be positive");
  if (T > RTV_FRAMES_MAX) return set_error(-1, "frames_from_rgb8: T above RTV_FRAMES_MAX (16) frames per call");
  if (H % 8 || W % 8) return set_error(-1, "frames_from_rgb8: H and W must be multiples of 8");
  if ((uintptr_t)out & 15) return set_error(-1, "frames_from_rgb8: out must be 16-byte aligned");
  if (out_t0 < 0 || out_t0 > out_T - T) return set_error(-1, "frames_from_rgb8: frames out_t0 .. out_t0 + T outside [0, out_T)");
  if (slot_stride < 0) return set_error(-1, "frames_from_rgb8: negative slot stride");
  FrameSlots fs;
  for (int i = 0; i < RTV_FRAMES_MAX; ++i) {
    fs.idx[i] = i < T ? (slots ? slots[i] : i) : 0;
    if (fs.idx[i] < 0) return set_error(-1, "frames_from_rgb8: negative slot index");
  }
  const size_t hw = (size_t)H * W;
  if (Hin == H && Win == W) {
    const size_t total = (size_t)T * (hw / 8);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 8192) blocks = 8192;
    ProfScope prof(PROF_MISC, (hipStream_t)stream, (double)T * (3.0 * Hin * Win + 6.0 * hw));
    hipLaunchKernelGGL(frames_decode_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)rgb8, fs, slot_stride,
                       T, hw, (f16_t*)out, out_T, out_t0);
    return check_launch("frames_from_rgb8 (decode)");
  }
  ResizeArgs a;
  a.rgb8 = (const uint8_t*)rgb8;
  a.out = (f16_t*)out;
  a.slots = fs;
  a.slot_stride = slot_stride;
  a.Hin = Hin, a.Win = Win, a.H = H, a.W = W, a.out_T = out_T, a.out_t0 = out_t0;
  a.sy = (float)Hin / (float)H;                   // torch area_pixel_compute_scale<float>: in / out
  a.sx = (float)Win / (float)W;
  // the largest tile whose source footprint fits the LDS: 128 x 16 up to a ~2x downscale, smaller tiles beyond
  static const int tiles[4][2] = {{16, 16}, {8, 8}, {4, 4}, {2, 2}};
  size_t lds = 0;
  int pick = -1;
  for (int i = 0; i < 4 && pick < 0; ++i) {
    lds = resize_lds(tiles[i][0], tiles[i][1], a.sx, a.sy, Hin, Win, &a.nc_max, &a.nr_max);
    if (lds <= (size_t)FI_LDS_LIMIT) pick = i;
  }
  if (pick < 0) return set_error(-1, "frames_from_rgb8: downscale too strong, the source footprint of a 16 x 2 tile exceeds the LDS");
  a.tw8 = tiles[pick][0], a.th = tiles[pick][1];
  const dim3 grid((W + 8 * a.tw8 - 1) / (8 * a.tw8), (H + a.th - 1) / a.th, T);
  if (grid.y > 65535u) return set_error(-1, "frames_from_rgb8: output too tall for this tile");
  ProfScope prof(PROF_MISC, (hipStream_t)stream, (double)T * (3.0 * Hin * Win + 6.0 * hw));
  hipLaunchKernelGGL(frames_resize_kernel, grid, dim3(a.tw8 * a.th), lds, (hipStream_t)stream, a);
  return check_launch("frames_from_rgb8 (resize)");
}

}  // extern "C"
