// TAEHV tiny-VAE streaming decoder (the `decoder` nn.Sequential of demo_utils/taehv.py:159-234, checkpoint taew2_1.pth for
// Wan 2.1): the opt-in fast decode behind `use_taehv`.  fp16 channels-last activations, fp32 accumulation on MFMA.
// The streaming encoder (the `encoder` of the same module) follows the decoder, from "encoder" below on.
//
// Every layer is a 3x3 'same' convolution run as an implicit GEMM (the LDS-DMA gather idiom of vae_conv.hip's
// conv_igemm_kernel, on its own kernel here so that the Wan decoder's code objects stay as they are):
//   out[pixel][co] = epilogue( sum_{dt, dy, dx, ci} in[slice t + dt][y + dy - 1][x + dx - 1][ci] * W[co][(dt * 3 + dy) * 3 + dx][ci] )
//   * MemBlock conv1 over cat[x_t, x_{t-1}] is a 2-slice convolution (kt = 2) over a [x_{t-1} | x_t] window of a concat buffer
//     [state | T new slices]: output frame t reads slices t and t + 1, the weight's time tap 0 holds the x_{t-1} half of
//     conv.0 (input channels C..2C-1), tap 1 the x_t half.  The channel concat is never materialised; slice 0 is the block's
//     carried state (its input at the previous frame, zeros on a stream's first call);
//   * nearest-2x upsampling is read through the gather (source = coordinate >> 1);
//   * TGrow (a bias-free 1x1 conv C -> stride * C, channel group s -> frame stride * t + s) is FOLDED into the 3x3 conv behind
//     it: nearest upsampling commutes with a 1x1 conv and the conv's zero padding is TGrow(0) = 0, so the composed filters
//     Wf[s * Cout + o][tap][c] = sum_c' Wconv[o][c'][tap] * Wtgrow[s * C + c'][c] (composed in fp32 on the host, then fp16)
//     give the same function; filter group s is scattered to frame stride * t + s in the epilogue (n_split).  Not bit-identical
//     with the unfolded two-layer form (one fp16 rounding of the composed weight instead of one of the TGrow output);
//   * epilogues: + bias, ReLU, the MemBlock tail ReLU(conv + bias + x_t) (x_t = the block's input slices), and the head
//     out = clamp(2 * (conv + bias) - 1, -1, 1) written as float32 [T][3][H][W] (3 filters padded to 8);
//   * Clamp (tanh(x / 3) * 3) is the prologue of the first conv: taehv_prep_kernel applies it while it transposes the latents
//     to channels-last and pads 16 -> 32 channels.
// The K order of an output pixel is (dt, dy, dx, channel slab), the same for every tile position and every T, and no
// launch splits K: a stream decoded as 3 + 3, 1 x 6 or 2 + 4 latent frames per call gives bit-identical pixels.  The tile
// configuration is chosen from the layer (Cout, head) only.
#include "gemm_core.h"
#include "rtv_internal.h"

#include <string>

namespace rtv {
namespace tae {

struct ConvParams {
  const uint16_t* in;        // [T + kt - 1][inH][inW][Cin]
  const uint16_t* w;         // [Cout][kt * 9][Cin]
  const uint16_t* bias;      // [Cout] or null
  const uint16_t* residual;  // [M][Cout] or null: out = ReLU(conv + bias + residual)
  void* out;                 // f16 [M][Cout] (n_split: f16 [2T][H][W][n_split]); head: float32 [T][3][H][W]
  const uint16_t* zeros;     // >= 16 bytes of zeros
  int T, H, W;               // output grid
  int inH, inW;              // input grid (H >> ups)
  int Cin, Cout, kt, ups, n_split, relu;
  int M, tiles_m, tiles_n;
  // encoder forms: DOWN kernels read input (2y + dy - 1, 2x + dx - 1) of slice t * tstride + dt; the latent head (HEAD == 2)
  // writes f16 planar [16][out_T][H][W] from frame out_j on
  int tstride, out_T, out_j;
};

template <int TN>
__device__ __forceinline__ int img_off(int row, int chunk, int half) {   // conv_img_off of vae_conv.hip (TN = 2)
  static_assert(TN == 2, "epilogue image laid out for two 32-filter blocks per wave");
  return row * 128 + ((chunk ^ (row & 7)) << 4) + ((half ^ ((row >> 3) & 1)) << 3);
}

template <int BM, int BN, int BK, int WM, int WN, int HEAD, bool DOWN>
__global__ __launch_bounds__(WM* WN * 64) void taehv_conv_kernel(ConvParams p) {
  typedef TileCfg<BM, BN, BK, WM, WN> Cfg;
  constexpr int STAGES = 3;
  constexpr int PIECES = Cfg::A_INST + Cfg::B_INST;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int id = xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n);
  const int tile_m = id / p.tiles_n, tile_n = id % p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const int cpos = lane % Cfg::CH;
  const int rsub = lane / Cfg::CH;
  const int HW = p.H * p.W;
  // per-lane gather state (see conv_igemm_kernel): base offset of the lane's pixel in the input, in-image bits of its 3 x 3
  // neighbourhood (bits 0-2 rows, 3-5 columns) and, with upsampling, the parities of its row / column (bits 6, 7)
  int base_off[Cfg::A_INST], flags[Cfg::A_INST];
#pragma unroll
  for (int i = 0; i < Cfg::A_INST; ++i) {
    const int row = (wave * Cfg::A_INST + i) * Cfg::RPI + rsub;
    const int m = min(m0 + row, p.M - 1);
    const int pt = m / HW;
    const int rem = m - pt * HW;
    const int py = rem / p.W, px = rem - py * p.W;
    int f = 0;
    if constexpr (DOWN) {
      // stride 2: the 3 x 3 neighbourhood is centred on input (2 py, 2 px); in-image bits are taken on the input grid
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (2 * py + k - 1 >= 0 && 2 * py + k - 1 < p.inH) f |= 1 << k;
        if (2 * px + k - 1 >= 0 && 2 * px + k - 1 < p.inW) f |= 8 << k;
      }
      flags[i] = f;
      base_off[i] = ((pt * p.tstride * p.inH + 2 * py) * p.inW + 2 * px) * p.Cin + Cfg::swz(row, cpos) * 8;
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (py + k - 1 >= 0 && py + k - 1 < p.H) f |= 1 << k;
        if (px + k - 1 >= 0 && px + k - 1 < p.W) f |= 8 << k;
      }
      if (p.ups) f |= ((py & 1) << 6) | ((px & 1) << 7);
      flags[i] = f;
      base_off[i] = ((pt * p.inH + (py >> p.ups)) * p.inW + (px >> p.ups)) * p.Cin + Cfg::swz(row, cpos) * 8;
    }
  }
  uint32_t b_off[Cfg::B_INST];
  const int Ktot = p.kt * 9 * p.Cin;
#pragma unroll
  for (int i = 0; i < Cfg::B_INST; ++i) {
    const int row = (wave * Cfg::B_INST + i) * Cfg::RPI + rsub;
    const int gn = min(n0 + row, p.Cout - 1);
    b_off[i] = (uint32_t)gn * (uint32_t)Ktot + Cfg::swz(row, cpos) * 8;
  }
  const int nk = p.kt * 9 * (p.Cin / BK);
  const int slice = p.inH * p.inW * p.Cin;

  int is_dt = 0, is_dy = 0, is_dx = 0, is_c = 0, is_ks = 0;
  const uint16_t* a_src[Cfg::A_INST];
  int a_live[Cfg::A_INST];
  auto tap_setup = [&]() __attribute__((always_inline)) {
    const int ry = is_dy - 1, rx = is_dx - 1;
    const int row_e = p.ups ? (ry >> 1) : ry, row_o = p.ups ? ((ry + 1) >> 1) : ry;
    const int col_e = p.ups ? (rx >> 1) : rx, col_o = p.ups ? ((rx + 1) >> 1) : rx;
    const int t_off = is_dt * slice;
    const int d_re = t_off + row_e * p.inW * p.Cin, d_ro = t_off + row_o * p.inW * p.Cin;
    const int d_ce = col_e * p.Cin, d_co = col_o * p.Cin;
#pragma unroll
    for (int i = 0; i < Cfg::A_INST; ++i) {
      const int f = flags[i];
      const bool ok = ((f >> is_dy) & (f >> (3 + is_dx)) & 1) != 0;
      const int off = base_off[i] + ((f & 64) ? d_ro : d_re) + ((f & 128) ? d_co : d_ce);
      a_src[i] = ok ? p.in + (ptrdiff_t)off : p.zeros;
      a_live[i] = ok ? 1 : 0;
    }
  };
  auto issue = [&]() __attribute__((always_inline)) {
    char* sA = smem + (is_ks % STAGES) * Cfg::STAGE_BYTES;
    char* sB = sA + Cfg::A_BYTES;
    if (is_c == 0) tap_setup();
#pragma unroll
    for (int i = 0; i < Cfg::A_INST; ++i) dma16(a_src[i] + a_live[i] * is_c, sA + (wave * Cfg::A_INST + i) * 1024);
    const uint16_t* Wk = p.w + (size_t)is_ks * BK;
#pragma unroll
    for (int i = 0; i < Cfg::B_INST; ++i) dma16(Wk + b_off[i], sB + (wave * Cfg::B_INST + i) * 1024);
    ++is_ks;
    is_c += BK;
    if (is_c == p.Cin) {
      is_c = 0;
      if (++is_dx == 3) {
        is_dx = 0;
        if (++is_dy == 3) {
          is_dy = 0;
          ++is_dt;
        }
      }
    }
  };

  f32x16 acc[Cfg::TM][Cfg::TN];
#pragma unroll
  for (int mi = 0; mi < Cfg::TM; ++mi)
#pragma unroll
    for (int ni = 0; ni < Cfg::TN; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  const int wm = wave / WN, wn = wave % WN;
  const int a_row0 = wm * (BM / WM), b_row0 = wn * (BN / WN);

#define TV_FENCE() __builtin_amdgcn_sched_barrier(0)
  issue();
  if (nk > 1) issue();
  for (int ks = 0; ks < nk; ++ks) {
    if (ks + 1 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    TV_FENCE();
    __builtin_amdgcn_s_barrier();
    TV_FENCE();
    if (ks + 2 < nk) issue();
    TV_FENCE();
    const char* sA = smem + (ks % STAGES) * Cfg::STAGE_BYTES;
    mma_stage<true, Cfg, BK>(sA, sA + Cfg::A_BYTES, a_row0, b_row0, lane, acc);
    TV_FENCE();
  }
  __builtin_amdgcn_s_barrier();
  TV_FENCE();
#undef TV_FENCE

  const int l31 = lane & 31, g = lane >> 5;
  if constexpr (HEAD == 2) {
    // latent head: filters 0..15 sit in quads rq = 0, 1 of both half-waves (filter rq * 8 + g * 4 + i); f16 planar stores, 32
    // consecutive pixels per channel and instruction
    if (n0 + b_row0 != 0) return;
    uint16_t* out = (uint16_t*)p.out;
#pragma unroll
    for (int mi = 0; mi < Cfg::TM; ++mi) {
      const int m = m0 + a_row0 + mi * 32 + l31;
      if (m >= p.M) continue;
      const int t = m / HW, pix = m - t * HW;
#pragma unroll
      for (int rq = 0; rq < 2; ++rq)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int n = rq * 8 + g * 4 + i;
          const float v = acc[mi][0][rq * 4 + i] + (p.bias ? f16_to_f32(p.bias[n]) : 0.f);
          out[((size_t)n * p.out_T + p.out_j + t) * HW + pix] = f32_to_f16(v);
        }
    }
    return;
  } else if constexpr (HEAD == 1) {
    // filters 0..2 of the (one) 32-filter block sit in quad rq = 0 of the lanes with g = 0: float32 planar stores, 32
    // consecutive pixels per channel and instruction
    if (g != 0 || n0 + b_row0 != 0) return;
    float* out = (float*)p.out;
    const float b0 = p.bias ? f16_to_f32(p.bias[0]) : 0.f, b1 = p.bias ? f16_to_f32(p.bias[1]) : 0.f,
                b2 = p.bias ? f16_to_f32(p.bias[2]) : 0.f;
#pragma unroll
    for (int mi = 0; mi < Cfg::TM; ++mi) {
      const int m = m0 + a_row0 + mi * 32 + l31;
      if (m >= p.M) continue;
      const int t = m / HW, pix = m - t * HW;
      float* o = out + (size_t)t * 3 * HW + pix;
      o[0] = fminf(fmaxf(2.f * (acc[mi][0][0] + b0) - 1.f, -1.f), 1.f);
      o[HW] = fminf(fmaxf(2.f * (acc[mi][0][1] + b1) - 1.f, -1.f), 1.f);
      o[2 * (size_t)HW] = fminf(fmaxf(2.f * (acc[mi][0][2] + b2) - 1.f, -1.f), 1.f);
    }
    return;
  } else {
    // bias, then through a wave-private LDS image so that every lane moves 16 contiguous bytes of a pixel's channels;
    // residual + ReLU / ReLU on the way out
    constexpr int TM = Cfg::TM, TN = Cfg::TN, CPR = TN * 4;
    char* img = smem + wave * (TM * 32 * TN * 64);
    constexpr int PASSES = TM * 32 * CPR / 64;
    u32x4 res_pre[PASSES];
    if (p.residual) {
#pragma unroll
      for (int ps = 0; ps < PASSES; ++ps) {
        const int q = ps * 64 + lane;
        const int row = q / CPR, c = q - row * CPR;
        const int m = min(m0 + a_row0 + row, p.M - 1), n = min(n0 + b_row0 + c * 8, p.Cout - 8);   // clamped rows are never stored
        res_pre[ps] = *(const u32x4*)(p.residual + (size_t)m * p.Cout + n);
      }
    }
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
      const int row = mi * 32 + l31;
#pragma unroll
      for (int ni = 0; ni < TN; ++ni)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const int n = min(n0 + b_row0 + ni * 32 + rq * 8 + g * 4, p.Cout - 4);
          float v[4] = {acc[mi][ni][rq * 4 + 0], acc[mi][ni][rq * 4 + 1], acc[mi][ni][rq * 4 + 2], acc[mi][ni][rq * 4 + 3]};
          if (p.bias) {
            const u32x2 bb = *(const u32x2*)(p.bias + n);
            v[0] += f16_to_f32(bb[0] & 0xffff);
            v[1] += f16_to_f32(bb[0] >> 16);
            v[2] += f16_to_f32(bb[1] & 0xffff);
            v[3] += f16_to_f32(bb[1] >> 16);
          }
          u32x2 o;
          o[0] = pack_f16x2(v[0], v[1]);
          o[1] = pack_f16x2(v[2], v[3]);
          *(u32x2*)(img + img_off<TN>(row, ni * 4 + rq, g)) = o;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    uint16_t* out = (uint16_t*)p.out;
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
      const int q = ps * 64 + lane;
      const int row = q / CPR, c = q - row * CPR;
      const int m = m0 + a_row0 + row;
      const int n = n0 + b_row0 + c * 8;
      u32x4 t = *(const u32x4*)(img + img_off<TN>(row, c, 0) - (((row >> 3) & 1) << 3));   // chunk start; halves swapped on odd octets
      if ((row >> 3) & 1) t = u32x4{t[2], t[3], t[0], t[1]};
      if (m >= p.M || n >= p.Cout) continue;
      if (p.residual || p.relu) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float a0, a1;
          unpack_f16x2(t[i], a0, a1);
          if (p.residual) {
            float r0, r1;
            unpack_f16x2(res_pre[ps][i], r0, r1);
            a0 += r0;
            a1 += r1;
          }
          t[i] = pack_f16x2(fmaxf(a0, 0.f), fmaxf(a1, 0.f));
        }
      }
      size_t drow = (size_t)m;
      int ch = n, ld = p.Cout;
      if (p.n_split > 0) {
        const int tt = m / HW, pix = m - tt * HW;
        const int grp = n / p.n_split;
        drow = (size_t)(2 * tt + grp) * HW + pix;
        ch = n - grp * p.n_split;
        ld = p.n_split;
      }
      *(u32x4*)(out + drow * ld + ch) = t;
    }
  }
}

template <int BM, int BN, int BK, int WM, int WN, int HEAD, bool DOWN = false>
static int launch_cfg(ConvParams p, hipStream_t stream) {
  typedef TileCfg<BM, BN, BK, WM, WN> Cfg;
  static_assert(HEAD || Cfg::NW * Cfg::TM * 32 * Cfg::TN * 64 <= 3 * Cfg::STAGE_BYTES, "epilogue image must fit the stage buffers");
  static_assert(HEAD || Cfg::TN == 2, "epilogue image layout");
  static_assert(!HEAD || (BN == 32 && WN == 1), "head: one 32-filter block");
  p.tiles_m = (p.M + BM - 1) / BM;
  p.tiles_n = (p.Cout + BN - 1) / BN;
  const int lds = 3 * Cfg::STAGE_BYTES;
  auto kern = taehv_conv_kernel<BM, BN, BK, WM, WN, HEAD, DOWN>;
  static LdsAttr lds_attr;
  if (int st = ensure_dynamic_lds((const void*)kern, lds, &lds_attr, "taehv_conv")) return st;
  ProfScope prof(PROF_CONV, stream, 2.0 * p.M * (double)p.Cout * p.kt * 9 * p.Cin);
  hipLaunchKernelGGL(kern, dim3(p.tiles_m * p.tiles_n), dim3(Cfg::NT), lds, stream, p);
  return check_launch("taehv_conv");
}

// The common layer: one time tap, bias, no residual / upsampling / frame scatter / ReLU.  A call site sets what differs.
static ConvParams make_params(const void* in, rtv_vae_conv c, void* out, const void* zeros, int T, int H, int W, int Cin, int Cout) {
  ConvParams p{};
  p.in = (const uint16_t*)in;
  p.w = (const uint16_t*)c.w;
  p.bias = (const uint16_t*)c.b;
  p.out = out;
  p.zeros = (const uint16_t*)zeros;
  p.T = T;
  p.H = H;
  p.W = W;
  p.Cin = Cin;
  p.Cout = Cout;
  p.kt = 1;
  return p;
}

static int fail(const char* who, const char* what) { return set_error(-1, (std::string(who) + ": " + what).c_str()); }

// PLAIN (also the upsampled and frame-scattering forms) and RGB_HEAD are the layers of rtv_taehv_conv; DOWN (stride 2, the
// folded TPool's time taps) and LATENT_HEAD those of rtv_taehv_enc_conv
enum Form { PLAIN, RGB_HEAD, DOWN, LATENT_HEAD };

// One layer.  The kernel configuration is a function of the layer only (form or Cout), never of T / H / W.
static int launch_layer(ConvParams p, Form form, hipStream_t stream) {
  const bool enc = form == DOWN || form == LATENT_HEAD, head = form == RGB_HEAD || form == LATENT_HEAD;
  const char* who = enc ? "taehv_enc_conv" : "taehv_conv";
  if (!p.in || !p.w || !p.out || !p.zeros) return fail(who, "null pointer");
  if (p.T <= 0) return 0;
  if (p.H <= 0 || p.W <= 0) return fail(who, "bad size");
  if (p.kt != 1 && p.kt != 2) return fail(who, "kt must be 1 or 2");
  if (!enc) {
    if (p.ups != 0 && p.ups != 1) return fail(who, "ups must be 0 or 1");
    if (p.ups && ((p.H | p.W) & 1)) return fail(who, "upsampled output dims must be even");
    if (p.Cin <= 0 || p.Cin % 32) return fail(who, "Cin must be a multiple of 32 (pad channels)");
    if (head ? p.Cout != 8 : (p.Cout != 64 && p.Cout % 128 != 0)) return fail(who, "Cout must be 8 (head), 64 or a multiple of 128");
    if (head && (p.residual || p.n_split || p.relu)) return fail(who, "the head has a bias-only epilogue");
    if (p.n_split && (p.n_split % 8 || p.Cout != 2 * p.n_split)) return fail(who, "n_split must be Cout / 2");
    p.inH = p.H >> p.ups;
    p.inW = p.W >> p.ups;
    p.tstride = 1;
  } else {
    if (p.Cin != 64) return fail(who, "Cin must be 64");
    if (p.Cout != (head ? 16 : 64)) return fail(who, "Cout must be 64 (stride 2) or 16 (head)");
    if (head && (p.kt != 1 || p.out_j < 0 || p.out_T <= 0 || p.out_j + p.T > p.out_T))
      return fail(who, "head frames outside the output tensor");
    p.ups = 0;
    p.n_split = 0;
    p.relu = 0;
    p.residual = nullptr;
    p.inH = head ? p.H : 2 * p.H;
    p.inW = head ? p.W : 2 * p.W;
    p.tstride = head ? 1 : p.kt;   // the folded TPool(64, 2) reads the frame pair (2t, 2t + 1): windows do not overlap
  }
  // the latent head stores single 2-byte elements
  if ((((uintptr_t)p.in | (uintptr_t)p.w | (uintptr_t)p.residual | (uintptr_t)p.zeros) & 15) ||
      ((uintptr_t)p.out & (form == LATENT_HEAD ? 1 : 15)) || ((uintptr_t)p.bias & 7))
    return fail(who, "pointers must be 16-byte aligned (bias 8)");
  // the gather indexes the input (slices 0 .. (T - 1) * tstride + kt - 1) with 32-bit element offsets
  if (((size_t)(p.T - 1) * p.tstride + p.kt) * p.inH * p.inW * p.Cin >= 0x7fffffffull || (size_t)p.T * p.H * p.W >= 0x7fffffffull)
    return fail(who, "input too large for 32-bit offsets");
  p.M = p.T * p.H * p.W;
  if (form == RGB_HEAD) return launch_cfg<128, 32, 32, 2, 1, 1>(p, stream);
  if (form == PLAIN) return p.Cout == 64 ? launch_cfg<256, 64, 32, 4, 1, 0>(p, stream) : launch_cfg<128, 128, 32, 2, 2, 0>(p, stream);
  if (form == LATENT_HEAD) return launch_cfg<128, 32, 32, 2, 1, 2>(p, stream);
  return launch_cfg<256, 64, 32, 4, 1, 0, true>(p, stream);
}

// z fp16 [T][16][h][w] -> Clamp (tanh(x / 3) * 3) -> channels-last [T][h][w][32] (16 real + 16 zero channels)
__global__ void taehv_prep_kernel(const f16_t* __restrict__ z, int T, int hw, f16_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)T * hw) return;
  const int64_t t = i / hw, p = i - t * hw;
  u32x4 o[4];
#pragma unroll
  for (int c = 0; c < 16; c += 2) {
    const float a = f16_to_f32(z[(t * 16 + c) * hw + p]), b = f16_to_f32(z[(t * 16 + c + 1) * hw + p]);
    o[c >> 3][(c & 7) >> 1] = pack_f16x2(tanhf(a / 3.f) * 3.f, tanhf(b / 3.f) * 3.f);
  }
  o[2] = u32x4{0u, 0u, 0u, 0u};
  o[3] = u32x4{0u, 0u, 0u, 0u};
  u32x4* dst = (u32x4*)(out + i * 32);
  dst[0] = o[0];
  dst[1] = o[1];
  dst[2] = o[2];
  dst[3] = o[3];
}
// its launch: rtv_taehv_decode and the test entry rtv_taehv_prep both go through it
static int launch_prep(const void* z, int T, int hw, void* out, hipStream_t stream) {
  const int n = T * hw;
  hipLaunchKernelGGL(taehv_prep_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const f16_t*)z, T, hw, (f16_t*)out);
  return check_launch("taehv_prep");
}

// ---------------------------------------------------------------- arena
// [9 MemBlock state slices | codec region `pre` | per stage: two concat and two scratch buffers for calls of up to t_max
// frames | codec region `post` | zero page].  The state slices come first, at offsets that depend on the frame size only, so a
// stream can move to a larger arena by copying that prefix.
struct Stage {
  int H, W, C, F;   // geometry and frames per call of the stage's three MemBlocks
  // cat: [state | F new slices]; cat[0] takes the stage's input in slices 1..F, cat[1] holds its output there after three blocks
  size_t state[3], cat[2], tmp[2];
  size_t slice() const { return (size_t)H * W * C; }   // elements
};
struct Layout {
  Stage st[3];
  size_t state_bytes, pre, post, zeros, total;
};

static size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

// L->st[s].{H, W, C, F} are set by the caller
static void make_layout(Layout* L, size_t pre_bytes, size_t post_bytes) {
  size_t off = 0;
  for (Stage& g : L->st)
    for (size_t& o : g.state) {
      o = off;
      off += al(g.slice() * 2);
    }
  L->state_bytes = off;
  L->pre = off;
  off += al(pre_bytes);
  for (Stage& g : L->st) {
    for (size_t& o : g.cat) {
      o = off;
      off += al((size_t)(g.F + 1) * g.slice() * 2);
    }
    for (size_t& o : g.tmp) {
      o = off;
      off += al((size_t)g.F * g.slice() * 2);
    }
  }
  L->post = off;
  off += al(post_bytes);
  L->zeros = off;
  off += 256;
  L->total = off;
}

// Decoder: stages at (h, w) x 256, (2h, 2w) x 128, (4h, 4w) x 64 channels, the last at twice the latent frame rate.  pre = x0
// (the prepped latents, 32 channels), post = fin (one 64-channel frame pair at 8h x 8w)
static bool make_dec_layout(int h, int w, int t_max, Layout* L) {
  if (h <= 0 || w <= 0 || h > 1024 || w > 1024 || t_max < 0 || t_max > 4096) return false;
  for (int s = 0; s < 3; ++s) L->st[s] = Stage{h << s, w << s, 256 >> s, s < 2 ? t_max : 2 * t_max, {}, {}, {}};
  make_layout(L, (size_t)t_max * h * w * 32 * 2, (size_t)2 * (8 * h) * (8 * w) * 64 * 2);
  return true;
}

// One helper behind rtv_taehv_state_slot and rtv_taehv_enc_state_slot
static int state_slot(const Layout& L, const char* who, int slot, size_t* offset, int* C, int* H, int* W) {
  if (slot < 0 || slot >= 9) return fail(who, "state slot must be 0..8");
  const Stage& g = L.st[slot / 3];
  if (offset) *offset = g.state[slot % 3];
  if (C) *C = g.C;
  if (H) *H = g.H;
  if (W) *W = g.W;
  return 0;
}

// The three MemBlocks of a stage, each ReLU(conv.4(ReLU(conv.2(ReLU(conv.0 over [x_{t-1} | x_t])))) + x_t).  The stage's input
// is in slices 1..F of cat[0]; its output ends up in slices 1..F of cat[1].
static int run_memblocks(char* A, const Stage& g, const rtv_vae_conv (*mem)[3], const uint16_t* zeros, const char* who,
                         hipStream_t stream) {
  auto at = [&](size_t off) { return (uint16_t*)(A + off); };
  const size_t sl = g.slice();
  auto conv = [&](const void* in, rtv_vae_conv c, const uint16_t* res, void* out, int kt) {
    ConvParams p = make_params(in, c, out, zeros, g.F, g.H, g.W, g.C, g.C);
    p.residual = res;
    p.kt = kt;
    p.relu = 1;
    return launch_layer(p, PLAIN, stream);
  };
  for (int b = 0; b < 3; ++b) {
    uint16_t *cur = at(g.cat[b & 1]), *nxt = at(g.cat[(b + 1) & 1]), *state = at(g.state[b]);
    // [x_{t-1} | x_t] window: slice 0 = the block's input at the previous frame (carried across calls)
    if (hipMemcpyAsync(cur, state, sl * 2, hipMemcpyDeviceToDevice, stream) != hipSuccess) return fail(who, "copy failed");
    if (int st = conv(cur, mem[b][0], nullptr, at(g.tmp[0]), 2)) return st;
    if (hipMemcpyAsync(state, cur + (size_t)g.F * sl, sl * 2, hipMemcpyDeviceToDevice, stream) != hipSuccess)
      return fail(who, "copy failed");
    if (int st = conv(at(g.tmp[0]), mem[b][1], nullptr, at(g.tmp[1]), 1)) return st;
    if (int st = conv(at(g.tmp[1]), mem[b][2], cur + sl, nxt + sl, 1)) return st;
  }
  return 0;
}

// The start of a decode / encode call: the zero page, and on a stream's first call the state
static int zero_fill(char* A, const Layout& L, int first, const char* who, hipStream_t stream) {
  if (hipMemsetAsync(A + L.zeros, 0, 256, stream) != hipSuccess) return fail(who, "memset failed");
  if (first && hipMemsetAsync(A, 0, L.state_bytes, stream) != hipSuccess) return fail(who, "memset failed");
  return 0;
}


// ================================================================ encoder (the `encoder` of demo_utils/taehv.py:172-178)
// conv 3 -> 64 + ReLU at full resolution; TPool(64, 2) folded into the stride-2 conv behind it (both linear and bias-free,
// TPool(0) = 0 keeps the conv's zero padding: one stride-2 conv with two time taps over the frame pair 2j, 2j + 1); three
// MemBlocks at H/2 and half the frame rate; the same again to H/4 and a quarter of the frame rate; TPool(64, 1) folded into
// a plain stride-2 conv to H/8; three MemBlocks; conv 64 -> 16 + bias written as planar f16 latents.  The MemBlock convs are
// the decoder's Cout = 64 forms above.  A call holds a multiple of 4 frames, so no TPool pair straddles two calls and the
// carried state is the nine MemBlock inputs of the previous frame only.

struct FirstParams {
  const uint16_t* frames;   // f16 planar [3][T_total][H][W] in [-1, 1]
  const uint16_t* w;        // [64][32]: tap c * 9 + dy * 3 + dx, taps 27..31 zero
  const uint16_t* bias;     // [64]
  uint16_t* out;            // f16 channels-last [T][H][W][64]
  int T_total, t0, T, H, W, M;
};

// Encoder layer 0: conv 3 -> 64 + bias, ReLU on TAEHV's [0, 1] pixels (0.5 * x + 0.5 of the wrapper's [-1, 1] frames, applied
// to in-image taps only so that the zero padding stays zero in [0, 1] space).  One wave = 32 pixels x 64 filters: each lane
// gathers 16 of its pixel's 27 (padded to 32) taps straight from the planar frames (2-byte loads, consecutive lanes =
// consecutive pixels), four 32x32x16 f16 MFMAs against the register-resident [64][32] weight, then bias + ReLU and a
// half-wave exchange (v_permlane32_swap) so that every lane stores 16 contiguous bytes: 4 global_store_dwordx4 per lane,
// the 128 contiguous bytes of a pixel written by its two lanes.
// Bound by its output: 128 B written per pixel (51 MB per 480 x 832 frame) against 6 B read and 4 MFMAs per 32 pixels.
__global__ __launch_bounds__(256) void taehv_enc_first_kernel(FirstParams p) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, g = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = (blockIdx.x * 4 + wave) * 32 + l31;
  const int mc = min(m, p.M - 1);   // clamped pixels compute in bounds and are not stored
  const int HW = p.H * p.W;
  const int t = mc / HW, rem = mc - t * HW;
  const int y = rem / p.W, x = rem - y * p.W;
  int f = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (y + k - 1 >= 0 && y + k - 1 < p.H) f |= 1 << k;
    if (x + k - 1 >= 0 && x + k - 1 < p.W) f |= 8 << k;
  }
  const uint16_t* src = p.frames + (size_t)(p.t0 + t) * HW + rem;
  const int plane = p.T_total * HW;
  // MFMA K slot ks * 16 + g * 8 + i = tap index; the two half-waves hold different taps of the same pixel
  u32x4 bfrag[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k0 = ks * 16 + i, k1 = k0 + 8;
      const int off0 = k0 < 27 ? (k0 / 9) * plane + ((k0 % 9) / 3 - 1) * p.W + (k0 % 3 - 1) : 0;
      const int off1 = k1 < 27 ? (k1 / 9) * plane + ((k1 % 9) / 3 - 1) * p.W + (k1 % 3 - 1) : 0;
      const int mask0 = k0 < 27 ? (1 << ((k0 % 9) / 3)) | (8 << (k0 % 3)) : 64;   // bit 6 is never set: a padding tap
      const int mask1 = k1 < 27 ? (1 << ((k1 % 9) / 3)) | (8 << (k1 % 3)) : 64;
      const int mask = g ? mask1 : mask0;
      const bool ok = (f & mask) == mask;
      const int off = ok ? (g ? off1 : off0) : 0;
      const float px = f16_to_f32(src[off]);
      v[i] = ok ? 0.5f * px + 0.5f : 0.f;
    }
    bfrag[ks] = u32x4{pack_f16x2(v[0], v[1]), pack_f16x2(v[2], v[3]), pack_f16x2(v[4], v[5]), pack_f16x2(v[6], v[7])};
  }
  f32x16 acc[2];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const u32x4 wf = *(const u32x4*)(p.w + (nb * 32 + l31) * 32 + ks * 16 + g * 8);
      acc[nb] = Mfma32<true>::run(wf, bfrag[ks], acc[nb]);
    }
  }
  // acc[nb][rq * 4 + i] = filter nb * 32 + rq * 8 + g * 4 + i of pixel l31
  uint16_t* dst = p.out + (size_t)mc * 64 + g * 8;
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int rq = 0; rq < 4; rq += 2) {
      u32x2 o[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const u32x2 bb = *(const u32x2*)(p.bias + nb * 32 + (rq + q) * 8 + g * 4);
        float b0, b1, b2, b3;
        unpack_f16x2(bb[0], b0, b1);
        unpack_f16x2(bb[1], b2, b3);
        const int r = (rq + q) * 4;
        o[q][0] = pack_f16x2(fmaxf(acc[nb][r + 0] + b0, 0.f), fmaxf(acc[nb][r + 1] + b1, 0.f));
        o[q][1] = pack_f16x2(fmaxf(acc[nb][r + 2] + b2, 0.f), fmaxf(acc[nb][r + 3] + b3, 0.f));
      }
      // lanes 32-63 of quad rq <-> lanes 0-31 of quad rq + 1: the low half-wave ends up with filters 8 rq' .. 8 rq' + 7 of its
      // pixel (rq' = rq), the high one with the next eight
      const auto s0 = __builtin_amdgcn_permlane32_swap(o[0][0], o[1][0], false, false);
      const auto s1 = __builtin_amdgcn_permlane32_swap(o[0][1], o[1][1], false, false);
      if (m < p.M) *(u32x4*)(dst + nb * 32 + (rq >> 1) * 16) = u32x4{s0[0], s1[0], s0[1], s1[1]};
    }
}

static int launch_enc_first(FirstParams p, hipStream_t stream) {
  if (!p.frames || !p.w || !p.bias || !p.out) return set_error(-1, "taehv_enc_first: null pointer");
  if (p.T <= 0) return 0;
  if (p.H <= 0 || p.W <= 0 || p.t0 < 0 || p.t0 + p.T > p.T_total) return set_error(-1, "taehv_enc_first: bad size / frame range");
  if ((((uintptr_t)p.w | (uintptr_t)p.out) & 15) || ((uintptr_t)p.bias & 7) || ((uintptr_t)p.frames & 1))
    return set_error(-1, "taehv_enc_first: weights / output must be 16-byte aligned (bias 8)");
  if ((size_t)3 * p.T_total * p.H * p.W >= 0x7fffffffull || (size_t)p.T * p.H * p.W >= 0x7fffffffull / 64)
    return set_error(-1, "taehv_enc_first: input too large for 32-bit offsets");
  p.M = p.T * p.H * p.W;
  ProfScope prof(PROF_CONV, stream, 2.0 * p.M * 64.0 * 27);
  hipLaunchKernelGGL(taehv_enc_first_kernel, dim3((p.M + 127) / 128), dim3(256), 0, stream, p);
  return check_launch("taehv_enc_first");
}

// Encoder: three 64-channel stages at H/2 (half the frame rate), H/4 and H/8 (a quarter).  pre = two full-resolution 64-channel
// frames: layer 0 and the first folded down-conv run one frame pair at a time, so the full-resolution activations never take
// more than two frames.  No post region.
static bool make_enc_layout(int H, int W, int t_max, Layout* L) {
  if (H <= 0 || W <= 0 || H > 8192 || W > 8192 || (H & 7) || (W & 7) || t_max < 0 || t_max > 4096 || (t_max & 3)) return false;
  for (int s = 0; s < 3; ++s) L->st[s] = Stage{H >> (s + 1), W >> (s + 1), 64, s == 0 ? t_max / 2 : t_max / 4, {}, {}, {}};
  make_layout(L, (size_t)2 * H * W * 64 * 2, 0);
  return true;
}

}  // namespace tae
}  // namespace rtv

using namespace rtv;

#define TAE_TRY(expr)         \
  do {                        \
    int st_ = (expr);         \
    if (st_) return st_;      \
  } while (0)

extern "C" size_t rtv_taehv_arena_bytes(int h, int w, int t_max) {
  tae::Layout L;
  if (t_max <= 0 || !tae::make_dec_layout(h, w, t_max, &L)) return 0;
  return L.total;
}

extern "C" int rtv_taehv_state_slot(int h, int w, int slot, size_t* offset, int* C, int* H, int* W) {
  tae::Layout L;
  if (!tae::make_dec_layout(h, w, 0, &L)) return set_error(-1, "taehv: bad latent size");
  return tae::state_slot(L, "taehv", slot, offset, C, H, W);
}

extern "C" int rtv_taehv_conv(const void* in, const void* w, const void* bias, const void* residual, void* out, int T, int H,
                              int W, int Cin, int Cout, int kt, int ups, int n_split, int relu, int head, const void* zeros,
                              rtv_stream_t stream) {
  tae::ConvParams p = tae::make_params(in, {w, bias}, out, zeros, T, H, W, Cin, Cout);
  p.residual = (const uint16_t*)residual;
  p.kt = kt;
  p.ups = ups;
  p.n_split = n_split;
  p.relu = relu ? 1 : 0;
  return tae::launch_layer(p, head ? tae::RGB_HEAD : tae::PLAIN, (hipStream_t)stream);
}

// the Clamp + layout prologue of rtv_taehv_decode on its own, used by the tests
extern "C" int rtv_taehv_prep(const void* z, int T, int hw, void* out, rtv_stream_t stream) {
  if (!z || !out) return set_error(-1, "taehv_prep: null argument");
  if (T <= 0 || hw <= 0 || (int64_t)T * hw > (1 << 26)) return set_error(-1, "taehv_prep: T and hw must be positive");
  if (((uintptr_t)out) & 15) return set_error(-1, "taehv_prep: out must be 16-byte aligned");
  return tae::launch_prep(z, T, hw, out, (hipStream_t)stream);
}

extern "C" int rtv_taehv_decode(const rtv_taehv_weights* wt, const void* z, int T, int h, int w, int first, void* arena,
                                size_t arena_bytes, void* pixels, rtv_stream_t stream_) {
  if (!wt || !z || !arena || !pixels) return set_error(-1, "taehv_decode: null argument");
  if (T <= 0) return set_error(-1, "taehv_decode: T must be positive");
  if (((uintptr_t)arena) & 255) return set_error(-1, "taehv_decode: arena must be 256-byte aligned");
  tae::Layout L;
  if (!tae::make_dec_layout(h, w, T, &L)) return set_error(-1, "taehv_decode: unsupported latent size or T");
  if (arena_bytes < L.total) return set_error(-1, "taehv_decode: arena too small for T (see rtv_taehv_arena_bytes)");
  // the largest gather input (the 64-channel MemBlock concat buffers, 2T + 1 slices) must stay within 32-bit offsets
  if ((size_t)(2 * T + 1) * (4 * h) * (4 * w) * 64 >= 0x7fffffffull) return set_error(-1, "taehv_decode: T too large");
  hipStream_t stream = (hipStream_t)stream_;
  char* A = (char*)arena;
  auto at = [&](size_t off) { return (uint16_t*)(A + off); };
  const uint16_t* zeros = at(L.zeros);
  TAE_TRY(tae::zero_fill(A, L, first, "taehv_decode", stream));

  // decoder.0 (Clamp) + layout, decoder.1 / 2: conv 16 -> 256 + bias, ReLU -> slices 1..T of the first MemBlock's concat buffer
  {
    TAE_TRY(tae::launch_prep(z, T, h * w, at(L.pre), stream));
    tae::ConvParams p = tae::make_params(at(L.pre), wt->conv_in, at(L.st[0].cat[0]) + L.st[0].slice(), zeros, T, h, w, 32, 256);
    p.relu = 1;
    TAE_TRY(tae::launch_layer(p, tae::PLAIN, stream));
  }
  for (int s = 0; s < 3; ++s) {
    const tae::Stage& g = L.st[s];
    TAE_TRY(tae::run_memblocks(A, g, wt->mem + 3 * s, zeros, "taehv_decode", stream));
    if (s < 2) {   // decoder.{6,7,8} / {12,13,14}: up 2x, TGrow folded into the conv -> slices 1.. of the next stage's buffer
      const tae::Stage& n = L.st[s + 1];
      tae::ConvParams p = tae::make_params(at(g.cat[1]) + g.slice(), {wt->up[s], nullptr}, at(n.cat[0]) + n.slice(), zeros, g.F,
                                           n.H, n.W, g.C, 128);
      p.ups = 1;
      p.n_split = s == 0 ? 0 : 64;
      TAE_TRY(tae::launch_layer(p, tae::PLAIN, stream));
    }
  }
  // decoder.{18..22}: up 2x + TGrow(64, 2) folded into conv 64 -> 64, ReLU, conv 64 -> 3, one 64-channel frame j (= output frames
  // 2j, 2j + 1) at a time; on a stream's first call the output frames 0..2 are TAEHV's warm-up frames and are not produced
  {
    const tae::Stage& g = L.st[2];
    const int H = 8 * h, W = 8 * w;
    const size_t fsl = (size_t)H * W * 64;
    const int skip = first ? 3 : 0;
    for (int j = 0; j < g.F; ++j) {
      const int lo = 2 * j > skip ? 2 * j : skip;
      if (lo >= 2 * j + 2) continue;
      tae::ConvParams p = tae::make_params(at(g.cat[1]) + (size_t)(1 + j) * g.slice(), {wt->up[2], nullptr}, at(L.post), zeros, 1, H,
                                           W, 64, 128);
      p.ups = 1;
      p.n_split = 64;
      p.relu = 1;
      TAE_TRY(tae::launch_layer(p, tae::PLAIN, stream));
      p = tae::make_params(at(L.post) + (size_t)(lo - 2 * j) * fsl, wt->head, (float*)pixels + (size_t)(lo - skip) * 3 * H * W, zeros,
                           2 * j + 2 - lo, H, W, 64, 8);
      TAE_TRY(tae::launch_layer(p, tae::RGB_HEAD, stream));
    }
  }
  return 0;
}

// ---------------------------------------------------------------- encoder C ABI
extern "C" size_t rtv_taehv_enc_arena_bytes(int H, int W, int t_max) {
  tae::Layout L;
  if (t_max <= 0 || !tae::make_enc_layout(H, W, t_max, &L)) return 0;
  return L.total;
}

extern "C" int rtv_taehv_enc_state_slot(int H, int W, int slot, size_t* offset, int* C, int* h, int* w) {
  tae::Layout L;
  if (!tae::make_enc_layout(H, W, 0, &L)) return set_error(-1, "taehv_enc: frame size must be positive multiples of 8");
  return tae::state_slot(L, "taehv_enc", slot, offset, C, h, w);
}

extern "C" int rtv_taehv_enc_conv(const void* in, const void* w, const void* bias, void* out, int form, int T, int H, int W,
                                  int kt, int n_total, int n0, const void* zeros, rtv_stream_t stream) {
  if (form == 0) {
    const tae::FirstParams f{(const uint16_t*)in, (const uint16_t*)w, (const uint16_t*)bias, (uint16_t*)out, n_total, n0, T, H, W, 0};
    return tae::launch_enc_first(f, (hipStream_t)stream);
  }
  if (form != 1 && form != 2) return set_error(-1, "taehv_enc_conv: form must be 0 (first), 1 (stride 2) or 2 (head)");
  tae::ConvParams p = tae::make_params(in, {w, bias}, out, zeros, T, H, W, 64, form == 2 ? 16 : 64);
  p.kt = kt;
  p.out_T = n_total;
  p.out_j = n0;
  return tae::launch_layer(p, form == 2 ? tae::LATENT_HEAD : tae::DOWN, (hipStream_t)stream);
}

extern "C" int rtv_taehv_encode(const rtv_taehv_enc_weights* wt, const void* frames, int T_total, int t0, int tn, int H, int W,
                                int first, void* arena, size_t arena_bytes, void* latents, int T_out, int j,
                                rtv_stream_t stream_) {
  if (!wt || !frames || !arena || !latents) return set_error(-1, "taehv_encode: null argument");
  if (tn <= 0 || (tn & 3)) return set_error(-1, "taehv_encode: tn must be a positive multiple of 4");
  if (t0 < 0 || t0 + tn > T_total) return set_error(-1, "taehv_encode: frames t0 .. t0 + tn outside the clip");
  if (j < 0 || j + tn / 4 > T_out) return set_error(-1, "taehv_encode: latent frames outside the output tensor");
  if (((uintptr_t)arena) & 255) return set_error(-1, "taehv_encode: arena must be 256-byte aligned");
  tae::Layout L;
  if (!tae::make_enc_layout(H, W, tn, &L)) return set_error(-1, "taehv_encode: H and W must be multiples of 8 (or tn too large)");
  if (arena_bytes < L.total) return set_error(-1, "taehv_encode: arena too small for tn (see rtv_taehv_enc_arena_bytes)");
  hipStream_t stream = (hipStream_t)stream_;
  char* A = (char*)arena;
  auto at = [&](size_t off) { return (uint16_t*)(A + off); };
  const uint16_t* zeros = at(L.zeros);
  TAE_TRY(tae::zero_fill(A, L, first, "taehv_encode", stream));
  // a folded TPool + stride-2 conv onto the output grid (Hh, Ww); kt = the TPool's time stride
  auto down = [&](const void* in, const void* wts, void* out, int Tn, int Hh, int Ww, int kt) {
    tae::ConvParams p = tae::make_params(in, {wts, nullptr}, out, zeros, Tn, Hh, Ww, 64, 64);
    p.kt = kt;
    return tae::launch_layer(p, tae::DOWN, stream);
  };

  // encoder.{0..3}: conv 3 -> 64 + ReLU on a frame pair, then TPool(64, 2) + stride-2 conv as one layer -> slice 1 + q of the
  // first MemBlock's concat buffer at H/2
  for (int q = 0; q < tn / 2; ++q) {
    const tae::FirstParams f{(const uint16_t*)frames, (const uint16_t*)wt->conv_in.w, (const uint16_t*)wt->conv_in.b, at(L.pre),
                             T_total, t0 + 2 * q, 2, H, W, 0};
    TAE_TRY(tae::launch_enc_first(f, stream));
    TAE_TRY(down(at(L.pre), wt->down[0], at(L.st[0].cat[0]) + (size_t)(1 + q) * L.st[0].slice(), 1, H / 2, W / 2, 2));
  }
  for (int s = 0; s < 3; ++s) {
    const tae::Stage& g = L.st[s];
    TAE_TRY(tae::run_memblocks(A, g, wt->mem + 3 * s, zeros, "taehv_encode", stream));
    if (s < 2) {   // encoder.{7,8}: TPool(64, 2) + stride-2 conv; encoder.{12,13}: TPool(64, 1) + stride-2 conv
      const tae::Stage& n = L.st[s + 1];
      TAE_TRY(down(at(g.cat[1]) + g.slice(), wt->down[s + 1], at(n.cat[0]) + n.slice(), n.F, n.H, n.W, s == 0 ? 2 : 1));
    }
  }
  // encoder.17: conv 64 -> 16 + bias -> latent frames j .. j + tn / 4 of the planar output
  {
    const tae::Stage& g = L.st[2];
    tae::ConvParams p = tae::make_params(at(g.cat[1]) + g.slice(), wt->head, latents, zeros, g.F, g.H, g.W, 64, 16);
    p.out_T = T_out;
    p.out_j = j;
    TAE_TRY(tae::launch_layer(p, tae::LATENT_HEAD, stream));
  }
  return 0;
}
