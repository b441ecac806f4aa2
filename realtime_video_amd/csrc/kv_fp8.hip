// The e4m3-only KV cache of fp8 self-attention (include/rtv_hip_attn_fp8_only.h, rtv_hip_attn_fp8_only_center.h): the two kernels
// that write a block's K and V rows straight into k8 / v8t, with no bf16 cache row in between.
//
//   qk_norm_rope_k8_kernel<CPL, CENTER>  qk_norm_rope_cache_kernel (elementwise.hip) with the k role storing e4m3 codes: the same
//                              canonical sum of squares, the same roundings, the same RoPE, the same ring mapping; the rotated chunk
//                              is packed to bf16 as the cache write packs it, unpacked, and quantised as attn_quantize_kv_kernel
//                              (attn_fp8.hip) quantises the cache row - so the codes are those of the shadow mode.  No V role.
//                              CENTER codes k - c (K smoothing on the compact cache).  The row body restates that of the bf16 kernel
//                              on purpose: carved into shared device functions it changed the instruction streams of the bf16
//                              kernel, which the default path runs (profiles/r26_kv_fp8_fold_isa.txt).
//   attn_quantize_v_rows_kernel  the V half of attn_quantize_kv_kernel reading a staging matrix (the V third of the projection
//                              buffer) instead of the cache: one workgroup per (storage tile, head), whole tiles leave LDS as
//                              16-byte pieces, partly covered tiles as words and bytes of their own rows only.
// Both are read-once / write-once row kernels (yardstick: the 4.7 TB/s copy rate noted in elementwise.hip).
#include <cmath>

#include "../../include/rtv_hip_attn_fp8_only.h"
#include "../../include/rtv_hip_attn_fp8_only_center.h"
#include "attn_common.h"
#include "fp8_quant.h"
#include "ln_row.h"
#include "rope_row.h"
#include "rtv_common.h"
#include "rtv_internal.h"

namespace rtv {

struct RopeK8Args {
  const bf16_t* qkv;
  bf16_t* q_out;     // null: no q role (the kv_only pass)
  uint8_t* k8;
  unsigned* amax;    // null: no running maximum
  const float* center;   // CENTER only: [H][128] fp32 = [d] in the row's column order
  float k_scale;
  int cache_row0;
  int M, d, hd;
  float eps;
  const bf16_t* wq;
  const bf16_t* wk;
  const float2* rope_cs;  // [1024][hd/2]
  int gh, gw, start_frame, row_offset;
  int ring_lo, ring_size, ring_shift;
};

// Two waves per row as in qk_norm_rope_cache_kernel: one normalises and rotates q, the other k (one wave per row without q).
// A wave behind the last row does nothing but reach the barrier of the workgroup's maximum.  The head dimension is 128, so a lane's
// four (cos, sin) pairs are the same for all of its chunks (the LANE_CS form of qk_norm_rope_cache_kernel).
// CENTER: the centre is read at the point of use - two 16-byte loads per chunk, L2-resident, 20 KB at 14B width - and never held
// across the row.
template <int CPL, bool CENTER>
__global__ __launch_bounds__(EW_THREADS) __attribute__((amdgpu_waves_per_eu(CPL <= 10 ? 5 : 3, 8))) void qk_norm_rope_k8_kernel(RopeK8Args a) {
  __shared__ float s_max[EW_THREADS / 64];
  const int lane = threadIdx.x & 63;
  const int nroles = a.q_out != nullptr ? 2 : 1;   // kernel-uniform
  const int wid = __builtin_amdgcn_readfirstlane(blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6));
  const int row = wid / nroles;
  const bool is_k = wid - row * nroles == nroles - 1;   // wave-uniform
  float kmax = 0.f;
  if (row < a.M) {
    const int d = a.d;
    const int nchunks = d >> 3;
    const bf16_t* xr = a.qkv + (size_t)row * 3 * d + (is_k ? d : 0);
    const bf16_t* wx = is_k ? a.wk : a.wq;

    // positions of this token (wave-uniform) and the (cos, sin) pairs of this lane's columns
    const int half = a.hd >> 1;
    const int c1 = half / 3, c0 = half - 2 * c1;
    const int per_frame = a.gh * a.gw;
    const int grow = a.row_offset + row;  // global token index
    const int f = grow / per_frame;
    const int rem = grow - f * per_frame;
    const int pos_h = rem / a.gw, pos_w = rem - pos_h * a.gw;
    const int pos_f = a.start_frame + f;
    auto load_cs = [&](int col, float2* w) {
      const int pj0 = (col % a.hd) >> 1;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int pj = pj0 + t;
        const int pos = pj < c0 ? pos_f : (pj < c0 + c1 ? pos_h : pos_w);
        w[t] = a.rope_cs[pos * half + pj];
      }
    };
    float2 cs[4];
    load_cs(lane * 8, cs);

    int kv_row = a.cache_row0 + grow;
    if (a.ring_size > 0 && kv_row >= a.ring_lo) kv_row = a.ring_lo + (kv_row - a.ring_lo + a.ring_shift) % a.ring_size;
    bf16_t* const qo = a.q_out + (size_t)row * d;
    uint8_t* const ko = a.k8 + (size_t)kv_row * d;

    u32x4 raw[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int c = lane + i * 64;
      if (c < nchunks) raw[i] = *(const u32x4*)(xr + c * 8);
    }
    // the canonical order of qk_norm_rope_cache_kernel: four accumulators per lane column, ((0 + 1) + 2) + 3, the 64-lane butterfly
    float acc4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      if (lane + i * 64 < nchunks) {
        float t[8];
        unpack_bf16x8(raw[i], t);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc4[i & 3] = __builtin_fmaf(t[j], t[j], acc4[i & 3]);
      }
    }
    const float sx = ((acc4[0] + acc4[1]) + acc4[2]) + acc4[3];
    const float rx = rsqrtf(wave_sum(sx) / (float)d + a.eps);
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < CPL; ++i) launder(raw[i]);
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int c = lane + i * 64;
      if (c < nchunks) {
        float w8[8], x[8];
        unpack_bf16x8(*(const u32x4*)(wx + c * 8), w8);
        unpack_bf16x8(raw[i], x);
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = round_bf16(round_bf16(x[j] * rx) * w8[j]);
        rope8(x, cs);
        const u32x4 packed = pack_bf16x8(x);   // the rounding of the cache write
        if (!is_k) {
          *(u32x4*)(qo + c * 8) = packed;
        } else {
          unpack_bf16x8(packed, x);            // ... and what the quantiser would read back from the cache
          if constexpr (CENTER) {
            const f32x4 ce0 = *(const f32x4*)(a.center + c * 8), ce1 = *(const f32x4*)(a.center + c * 8 + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] -= ce0[j], x[4 + j] -= ce1[j];   // fp32, rounded once, before the division
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) kmax = fmaxf(kmax, fabsf(x[j]));
          *(u32x2*)(ko + c * 8) = quantize8(x, a.k_scale);
        }
      }
    }
  }
  if (a.amax == nullptr) return;   // kernel-uniform
  block_max_stage(kmax, s_max);
  __syncthreads();
  if (threadIdx.x == 0) block_max_commit(s_max, a.amax);
}

struct QuantVArgs {
  const uint16_t* v;   // source row 0
  int64_t rs;
  int row0, rows, H, tile0;   // destination rows [row0, row0 + rows); tile0 = row0 >> 6
  uint8_t* v8t;
  float v_scale;
  unsigned* amax;      // float[2]; [1] is V's
};

// One workgroup = one (storage tile, head), thread (kq, dc) = keys 4 kq .. 4 kq + 3 of the tile, dims 8 dc .. 8 dc + 7: the thread
// layout, the LDS image and the partial-tile rule of attn_quantize_kv_kernel.  Physical row p reads source row p - row0.
__global__ __launch_bounds__(256) void attn_quantize_v_rows_kernel(QuantVArgs p) {
  constexpr int LD = 17;   // words per dim row of the LDS image (16 + 1: the dims of a wave do not all start in one bank)
  __shared__ __attribute__((aligned(16))) uint32_t sV[ATT_D * LD];
  __shared__ float s_max[4];
  const int tid = threadIdx.x;
  const int T = p.tile0 + blockIdx.x, h = blockIdx.y;
  const int dc = tid & 15, kq = tid >> 4;
  const int r_lo = max(p.row0 - T * ATT_KT, 0), r_hi = min(p.row0 + p.rows - T * ATT_KT, ATT_KT);   // tile-local rows to convert
  float vmax = 0.f;
  uint32_t vw[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int key = 4 * kq + jj;
    if (key < r_lo || key >= r_hi) continue;
    const int64_t src_row = (int64_t)T * ATT_KT + key - p.row0;   // in [0, rows)
    const u32x4 vr = *(const u32x4*)(p.v + (size_t)(src_row * p.rs) + (size_t)h * ATT_D + dc * 8);
    float x[8];
    unpack_bf16x8(vr, x);
#pragma unroll
    for (int d = 0; d < 8; ++d) vmax = fmaxf(vmax, fabsf(x[d]));
    const u32x2 cv = quantize8(x, p.v_scale);
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const uint32_t w = d < 4 ? cv[0] : cv[1];
      vw[d] |= ((w >> (8 * (d & 3))) & 0xffu) << (8 * jj);
    }
  }
  // keys 4 kq .. + 3 = (kb, i, g) = (kq >> 3, (kq >> 1) & 3, kq & 1), j = 0..3  ->  slots 32 g + 16 kb + 4 i + j = word 8 g + 4 kb + i
  const int word = 8 * (kq & 1) + 4 * (kq >> 3) + ((kq >> 1) & 3);
#pragma unroll
  for (int d = 0; d < 8; ++d) sV[(dc * 8 + d) * LD + word] = vw[d];
  if (p.amax != nullptr) {
    vmax = wave_max(vmax);
    if ((tid & 63) == 0) s_max[tid >> 6] = vmax;
  }
  __syncthreads();
  if (p.amax != nullptr && tid == 0) {
    const unsigned bits = __float_as_uint(fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3])));
    if (bits > __atomic_load_n(p.amax + 1, __ATOMIC_RELAXED)) atomicMax(p.amax + 1, bits);
  }
  uint8_t* const tile = p.v8t + ((size_t)T * p.H + h) * (ATT_KT * ATT_D);
  const bool whole = r_lo == 0 && r_hi == ATT_KT;   // workgroup-uniform
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int id = tid + it * 256, dim = id >> 2, c = id & 3;
    uint32_t w4[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) w4[w] = sV[dim * LD + 4 * c + w];
    uint8_t* const dst = tile + dim * ATT_KT + c * 16;
    if (whole) {
      *(u32x4*)dst = u32x4{w4[0], w4[1], w4[2], w4[3]};
    } else {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int W = 4 * c + w;                                           // slots 4 W .. 4 W + 3
        const int key0 = 32 * ((W >> 2) & 1) + 8 * (W & 3) + 4 * (W >> 3);   // = keys key0 .. key0 + 3
        if (key0 >= r_lo && key0 + 4 <= r_hi) {
          *(uint32_t*)(dst + 4 * w) = w4[w];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (key0 + j >= r_lo && key0 + j < r_hi) dst[4 * w + j] = (uint8_t)(w4[w] >> (8 * j));
        }
      }
    }
  }
}

}  // namespace rtv

using namespace rtv;

// The checks and the launch of both e4m3 K writers; center != null selects the CENTER instantiation.
static int qk_norm_rope_k8_launch(const char* who, const void* qkv, void* q_out, void* k8, int cache_rows, float k_scale, void* amax,
                                  int cache_row0, int M, int d, int num_heads, float eps, const void* wq, const void* wk,
                                  const void* rope_cs, int F, int gh, int gw, int start_frame, int row_offset, int ring_lo,
                                  int ring_size, int ring_shift, const float* center, rtv_stream_t stream) {
  if (M <= 0) return 0;
  if (qk_norm_rope_check(d, cache_row0, M, d, num_heads, F, gh, gw, start_frame, row_offset, 0, 0, 0, ring_lo, ring_size, ring_shift,
                         q_out ? 3 : 2))
    return -1;
  if (d / num_heads != ATT_D) return set_error(-1, "qk_norm_rope_k8: head_dim must be 128");
  if (!qkv || !k8 || !wq || !wk || !rope_cs) return set_error(-1, "qk_norm_rope_k8: null pointer");
  if (((uintptr_t)qkv | (uintptr_t)q_out | (uintptr_t)k8 | (uintptr_t)wq | (uintptr_t)wk) & 15)
    return set_error(-1, "qk_norm_rope_k8: qkv, q_out, k8, wq and wk must be 16-byte aligned");
  if (((uintptr_t)rope_cs & 7) || ((uintptr_t)amax & 3)) return set_error(-1, "qk_norm_rope_k8: rope_cs must be 8-byte, amax 4-byte aligned");
  if (cache_rows <= 0) return set_error(-1, "qk_norm_rope_k8: cache_rows must be positive");
  // the largest physical row: without a ring the last logical row; with one, rows at or above ring_lo stay below ring_lo + ring_size
  const int64_t end = ring_size > 0 ? (int64_t)ring_lo + ring_size : (int64_t)cache_row0 + row_offset + M;
  if (end > cache_rows) return set_error(-1, "qk_norm_rope_k8: row range outside [0, cache_rows)");
  if (!good_scale(k_scale)) return set_error(-1, "qk_norm_rope_k8: k_scale must be finite and positive");
  RopeK8Args a;
  a.qkv = (const bf16_t*)qkv;
  a.q_out = (bf16_t*)q_out;
  a.k8 = (uint8_t*)k8;
  a.amax = (unsigned*)amax;
  a.k_scale = k_scale;
  a.cache_row0 = cache_row0;
  a.M = M;
  a.d = d;
  a.hd = ATT_D;
  a.eps = eps;
  a.wq = (const bf16_t*)wq;
  a.wk = (const bf16_t*)wk;
  a.rope_cs = (const float2*)rope_cs;
  a.gh = gh;
  a.gw = gw;
  a.start_frame = start_frame;
  a.row_offset = row_offset;
  a.ring_lo = ring_lo;
  a.ring_size = ring_size;
  a.ring_shift = ring_shift;
  a.center = center;
  // bytes: q read + written as bf16, k read as bf16 and written as codes (the centre stays in L2)
  ProfScope prof(PROF_ROPE, (hipStream_t)stream, ((q_out ? 4.0 : 0.0) + 3.0) * M * d);
  const int waves = M * (q_out ? 2 : 1);
  const dim3 grid((waves + ROWS_PER_WG - 1) / ROWS_PER_WG);
#define RTV_ROPE_K8_CALL(CPL)                                                                                        \
  if (center) hipLaunchKernelGGL((qk_norm_rope_k8_kernel<CPL, true>), grid, dim3(EW_THREADS), 0, (hipStream_t)stream, a); \
  else hipLaunchKernelGGL((qk_norm_rope_k8_kernel<CPL, false>), grid, dim3(EW_THREADS), 0, (hipStream_t)stream, a)
  RTV_ROW_DISPATCH(d, RTV_ROPE_K8_CALL);
#undef RTV_ROPE_K8_CALL
  return check_launch(who);
}

extern "C" int rtv_qk_norm_rope_k8(const void* qkv, void* q_out, void* k8, int cache_rows, float k_scale, void* amax, int cache_row0,
                                   int M, int d, int num_heads, float eps, const void* wq, const void* wk, const void* rope_cs, int F,
                                   int gh, int gw, int start_frame, int row_offset, int ring_lo, int ring_size, int ring_shift,
                                   rtv_stream_t stream) {
  return qk_norm_rope_k8_launch("qk_norm_rope_k8", qkv, q_out, k8, cache_rows, k_scale, amax, cache_row0, M, d, num_heads, eps, wq, wk,
                                rope_cs, F, gh, gw, start_frame, row_offset, ring_lo, ring_size, ring_shift, nullptr, stream);
}

extern "C" int rtv_qk_norm_rope_k8_centered(const void* qkv, void* q_out, void* k8, int cache_rows, float k_scale, void* amax,
                                            int cache_row0, int M, int d, int num_heads, float eps, const void* wq, const void* wk,
                                            const void* rope_cs, int F, int gh, int gw, int start_frame, int row_offset, int ring_lo,
                                            int ring_size, int ring_shift, const float* center, rtv_stream_t stream) {
  if (!center || ((uintptr_t)center & 15))
    return set_error(-1, "qk_norm_rope_k8: center must be a 16-byte aligned device float[H][128]");
  return qk_norm_rope_k8_launch("qk_norm_rope_k8_centered", qkv, q_out, k8, cache_rows, k_scale, amax, cache_row0, M, d, num_heads, eps,
                                wq, wk, rope_cs, F, gh, gw, start_frame, row_offset, ring_lo, ring_size, ring_shift, center, stream);
}

extern "C" int rtv_attn_quantize_v_rows(const void* v_src, int64_t src_row_stride, int rows, int H, void* v8t, int cache_rows,
                                        int dst_row0, float v_scale, void* amax, rtv_stream_t stream) {
  if (!v_src || !v8t) return set_error(-1, "attn_quantize_v_rows: null pointer");
  if (((uintptr_t)v_src | (uintptr_t)v8t) & 15) return set_error(-1, "attn_quantize_v_rows: v_src and v8t must be 16-byte aligned");
  if ((uintptr_t)amax & 3) return set_error(-1, "attn_quantize_v_rows: amax must be 4-byte aligned");
  if (rows <= 0 || H <= 0 || cache_rows <= 0) return set_error(-1, "attn_quantize_v_rows: rows, H and cache_rows must be positive");
  if (dst_row0 < 0 || (int64_t)dst_row0 + rows > cache_rows) return set_error(-1, "attn_quantize_v_rows: row range outside [0, cache_rows)");
  if (src_row_stride < (int64_t)H * ATT_D || (src_row_stride & 7))
    return set_error(-1, "attn_quantize_v_rows: row stride must be a multiple of 8 elements and hold H heads");
  if (!good_scale(v_scale)) return set_error(-1, "attn_quantize_v_rows: scale must be finite and positive");
  if (H > 65535) return set_error(-1, "attn_quantize_v_rows: more than 65535 heads");
  QuantVArgs p;
  p.v = (const uint16_t*)v_src;
  p.rs = src_row_stride;
  p.row0 = dst_row0;
  p.rows = rows;
  p.H = H;
  p.tile0 = dst_row0 >> 6;
  p.v8t = (uint8_t*)v8t;
  p.v_scale = v_scale;
  p.amax = (unsigned*)amax;
  const int tiles = ((dst_row0 + rows - 1) >> 6) - p.tile0 + 1;
  ProfScope prof(PROF_MISC, (hipStream_t)stream, 3.0 * rows * H * ATT_D);
  hipLaunchKernelGGL(attn_quantize_v_rows_kernel, dim3(tiles, H), dim3(256), 0, (hipStream_t)stream, p);
  return check_launch("attn_quantize_v_rows");
}
