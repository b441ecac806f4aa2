// K smoothing on the e4m3-only KV cache (include/rtv_hip_attn_fp8_only_center.h): the three kernels that keep a compact cache under
// a centre without a bf16 K row to go back to.
//
//   qk_norm_rope_k8_centered_kernel  qk_norm_rope_k8_kernel (kv_fp8.hip) with the k role coding k - c: the row body is restated here,
//                              not shared, so that the instantiations of kv_fp8.hip stay byte for byte what they were (the r06 table:
//                              a new instantiation in a hot translation unit moved its neighbours).  The centre is read at the point
//                              of use - two 16-byte loads per chunk, L2-resident, 20 KB at 14B width - and never held across the row.
//   attn_k8_center_*_kernel    attn_kv_center_*_kernel (attn_fp8.hip) reading codes: the same chunks, the same order of additions.
//   attn_k8_recenter_kernel    a read-once / write-once byte kernel: 16-byte pieces, the thread's 16 deltas in registers over the rows
//                              it walks (yardstick: the 4.7 TB/s copy rate noted in elementwise.hip).
#include <cmath>

#include "../../include/rtv_hip_attn_fp8_only_center.h"
#include "attn_common.h"
#include "fp8_quant.h"
#include "ln_row.h"
#include "rope_row.h"
#include "rtv_common.h"
#include "rtv_internal.h"

namespace rtv {

struct RopeK8CenteredArgs {
  const bf16_t* qkv;
  bf16_t* q_out;     // null: no q role (the kv_only pass)
  uint8_t* k8;
  unsigned* amax;    // null: no running maximum
  const float* center;   // [H][128] fp32 = [d] in the row's column order
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

// The roles, the canonical sum of squares, the roundings and the ring mapping of qk_norm_rope_k8_kernel, statement for statement;
// the only difference is the subtraction in front of quantize8.
template <int CPL>
__global__ __launch_bounds__(EW_THREADS) __attribute__((amdgpu_waves_per_eu(CPL <= 10 ? 5 : 3, 8))) void qk_norm_rope_k8_centered_kernel(RopeK8CenteredArgs a) {
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
          unpack_bf16x8(packed, x);            // what the centred quantiser would read back from the cache
          const f32x4 ce0 = *(const f32x4*)(a.center + c * 8), ce1 = *(const f32x4*)(a.center + c * 8 + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) x[j] -= ce0[j], x[4 + j] -= ce1[j];   // fp32, rounded once, before the division
#pragma unroll
          for (int j = 0; j < 8; ++j) kmax = fmaxf(kmax, fabsf(x[j]));
          *(u32x2*)(ko + c * 8) = quantize8(x, a.k_scale);
        }
      }
    }
  }
  if (a.amax == nullptr) return;   // kernel-uniform
  kmax = wave_max(kmax);
  if (lane == 0) s_max[threadIdx.x >> 6] = kmax;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned bits = __float_as_uint(fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3])));
    if (bits > __atomic_load_n(a.amax, __ATOMIC_RELAXED)) atomicMax(a.amax, bits);
  }
}

// 16 e4m3 codes -> 16 floats (v_cvt_pk_f32_fp8: exact; 0x7F / 0xFF give NaN)
__device__ __forceinline__ void decode16(const u32x4& w, float* x) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    x[4 * i] = lo[0], x[4 * i + 1] = lo[1], x[4 * i + 2] = hi[0], x[4 * i + 3] = hi[1];
  }
}

struct K8CenterParams {
  const uint8_t* k8;
  int row0, n0, row1, n1, H;
  float k_scale;
  const float* c_old;   // [H][128] fp32
  float* part;          // [chunks][H][128] fp32
  float* center;        // [H][128] fp32
  int chunks;
};

// Stage 1 of attn_kv_center_partial_kernel on codes.  One workgroup = one (chunk of RTV_ATTN_CENTER_CHUNK window rows, head): thread
// (rq, dc) adds the rows rq, rq + 32, ... of the chunk, dims 16 dc .. 16 dc + 15 (a 16-byte piece of the row), in ascending order;
// the 32 row groups are then added in ascending order through LDS.
__global__ __launch_bounds__(256) void attn_k8_center_partial_kernel(K8CenterParams p) {
  __shared__ float sP[32][ATT_D + 4];
  const int tid = threadIdx.x, dc = tid & 7, rq = tid >> 3, h = blockIdx.y;
  const int n = p.n0 + p.n1;
  const int j0 = blockIdx.x * RTV_ATTN_CENTER_CHUNK, j1 = min(j0 + RTV_ATTN_CENTER_CHUNK, n);
  float acc[16];
#pragma unroll
  for (int d = 0; d < 16; ++d) acc[d] = 0.f;
  for (int j = j0 + rq; j < j1; j += 32) {
    const int64_t phys = j < p.n0 ? (int64_t)p.row0 + j : (int64_t)p.row1 + (j - p.n0);
    const u32x4 w = *(const u32x4*)(p.k8 + ((size_t)phys * p.H + h) * ATT_D + dc * 16);
    float x[16];
    decode16(w, x);
#pragma unroll
    for (int d = 0; d < 16; ++d) acc[d] = __fadd_rn(acc[d], __fmul_rn(x[d], p.k_scale));   // the dequantised key, then the sum
  }
#pragma unroll
  for (int d = 0; d < 16; ++d) sP[rq][dc * 16 + d] = acc[d];
  __syncthreads();
  if (tid < ATT_D) {
    float s = sP[0][tid];
#pragma unroll
    for (int r = 1; r < 32; ++r) s += sP[r][tid];
    p.part[((size_t)blockIdx.x * p.H + h) * ATT_D + tid] = s;
  }
}

// Stage 2: the chunks in ascending order, one division, then the centre the codes stand under.
__global__ __launch_bounds__(ATT_D) void attn_k8_center_reduce_kernel(K8CenterParams p) {
  const int d = threadIdx.x, h = blockIdx.x;
  float s = 0.f;
  for (int c = 0; c < p.chunks; ++c) s += p.part[((size_t)c * p.H + h) * ATT_D + d];
  const size_t i = (size_t)h * ATT_D + d;
  p.center[i] = __fadd_rn(p.c_old[i], s / (float)(p.n0 + p.n1));
}

struct K8RecenterParams {
  uint8_t* k8;
  int row0, rows, H;
  float k_scale;
  const float* c_old;
  const float* c_new;
  unsigned* amax;
};

constexpr int RECENTER_ROWS = 256;   // rows one workgroup walks: 8 per thread

// One workgroup = RECENTER_ROWS rows of one head; thread (rq, dc) owns the 16 channels 16 dc .. 16 dc + 15 and the rows rq, rq + 32, ...
// of the workgroup's range: a quarter wave reads and writes one head's 128 bytes of a row.  Read and write of a byte are the same
// thread's, so the kernel works in place.
__global__ __launch_bounds__(256) void attn_k8_recenter_kernel(K8RecenterParams p) {
  __shared__ float s_max[4];
  const int tid = threadIdx.x, dc = tid & 7, rq = tid >> 3, h = blockIdx.y;
  float delta[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const size_t o = (size_t)h * ATT_D + dc * 16 + 4 * i;
    const f32x4 co = *(const f32x4*)(p.c_old + o), cn = *(const f32x4*)(p.c_new + o);
#pragma unroll
    for (int j = 0; j < 4; ++j) delta[4 * i + j] = __fsub_rn(co[j], cn[j]);
  }
  const int j0 = blockIdx.x * RECENTER_ROWS, j1 = min(j0 + RECENTER_ROWS, p.rows);
  float kmax = 0.f;
  for (int j = j0 + rq; j < j1; j += 32) {
    uint8_t* const at = p.k8 + ((size_t)(p.row0 + j) * p.H + h) * ATT_D + dc * 16;
    const u32x4 w = *(const u32x4*)at;
    float t[16];
    decode16(w, t);
#pragma unroll
    for (int d = 0; d < 16; ++d) {
      t[d] = __fadd_rn(__fmul_rn(t[d], p.k_scale), delta[d]);   // two roundings: never an fma
      kmax = fmaxf(kmax, fabsf(t[d]));                          // (fmaxf drops a NaN)
    }
    const u32x2 a = quantize8(t, p.k_scale), b = quantize8(t + 8, p.k_scale);
    u32x4 out = u32x4{a[0], a[1], b[0], b[1]};
    // a NaN code keeps its byte (quantize8's clamp would turn the NaN into -448)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t m7 = w[i] & 0x7f7f7f7fu;
      uint32_t nan = (m7 + 0x01010101u) & 0x80808080u;   // bit 7 of a byte set iff its low seven bits are 0x7F (no carry across bytes)
      nan = (nan >> 7) * 0xffu;
      out[i] = (out[i] & ~nan) | (w[i] & nan);
    }
    *(u32x4*)at = out;
  }
  if (p.amax == nullptr) return;   // kernel-uniform
  kmax = wave_max(kmax);
  if ((tid & 63) == 0) s_max[tid >> 6] = kmax;
  __syncthreads();
  if (tid == 0) {
    const unsigned bits = __float_as_uint(fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3])));
    if (bits > __atomic_load_n(p.amax, __ATOMIC_RELAXED)) atomicMax(p.amax, bits);
  }
}

static bool good_scale(float s) { return std::isfinite(s) && s > 0.f; }

}  // namespace rtv

using namespace rtv;

extern "C" int rtv_qk_norm_rope_k8_centered(const void* qkv, void* q_out, void* k8, int cache_rows, float k_scale, void* amax,
                                            int cache_row0, int M, int d, int num_heads, float eps, const void* wq, const void* wk,
                                            const void* rope_cs, int F, int gh, int gw, int start_frame, int row_offset, int ring_lo,
                                            int ring_size, int ring_shift, const float* center, rtv_stream_t stream) {
  if (!center || ((uintptr_t)center & 15))
    return set_error(-1, "qk_norm_rope_k8: center must be a 16-byte aligned device float[H][128]");
  if (M <= 0) return 0;
  // the list of rtv_qk_norm_rope_k8, with its messages
  if (qk_norm_rope_check(d, cache_row0, M, d, num_heads, F, gh, gw, start_frame, row_offset, 0, 0, 0, ring_lo, ring_size, ring_shift,
                         q_out ? 3 : 2))
    return -1;
  if (d / num_heads != ATT_D) return set_error(-1, "qk_norm_rope_k8: head_dim must be 128");
  if (!qkv || !k8 || !wq || !wk || !rope_cs) return set_error(-1, "qk_norm_rope_k8: null pointer");
  if (((uintptr_t)qkv | (uintptr_t)q_out | (uintptr_t)k8 | (uintptr_t)wq | (uintptr_t)wk) & 15)
    return set_error(-1, "qk_norm_rope_k8: qkv, q_out, k8, wq and wk must be 16-byte aligned");
  if (((uintptr_t)rope_cs & 7) || ((uintptr_t)amax & 3)) return set_error(-1, "qk_norm_rope_k8: rope_cs must be 8-byte, amax 4-byte aligned");
  if (cache_rows <= 0) return set_error(-1, "qk_norm_rope_k8: cache_rows must be positive");
  const int64_t end = ring_size > 0 ? (int64_t)ring_lo + ring_size : (int64_t)cache_row0 + row_offset + M;
  if (end > cache_rows) return set_error(-1, "qk_norm_rope_k8: row range outside [0, cache_rows)");
  if (!good_scale(k_scale)) return set_error(-1, "qk_norm_rope_k8: k_scale must be finite and positive");
  RopeK8CenteredArgs a;
  a.qkv = (const bf16_t*)qkv;
  a.q_out = (bf16_t*)q_out;
  a.k8 = (uint8_t*)k8;
  a.amax = (unsigned*)amax;
  a.center = center;
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
  // bytes: q read + written as bf16, k read as bf16 and written as codes (the centre stays in L2)
  ProfScope prof(PROF_ROPE, (hipStream_t)stream, ((q_out ? 4.0 : 0.0) + 3.0) * M * d);
  const int waves = M * (q_out ? 2 : 1);
  const dim3 grid((waves + ROWS_PER_WG - 1) / ROWS_PER_WG);
#define RTV_ROPE_K8C_CALL(CPL) hipLaunchKernelGGL(qk_norm_rope_k8_centered_kernel<CPL>, grid, dim3(EW_THREADS), 0, (hipStream_t)stream, a)
  RTV_ROW_DISPATCH(d, RTV_ROPE_K8C_CALL);
#undef RTV_ROPE_K8C_CALL
  return check_launch("qk_norm_rope_k8_centered");
}

extern "C" int rtv_attn_k8_center(const void* k8, int cache_rows, int row0, int n0, int row1, int n1, int H, float k_scale,
                                  const float* c_old, float* center_new, void* workspace, size_t workspace_bytes, rtv_stream_t stream) {
  if (!k8 || !c_old || !center_new || !workspace) return set_error(-1, "attn_k8_center: null pointer");
  if (((uintptr_t)k8 | (uintptr_t)c_old | (uintptr_t)center_new | (uintptr_t)workspace) & 15)
    return set_error(-1, "attn_k8_center: k8, c_old, center_new and workspace must be 16-byte aligned");
  if (n0 <= 0 || H <= 0 || cache_rows <= 0) return set_error(-1, "attn_k8_center: n0, H and cache_rows must be positive");
  if (n1 < 0) return set_error(-1, "attn_k8_center: negative segment length");
  if (row0 < 0 || (int64_t)row0 + n0 > cache_rows || (n1 > 0 && (row1 < 0 || (int64_t)row1 + n1 > cache_rows)))
    return set_error(-1, "attn_k8_center: row range outside [0, cache_rows)");
  if ((int64_t)n0 + n1 > INT32_MAX) return set_error(-1, "attn_k8_center: too many rows");
  if (!good_scale(k_scale)) return set_error(-1, "attn_k8_center: k_scale must be finite and positive");
  if (H > 65535) return set_error(-1, "attn_k8_center: more than 65535 heads");
  if (workspace_bytes < rtv_attn_kv_center_workspace_bytes(n0 + n1, H))
    return set_error(-1, "attn_k8_center: workspace below rtv_attn_kv_center_workspace_bytes(n0 + n1, H)");
  K8CenterParams p;
  p.k8 = (const uint8_t*)k8;
  p.row0 = row0;
  p.n0 = n0;
  p.row1 = row1;
  p.n1 = n1;
  p.H = H;
  p.k_scale = k_scale;
  p.c_old = c_old;
  p.part = (float*)workspace;
  p.center = center_new;
  p.chunks = (n0 + n1 + RTV_ATTN_CENTER_CHUNK - 1) / RTV_ATTN_CENTER_CHUNK;
  ProfScope prof(PROF_MISC, (hipStream_t)stream, 1.0 * (n0 + n1) * H * ATT_D);
  hipLaunchKernelGGL(attn_k8_center_partial_kernel, dim3(p.chunks, H), dim3(256), 0, (hipStream_t)stream, p);
  hipLaunchKernelGGL(attn_k8_center_reduce_kernel, dim3(H), dim3(ATT_D), 0, (hipStream_t)stream, p);
  return check_launch("attn_k8_center");
}

extern "C" int rtv_attn_k8_recenter(void* k8, int cache_rows, int row0, int rows, int H, float k_scale, const float* c_old,
                                    const float* c_new, void* amax, rtv_stream_t stream) {
  if (!k8 || !c_old || !c_new) return set_error(-1, "attn_k8_recenter: null pointer");
  if (((uintptr_t)k8 | (uintptr_t)c_old | (uintptr_t)c_new) & 15)
    return set_error(-1, "attn_k8_recenter: k8, c_old and c_new must be 16-byte aligned");
  if ((uintptr_t)amax & 3) return set_error(-1, "attn_k8_recenter: amax must be 4-byte aligned");
  if (rows <= 0 || H <= 0 || cache_rows <= 0) return set_error(-1, "attn_k8_recenter: rows, H and cache_rows must be positive");
  if (row0 < 0 || (int64_t)row0 + rows > cache_rows) return set_error(-1, "attn_k8_recenter: row range outside [0, cache_rows)");
  if (!good_scale(k_scale)) return set_error(-1, "attn_k8_recenter: k_scale must be finite and positive");
  if (H > 65535) return set_error(-1, "attn_k8_recenter: more than 65535 heads");
  K8RecenterParams p;
  p.k8 = (uint8_t*)k8;
  p.row0 = row0;
  p.rows = rows;
  p.H = H;
  p.k_scale = k_scale;
  p.c_old = c_old;
  p.c_new = c_new;
  p.amax = (unsigned*)amax;
  ProfScope prof(PROF_MISC, (hipStream_t)stream, 2.0 * rows * H * ATT_D);
  hipLaunchKernelGGL(attn_k8_recenter_kernel, dim3((rows + RECENTER_ROWS - 1) / RECENTER_ROWS, H), dim3(256), 0, (hipStream_t)stream, p);
  return check_launch("attn_k8_recenter");
}
