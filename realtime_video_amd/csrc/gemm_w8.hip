// Weight-only fp8 GEMM for the text encoder's Linears at prompt length (include/rtv_hip_t5_w8.h):
//   C[m][n] = bf16( fp32_acc( sum_k A[m][k] * value(Wq[n][k]) ) * s_w[n] ),   A bf16 [M][K], Wq e4m3 codes [N][K], M = 32 .. 128 (.. 512)
// The shape is bound by the weight bytes, so the kernel is built around streaming them once:
//   * a workgroup (4 waves) owns W8_STRIP = 64 output channels, 16 per wave, for a chunk of at most W8_CHUNK = 128 rows and one
//     segment of K.  Its codes go HBM -> VGPRs as 16-byte non-temporal loads, 32 contiguous bytes of one weight row per lane and
//     K step (16 rows x 128 bytes per wave: whole lines), through a ring W8_RING steps deep; no LDS round trip.
//   * a code becomes bf16 in registers: v_cvt_pk_f32_fp8 (exact) and the high halves of the two floats (exact: e4m3 fits bf16).
//   * the rows come through LDS: 256 bytes (128 k) per row and K step, loaded in whole lines by 16 neighbouring threads, 16-byte
//     piece p of row r at p ^ (r & 15) so that the 16 rows a ds_read_b128 group reads are 16 different pieces of the 256-byte bank row.
//   * MFMA 16x16x32 bf16 with the weight as the first operand (gemm_core.h, Mfma16): a lane owns row m = l & 15 and the 4 consecutive
//     channels 4 (l >> 4) + r.  The k order inside a step is permuted (a lane's 32 bytes feed 4 MFMAs), the same way for both operands.
//   * K split: w8_segments(N, K) - a function of N and K alone - segments; each writes fp32 partials [segment][M][N] to the
//     workspace, gemm_w8_reduce_kernel adds them in ascending order, scales, rounds and stores.  One segment: the kernel stores itself.
// Nothing depends on M but the row chunks, and a row's arithmetic never sees another row: an output row has the same bits in every
// launch that holds it.
#include "gemm_core.h"
#include "rtv_common.h"
#include "rtv_internal.h"
#include "../../include/rtv_hip_t5_w8.h"

namespace rtv {

constexpr int W8_KSTEP = 128;       // k per step: K % W8_KSTEP == 0
constexpr int W8_STRIP = 64;        // output channels per workgroup
constexpr int W8_CHUNK = 128;       // rows per workgroup at most
constexpr int W8_RING = 4;          // K steps of codes in flight per wave
constexpr int W8_TARGET_WGS = 512;  // strips x segments the plan aims at (a constant: NOT the device's CU count)
constexpr int W8_MAX_SEGMENTS = 16;

// K segments for (N, K): enough that strips x segments reaches W8_TARGET_WGS, each at least two K steps long
static inline int w8_segments(int N, int K) {
  const int steps = K / W8_KSTEP, strips = (N + W8_STRIP - 1) / W8_STRIP;
  int s = (W8_TARGET_WGS + strips - 1) / strips;
  if (s > W8_MAX_SEGMENTS) s = W8_MAX_SEGMENTS;
  if (s > steps / 2) s = steps / 2;
  return s < 1 ? 1 : s;
}

struct W8Params {
  const bf16_t* A;
  const uint8_t* Wq;
  const float* scales;
  bf16_t* C;
  float* slabs;       // [segments][M][N] when segments > 1
  int lda, ldw, ldc, transpose;
  int M, N, K, segments;
  int m_base;         // first row of this launch's chunks
};

// 4 codes -> 4 bf16 (two packed pairs), exact
__device__ __forceinline__ u32x2 w8_decode4(uint32_t codes) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)codes, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)codes, true);
  const float a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
  return u32x2{(__float_as_uint(a0) >> 16) | (__float_as_uint(a1) & 0xffff0000u),
               (__float_as_uint(b0) >> 16) | (__float_as_uint(b1) & 0xffff0000u)};
}
// 8 codes (two words of a lane's 32 bytes) -> one MFMA operand
__device__ __forceinline__ u32x4 w8_decode8(uint32_t w0, uint32_t w1) {
  const u32x2 x = w8_decode4(w0), y = w8_decode4(w1);
  return u32x4{x[0], x[1], y[0], y[1]};
}

// y = bf16(acc * s) for a lane's 4 consecutive channels of row m
__device__ __forceinline__ void w8_store_quad(const W8Params& p, int m, int n, const float* acc4) {
  const float4 s = *(const float4*)(p.scales + n);
  const float v0 = acc4[0] * s.x, v1 = acc4[1] * s.y, v2 = acc4[2] * s.z, v3 = acc4[3] * s.w;
  if (!p.transpose) {
    *(u32x2*)(p.C + (size_t)m * p.ldc + n) = u32x2{pack_bf16x2(v0, v1), pack_bf16x2(v2, v3)};
  } else {
    bf16_t* c = p.C + (size_t)n * p.ldc + m;
    c[0] = f32_to_bf16(v0);
    c[(size_t)p.ldc] = f32_to_bf16(v1);
    c[(size_t)2 * p.ldc] = f32_to_bf16(v2);
    c[(size_t)3 * p.ldc] = f32_to_bf16(v3);
  }
}

// MT = 16-row blocks of the row chunk (2, 4, 6, 8).  grid = (strips, segments, chunks), 256 threads.
template <int MT>
__global__ __launch_bounds__(256) void gemm_w8_kernel(W8Params p) {
  __shared__ __attribute__((aligned(16))) char lds[MT * 16 * 256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, q = lane >> 4;
  const int steps = p.K / W8_KSTEP;
  const int ks0 = (int)((long)blockIdx.y * steps / p.segments), ks1 = (int)((long)(blockIdx.y + 1) * steps / p.segments);
  const int m0 = p.m_base + blockIdx.z * (MT * 16);
  const int n0 = blockIdx.x * W8_STRIP + wave * 16;
  // a wave past the last channel (N % 64 != 0) computes the last 16 channels again and stores nothing: no divergent barriers,
  // every load in bounds
  const bool active = n0 < p.N;
  const uint8_t* wp = p.Wq + (size_t)(min(n0, p.N - 16) + l15) * p.ldw + q * 32;
  // the rows: thread t takes 16-byte piece (t & 15) of rows (t >> 4) + 16 i
  const bf16_t* ap = p.A + (size_t)(m0 + (tid >> 4)) * p.lda + (tid & 15) * 8;
  char* aw = lds + (tid >> 4) * 256 + (((tid & 15) ^ ((tid >> 4) & 15)) << 4);

  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 wr[W8_RING][2];
#pragma unroll
  for (int d = 0; d < W8_RING; ++d) {
    const uint8_t* s = wp + (size_t)min(ks0 + d, ks1 - 1) * W8_KSTEP;   // steps past the segment's end re-read its last step
    wr[d][0] = __builtin_nontemporal_load((const u32x4*)s);
    wr[d][1] = __builtin_nontemporal_load((const u32x4*)(s + 16));
  }
  u32x4 ar[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) ar[i] = *(const u32x4*)(ap + (size_t)i * 16 * p.lda + (size_t)ks0 * W8_KSTEP);

  // one K step: the staged rows go to LDS, the next step's rows are requested (the last step requests itself again), then the
  // step's codes (the lane's 32 bytes) are decoded and meet the rows
  auto stage = [&](int step) {
    __syncthreads();             // the previous step's fragment reads are done
#pragma unroll
    for (int i = 0; i < MT; ++i) *(u32x4*)(aw + i * 16 * 256) = ar[i];
    __syncthreads();
    const size_t k = (size_t)min(step + 1, ks1 - 1) * W8_KSTEP;
#pragma unroll
    for (int i = 0; i < MT; ++i) ar[i] = *(const u32x4*)(ap + (size_t)i * 16 * p.lda + k);
  };
  // MFMA j of a step takes the lane's code bytes 8 j .. 8 j + 7 = k  32 q + 8 j ..
  auto decode = [&](const u32x4& c0, const u32x4& c1, u32x4* wf) {
    wf[0] = w8_decode8(c0[0], c0[1]);
    wf[1] = w8_decode8(c0[2], c0[3]);
    wf[2] = w8_decode8(c1[0], c1[1]);
    wf[3] = w8_decode8(c1[2], c1[3]);
  };
  auto compute = [&](const u32x4* wf) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const char* row = lds + (mt * 16 + l15) * 256;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u32x4 af = *(const u32x4*)(row + (((q * 4 + j) ^ l15) << 4));
        acc[mt] = Mfma16<false>::run(wf[j], af, acc[mt]);
      }
    }
  };
  // whole rounds of the ring: straight-line code (a branch per step makes hipcc drain the ring at every step), the refill of a
  // slot issued behind the row loads of the step, so that waiting for those rows leaves it in flight
  int ks = ks0;
  for (; ks + W8_RING <= ks1; ks += W8_RING) {
#pragma unroll
    for (int u = 0; u < W8_RING; ++u) {
      stage(ks + u);
      u32x4 wf[4];
      decode(wr[u][0], wr[u][1], wf);
      const uint8_t* s = wp + (size_t)min(ks + u + W8_RING, ks1 - 1) * W8_KSTEP;
      wr[u][0] = __builtin_nontemporal_load((const u32x4*)s);
      wr[u][1] = __builtin_nontemporal_load((const u32x4*)(s + 16));
      compute(wf);
    }
  }
  // the steps left, fewer than a round: their codes are in the ring's first slots, nothing is refilled
#pragma unroll
  for (int u = 0; u < W8_RING - 1; ++u) {
    if (ks + u < ks1) {            // uniform over the workgroup
      stage(ks + u);
      u32x4 wf[4];
      decode(wr[u][0], wr[u][1], wf);
      compute(wf);
    }
  }

  if (!active) return;
  const int n = n0 + q * 4;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m0 + mt * 16 + l15;
    const float v[4] = {acc[mt][0], acc[mt][1], acc[mt][2], acc[mt][3]};
    if (p.segments == 1) w8_store_quad(p, m, n, v);
    else *(float4*)(p.slabs + ((size_t)blockIdx.y * p.M + m) * p.N + n) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// the segments' partials, added in ascending segment order; one thread per (row, 4 channels)
__global__ __launch_bounds__(256) void gemm_w8_reduce_kernel(W8Params p) {
  const size_t per_row = p.N / 4, total = (size_t)p.M * per_row;
  const size_t slab = (size_t)p.M * p.N;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int m = (int)(i / per_row), n = (int)(i - (size_t)m * per_row) * 4;
    const float* src = p.slabs + (size_t)m * p.N + n;
    float4 a = *(const float4*)src;
    for (int s = 1; s < p.segments; ++s) {
      const float4 b = *(const float4*)(src + s * slab);
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    const float v[4] = {a.x, a.y, a.z, a.w};
    w8_store_quad(p, m, n, v);
  }
}

static bool w8_misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

template <int MT>
static void w8_launch(const W8Params& p, int strips, int chunks, hipStream_t st) {
  hipLaunchKernelGGL(gemm_w8_kernel<MT>, dim3(strips, p.segments, chunks), dim3(256), 0, st, p);
}

}  // namespace rtv

using namespace rtv;

extern "C" int rtv_gemm_w8_segments(int N, int K) {
  if (N <= 0 || N % 16 || K <= 0 || K % W8_KSTEP) return 0;
  return w8_segments(N, K);
}

extern "C" size_t rtv_gemm_w8_workspace_bytes(int M, int N, int K) {
  if (M <= 0 || M % 32) return 0;
  const int s = rtv_gemm_w8_segments(N, K);
  return s > 1 ? (size_t)s * M * N * sizeof(float) : 0;
}

extern "C" int rtv_gemm_w8(const void* A, int lda, const void* Wq, int ldw, const float* w_row_scales, void* C, int ldc,
                           int transpose_out, int M, int N, int K, void* workspace, size_t workspace_bytes, rtv_stream_t stream) {
  if (!A || !Wq || !w_row_scales || !C) return set_error(-1, "gemm_w8: null pointer");
  if (M <= 0 || M % 32) return set_error(-1, "gemm_w8: M must be a positive multiple of 32");
  if (K <= 0 || K % W8_KSTEP) return set_error(-1, "gemm_w8: K must be a positive multiple of 128");
  if (N <= 0 || N % 16) return set_error(-1, "gemm_w8: N must be a positive multiple of 16");
  if (transpose_out != 0 && transpose_out != 1) return set_error(-1, "gemm_w8: transpose_out must be 0 or 1");
  if (lda < K || lda % 8) return set_error(-1, "gemm_w8: lda must be a multiple of 8 elements and at least K");
  if (ldw < K || ldw % 16) return set_error(-1, "gemm_w8: ldw must be a multiple of 16 bytes and at least K");
  if (transpose_out ? ldc < M : (ldc < N || ldc % 4))
    return set_error(-1, "gemm_w8: ldc must be at least N and a multiple of 4 (transposed: at least M)");
  if (w8_misaligned(A, 16) || w8_misaligned(Wq, 16)) return set_error(-1, "gemm_w8: A and Wq must be 16-byte aligned");
  if (w8_misaligned(C, transpose_out ? 2 : 8)) return set_error(-1, "gemm_w8: C must be 8-byte aligned (transposed: 2-byte)");
  if (w8_misaligned(w_row_scales, 16)) return set_error(-1, "gemm_w8: w_row_scales must be 16-byte aligned");
  const int segments = w8_segments(N, K);
  if (segments > 1) {
    if (!workspace || w8_misaligned(workspace, 16)) return set_error(-1, "gemm_w8: this (N, K) splits K: workspace must be a 16-byte aligned buffer");
    if (workspace_bytes < rtv_gemm_w8_workspace_bytes(M, N, K))
      return set_error(-1, "gemm_w8: workspace too small (see rtv_gemm_w8_workspace_bytes)");
  }
  hipStream_t st = (hipStream_t)stream;
  W8Params p{(const bf16_t*)A, (const uint8_t*)Wq, w_row_scales, (bf16_t*)C, (float*)workspace, lda, ldw, ldc, transpose_out,
             M, N, K, segments, 0};
  const int strips = (N + W8_STRIP - 1) / W8_STRIP, full = M / W8_CHUNK, rest = M % W8_CHUNK;
  {
    ProfScope prof(PROF_GEMM, st, 2.0 * M * (double)N * K);
    if (full) w8_launch<8>(p, strips, full, st);
    p.m_base = full * W8_CHUNK;
    if (rest == 32) w8_launch<2>(p, strips, 1, st);
    else if (rest == 64) w8_launch<4>(p, strips, 1, st);
    else if (rest == 96) w8_launch<6>(p, strips, 1, st);
    if (segments > 1) {
      const size_t quads = (size_t)M * N / 4;
      const int blocks = (int)((quads + 255) / 256 > 2048 ? 2048 : (quads + 255) / 256);
      hipLaunchKernelGGL(gemm_w8_reduce_kernel, dim3(blocks), dim3(256), 0, st, p);
    }
  }
  return check_launch("gemm_w8");
}
