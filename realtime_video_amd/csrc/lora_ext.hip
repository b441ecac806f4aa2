// The extended LoRA merges (include/rtv_hip_lora_ext.h): rtv_lora_merge_ex, low-rank pairs plus dense deltas in one launch, and
// rtv_lora_merge_dora, the row-normalised DoRA merge in two.
//
// All three kernels are one template over the tile code of lora.hip, restated here so that lora.hip and the arithmetic of
// rtv_lora_merge stay as they are: a workgroup owns a 64-row x 128-column tile, base is read and W written in the copy layout
// (eight lanes on the 128 contiguous bytes of a row piece), the low-rank product comes out of mfma_f32_32x32x16_bf16 with the
// weight's row on the MFMA column and reaches the copy layout through an fp32 image in LDS (see the head of lora.hip for the
// layouts).  What is new happens in the copy layout, after the image has been read back:
//   EX     delta = image + sum_t diff_scale_t * diff_t, the diffs read as base is; a zero delta keeps the bits of base.
//   NORM   V = base + image; one fp32 sum of V^2 per (row, tile): 8 squares as a tree on the lane, 8 lanes of the row's 64-column
//          half by three butterfly steps, the two halves (two waves) through LDS.  One store per row, no atomics.
//   DORA   the row's partials added in a fixed order (four runs of consecutive tiles, one per wave, then the four sums by one
//          thread per row), g = mag / sqrt(sum); V recomputed by the very code of NORM; W = base + strength * (g V - base).
#include <math.h>
#include <stdio.h>

#include "rtv_common.h"
#include "rtv_internal.h"
#include "../../include/rtv_hip_lora_ext.h"

namespace rtv {

constexpr int LX_TN = 64, LX_TK = 128, LX_RC = 64, LX_LD = LX_RC + 8;   // as LM_* of lora.hip
constexpr int LX_DLD = 64 + 4;
constexpr int LX_OPERAND_BYTES = (LX_TK + LX_TN) * LX_LD * 2, LX_IMAGE_BYTES = 4 * 32 * LX_DLD * 4;
constexpr int LX_LDS_BYTES = LX_OPERAND_BYTES > LX_IMAGE_BYTES ? LX_OPERAND_BYTES : LX_IMAGE_BYTES;

enum { LX_EX = 0, LX_NORM = 1, LX_DORA = 2 };

struct LoraExArgs {
  const bf16_t* base;
  bf16_t* W;
  int64_t ldb, ldw;
  int N, K, count, tiles_k;               // count: low-rank pairs
  const bf16_t* A[RTV_LORA_MAX_ADAPTERS];
  const bf16_t* B[RTV_LORA_MAX_ADAPTERS];
  int rank[RTV_LORA_MAX_ADAPTERS];
  int b_vec[RTV_LORA_MAX_ADAPTERS];      // B rows are 16-byte pieces (rank % 8 == 0, aligned pointer)
  float scale[RTV_LORA_MAX_ADAPTERS];
  int ndiff;                              // EX: dense deltas
  const bf16_t* diff[RTV_LORA_MAX_ADAPTERS];
  int64_t ldd[RTV_LORA_MAX_ADAPTERS];
  float dscale[RTV_LORA_MAX_ADAPTERS];
  const bf16_t* mag;                      // NORM / DORA
  float* part;                            // [tiles_k][N] partial sums of V^2
  float strength;
};

template <int MODE>
__global__ __launch_bounds__(256, 4) void lora_ex_kernel(const LoraExArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[LX_LDS_BYTES];
  __shared__ float rowv[4][LX_TN];        // NORM: [0], [1] the two 64-column halves of a row's sum; DORA: quarter sums, then [0] = g, [1] = nrm
  bf16_t* const At = (bf16_t*)smem;
  bf16_t* const Bs = At + LX_TK * LX_LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int tile_k = (int)(blockIdx.x % a.tiles_k);
  const int n0 = (int)(blockIdx.x / a.tiles_k) * LX_TN, k0 = tile_k * LX_TK;
  const int nw = 32 * (wave & 1), kw = 64 * (wave >> 1);
  const int N = a.N, K = a.K;

  // the lane's pieces of base, in the copy layout: piece `it` is row nw + 8 it + lane / 8, columns kw + 8 (lane % 8) .. + 7
  const int er = lane >> 3, ek = k0 + kw + 8 * (lane & 7);
  u32x4 bv[4];
  bool ok[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int n = n0 + nw + 8 * it + er;
    ok[it] = n < N && ek < K;
    bv[it] = u32x4{0, 0, 0, 0};
    if (ok[it]) bv[it] = *(const u32x4*)(a.base + (int64_t)n * a.ldb + ek);
  }

  if (MODE == LX_DORA) {
    // the row's partials in a fixed order - the same in every workgroup of the row, on every call: wave q adds a quarter of them
    // (consecutive tiles, in tile order) for all 64 rows, lanes on consecutive rows; one thread per row adds the four in order
    const int n = n0 + lane, per = (a.tiles_k + 3) >> 2, t0 = wave * per, t1 = min(t0 + per, a.tiles_k);
    float s = 0.f;
    if (n < N) {
#pragma unroll 8
      for (int t = t0; t < t1; ++t) s += a.part[(int64_t)t * N + n];
    }
    rowv[wave][lane] = s;
    __syncthreads();
    if (tid < LX_TN) {
      s = ((rowv[0][tid] + rowv[1][tid]) + rowv[2][tid]) + rowv[3][tid];
      const float m = n < N ? __uint_as_float((uint32_t)a.mag[n] << 16) : 0.f, nrm = sqrtf(s);
      rowv[0][tid] = nrm > 0.f ? m / nrm : 0.f;      // (a thread reads and writes its own row only; read after the barriers below)
      rowv[1][tid] = nrm;
    }
  }

  f32x16 tot[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) tot[t][i] = 0.f;

  for (int ad = 0; ad < a.count; ++ad) {
    const bf16_t* __restrict__ A = a.A[ad];
    const bf16_t* __restrict__ B = a.B[ad];
    const int rank = a.rank[ad], rp = (rank + 15) & ~15;
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    for (int j0 = 0; j0 < rp; j0 += LX_RC) {
      const int rc = min(LX_RC, rp - j0);      // a multiple of 16
      __syncthreads();                         // the previous chunk's fragments have been read
      // At: task = (pair of rank rows, 8 columns); consecutive lanes take consecutive pairs, so the 4-byte LDS writes of a wave
      // instruction fall on consecutive banks
      const int pairs = rc >> 1;
      for (int t = tid; t < pairs * (LX_TK / 8); t += 256) {
        const int jp = t % pairs, c = t / pairs;
        const int j = j0 + 2 * jp, k = k0 + 8 * c;
        u32x4 v0 = {0, 0, 0, 0}, v1 = {0, 0, 0, 0};
        if (k < K && j < rank) v0 = *(const u32x4*)(A + (int64_t)j * K + k);
        if (k < K && j + 1 < rank) v1 = *(const u32x4*)(A + (int64_t)(j + 1) * K + k);
        uint32_t* dst = (uint32_t*)&At[(8 * c) * LX_LD + 2 * jp];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t x = v0[i], y = v1[i];
          dst[(2 * i) * (LX_LD / 2)] = (x & 0xffffu) | (y << 16);
          dst[(2 * i + 1) * (LX_LD / 2)] = (x >> 16) | (y & 0xffff0000u);
        }
      }
      if (a.b_vec[ad]) {
        const int pieces = rc >> 3;
        for (int t = tid; t < LX_TN * pieces; t += 256) {
          const int jc = t % pieces, nl = t / pieces;
          const int j = j0 + 8 * jc;
          u32x4 v = {0, 0, 0, 0};
          if (n0 + nl < N && j < rank) v = *(const u32x4*)(B + (int64_t)(n0 + nl) * rank + j);
          *(u32x4*)&Bs[nl * LX_LD + 8 * jc] = v;
        }
      } else {
        for (int t = tid; t < LX_TN * rc; t += 256) {
          const int jl = t % rc, nl = t / rc;
          bf16_t v = 0;
          if (n0 + nl < N && j0 + jl < rank) v = B[(int64_t)(n0 + nl) * rank + j0 + jl];
          Bs[nl * LX_LD + jl] = v;
        }
      }
      __syncthreads();
      for (int s = 0; s < rc; s += 16) {
        const u32x4 bfrag = *(const u32x4*)&Bs[(nw + r) * LX_LD + s + 8 * h];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const u32x4 afrag = *(const u32x4*)&At[(kw + 32 * t + r) * LX_LD + s + 8 * h];
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, afrag), __builtin_bit_cast(bf16x8, bfrag),
                                                           acc[t], 0, 0, 0);
        }
      }
    }
    const float sc = a.scale[ad];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) tot[t][i] += sc * acc[t][i];
  }

  // MFMA row 8 g + 4 h + i of tile t is column 32 t + 8 g + 4 h + i of the wave's result: registers 4g .. 4g + 3 are one 16-byte write
  __syncthreads();      // every wave has read its last fragments: the operands' LDS becomes the result images
  float* const D = (float*)smem + wave * (32 * LX_DLD);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *(f32x4*)&D[r * LX_DLD + 32 * t + 8 * g + 4 * h] = f32x4{tot[t][4 * g], tot[t][4 * g + 1], tot[t][4 * g + 2], tot[t][4 * g + 3]};
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int nl = nw + 8 * it + er;
    const int64_t n = n0 + nl;
    const float* d = &D[(8 * it + er) * LX_DLD + 8 * (lane & 7)];
    const f32x4 d0 = *(const f32x4*)d, d1 = *(const f32x4*)(d + 4);
    float f[8], x[8];
    unpack_bf16x8(bv[it], f);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = i < 4 ? d0[i & 3] : d1[i & 3];
    if (MODE == LX_EX) {
      if (!ok[it]) continue;
      if (a.ndiff) {
        float ds[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ds[i] = 0.f;
        for (int t = 0; t < a.ndiff; ++t) {
          float g[8];
          unpack_bf16x8(*(const u32x4*)(a.diff[t] + n * a.ldd[t] + ek), g);
          const float sc = a.dscale[t];
#pragma unroll
          for (int i = 0; i < 8; ++i) ds[i] += sc * g[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] += ds[i];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) f[i] = x[i] == 0.f ? f[i] : f[i] + x[i];      // a zero sum keeps the bits of base (-0 stays -0)
      *(u32x4*)(a.W + n * a.ldw + ek) = pack_bf16x8(f);
    } else {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = f[i] + x[i];      // V: NORM and DORA run this very line (rows / columns outside: 0)
      if (MODE == LX_NORM) {
        float q = ((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3])) + ((v[4] * v[4] + v[5] * v[5]) + (v[6] * v[6] + v[7] * v[7]));
        q += __shfl_xor(q, 1);
        q += __shfl_xor(q, 2);
        q += __shfl_xor(q, 4);
        if ((lane & 7) == 0) rowv[wave >> 1][nl] = q;
      } else {
        if (!ok[it]) continue;
        const float g = rowv[0][nl], st = a.strength;
        if (st != 0.f && rowv[1][nl] > 0.f) {
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const float dl = st * (g * v[i] - f[i]);
            f[i] = dl == 0.f ? f[i] : f[i] + dl;
          }
        }
        *(u32x4*)(a.W + n * a.ldw + ek) = pack_bf16x8(f);      // (an untouched piece goes back as its own bits)
      }
    }
  }
  if (MODE == LX_NORM) {
    __syncthreads();
    if (tid < LX_TN && n0 + tid < N) a.part[(int64_t)tile_k * N + n0 + tid] = rowv[0][tid] + rowv[1][tid];
  }
}

static int lx_common(const char* who, const void* base, int ldb, void* W, int ldw, int N, int K, char* msg, size_t cap) {
  const char* what = nullptr;
  if (!base || !W) what = "null base or W pointer";
  else if (N <= 0 || K <= 0) what = "N and K must be positive";
  else if (K % 8 || ldb % 8 || ldw % 8) what = "misaligned: K and both strides must be multiples of 8";
  else if (ldb < K || ldw < K) what = "row stride below K";
  else if (((uintptr_t)base | (uintptr_t)W) & 15) what = "misaligned: base and W must be 16-byte aligned";
  if (!what) return 0;
  snprintf(msg, cap, "%s: %s", who, what);
  return -1;
}

static int lx_pair(const char* who, const char* scale_name, const void* A, const void* B, int rank, float scale, char* msg, size_t cap) {
  const char* what = nullptr;
  if (!A || !B) what = "null adapter A or B pointer";
  else if (rank < 1 || rank > RTV_LORA_MAX_RANK) what = "rank outside 1 .. RTV_LORA_MAX_RANK (256)";
  else if (!isfinite(scale)) what = "non-finite ";
  else if ((uintptr_t)A & 15) what = "misaligned: adapter A must be 16-byte aligned";
  else if ((uintptr_t)B & 1) what = "misaligned: adapter B must be 2-byte aligned";
  if (!what) return 0;
  snprintf(msg, cap, "%s: %s%s", who, what, isfinite(scale) || what[0] != 'n' || what[1] != 'o' ? "" : scale_name);
  return -1;
}

}  // namespace rtv

using namespace rtv;

extern "C" {

int rtv_lora_merge_ex(const void* base, int ldb, void* W, int ldw, int N, int K, const rtv_lora_term* terms, int count,
                      rtv_stream_t stream) {
  char msg[160];
  if (!base || !W) return set_error(-1, "lora_merge_ex: null base or W pointer");
  if (N <= 0 || K <= 0) return set_error(-1, "lora_merge_ex: N and K must be positive");
  if (count < 0 || count > RTV_LORA_MAX_ADAPTERS) return set_error(-1, "lora_merge_ex: count outside 0 .. RTV_LORA_MAX_ADAPTERS (4)");
  if (count > 0 && !terms) return set_error(-1, "lora_merge_ex: null term table");
  if (lx_common("lora_merge_ex", base, ldb, W, ldw, N, K, msg, sizeof msg)) return set_error(-1, msg);
  LoraExArgs a = {};
  a.base = (const bf16_t*)base, a.W = (bf16_t*)W, a.ldb = ldb, a.ldw = ldw, a.N = N, a.K = K;
  double flop = 0;
  for (int i = 0; i < count; ++i) {
    const rtv_lora_term& t = terms[i];
    const bool pair = t.A || t.B || t.rank != 0;
    if (!pair && !t.diff) return set_error(-1, "lora_merge_ex: a term with neither a low-rank pair nor a diff");
    if (pair) {
      if (lx_pair("lora_merge_ex", "scale", t.A, t.B, t.rank, t.scale, msg, sizeof msg)) return set_error(-1, msg);
      const int j = a.count++;
      a.A[j] = (const bf16_t*)t.A, a.B[j] = (const bf16_t*)t.B, a.rank[j] = t.rank, a.scale[j] = t.scale;
      a.b_vec[j] = t.rank % 8 == 0 && ((uintptr_t)t.B & 15) == 0;
      flop += 2.0 * N * K * t.rank;
    }
    if (t.diff) {
      if ((uintptr_t)t.diff & 15) return set_error(-1, "lora_merge_ex: misaligned: diff must be 16-byte aligned");
      if (t.ldd % 8) return set_error(-1, "lora_merge_ex: misaligned: a diff stride must be a multiple of 8");
      if (t.ldd < K) return set_error(-1, "lora_merge_ex: diff row stride below K");
      if (!isfinite(t.diff_scale)) return set_error(-1, "lora_merge_ex: non-finite diff_scale");
      const int j = a.ndiff++;
      a.diff[j] = (const bf16_t*)t.diff, a.ldd[j] = t.ldd, a.dscale[j] = t.diff_scale;
    }
  }
  a.tiles_k = (K + LX_TK - 1) / LX_TK;
  const int64_t tiles = (int64_t)a.tiles_k * ((N + LX_TN - 1) / LX_TN);
  if (tiles > 0x7fffffff) return set_error(-1, "lora_merge_ex: matrix too large for one launch");
  ProfScope prof(PROF_MISC, (hipStream_t)stream, flop);
  hipLaunchKernelGGL(lora_ex_kernel<LX_EX>, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("lora_merge_ex");
}

size_t rtv_lora_dora_workspace_bytes(int N, int K) {
  if (N <= 0 || K <= 0) return 0;
  const size_t bytes = (size_t)N * (size_t)((K + LX_TK - 1) / LX_TK) * sizeof(float);
  return (bytes + 15) & ~(size_t)15;
}

int rtv_lora_merge_dora(const void* base, int ldb, void* W, int ldw, int N, int K, const void* A, const void* B, int rank,
                        float factor, const void* mag, float strength, void* workspace, size_t workspace_bytes, rtv_stream_t stream) {
  char msg[160];
  if (lx_common("lora_merge_dora", base, ldb, W, ldw, N, K, msg, sizeof msg)) return set_error(-1, msg);
  if (lx_pair("lora_merge_dora", "factor", A, B, rank, factor, msg, sizeof msg)) return set_error(-1, msg);
  if (!isfinite(strength)) return set_error(-1, "lora_merge_dora: non-finite strength");
  if (!mag) return set_error(-1, "lora_merge_dora: null mag pointer");
  if ((uintptr_t)mag & 1) return set_error(-1, "lora_merge_dora: misaligned: mag must be 2-byte aligned");
  if (!workspace) return set_error(-1, "lora_merge_dora: null workspace");
  if ((uintptr_t)workspace & 15) return set_error(-1, "lora_merge_dora: misaligned: workspace must be 16-byte aligned");
  if (workspace_bytes < rtv_lora_dora_workspace_bytes(N, K))
    return set_error(-1, "lora_merge_dora: workspace too small (rtv_lora_dora_workspace_bytes)");
  LoraExArgs a = {};
  a.base = (const bf16_t*)base, a.W = (bf16_t*)W, a.ldb = ldb, a.ldw = ldw, a.N = N, a.K = K, a.count = 1;
  a.A[0] = (const bf16_t*)A, a.B[0] = (const bf16_t*)B, a.rank[0] = rank, a.scale[0] = factor;
  a.b_vec[0] = rank % 8 == 0 && ((uintptr_t)B & 15) == 0;
  a.mag = (const bf16_t*)mag, a.part = (float*)workspace, a.strength = strength;
  a.tiles_k = (K + LX_TK - 1) / LX_TK;
  const int64_t tiles = (int64_t)a.tiles_k * ((N + LX_TN - 1) / LX_TN);
  if (tiles > 0x7fffffff) return set_error(-1, "lora_merge_dora: matrix too large for one launch");
  ProfScope prof(PROF_MISC, (hipStream_t)stream, 4.0 * N * K * rank);
  hipLaunchKernelGGL(lora_ex_kernel<LX_NORM>, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, a);
  if (int rc = check_launch("lora_merge_dora (norm pass)")) return rc;
  hipLaunchKernelGGL(lora_ex_kernel<LX_DORA>, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("lora_merge_dora");
}

}  // extern "C"
