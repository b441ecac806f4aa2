// LoRA merge (include/rtv_hip_lora.h): W = bf16( base + sum_a scale_a * B_a @ A_a ) over one weight matrix, in place or not.
//
// The kernel is bound by memory (base read once, W written once; the low-rank operands are small and live in L2), so the layout
// serves the copy: base is read and W written as a copy kernel would, eight lanes on the 128 contiguous bytes of a row piece, and
// the low-rank product is brought into THAT layout through LDS.  mfma_f32_32x32x16_bf16 keeps the column of its result on the lane
// and four consecutive rows per register quad; with the weight's row n on the MFMA column and the weight's column k on the MFMA
// row, a lane's quad is four consecutive k of one row n: one 16-byte LDS write into a [n][k] fp32 image of the wave's 32 x 64
// result, which the epilogue reads back row-wise next to the base pieces it loaded at the start.
//
// Operands per workgroup tile (64 rows x 128 columns, 4 waves of 32 x 64) and rank chunk of 64, staged through LDS:
//   Bs[n][j]  <- B[n][j]   ("up", row-major along the rank: the MFMA B operand reads 8 consecutive j of row n, as stored)
//   At[k][j]  <- A[j][k]   ("down", row-major along k: transposed on the way in, two rank rows packed per 4-byte LDS write)
// Ranks are padded to the MFMA k-step (16) with zeros in LDS; rows >= N and columns >= K are zero-filled and never stored.
// The fp32 image reuses the operands' LDS once the last fragment has been read.
#include <math.h>

#include "rtv_common.h"
#include "rtv_internal.h"
#include "../../include/rtv_hip_lora.h"

namespace rtv {

constexpr int LM_TN = 64, LM_TK = 128, LM_RC = 64, LM_LD = LM_RC + 8;   // LD: +16 bytes per row, ds_read_b128 rows fall on distinct banks
constexpr int LM_DLD = 64 + 4;                                          // floats per row of a wave's 32 x 64 result image
constexpr int LM_OPERAND_BYTES = (LM_TK + LM_TN) * LM_LD * 2, LM_IMAGE_BYTES = 4 * 32 * LM_DLD * 4;
constexpr int LM_LDS_BYTES = LM_OPERAND_BYTES > LM_IMAGE_BYTES ? LM_OPERAND_BYTES : LM_IMAGE_BYTES;

struct LoraArgs {
  const bf16_t* base;
  bf16_t* W;
  int64_t ldb, ldw;
  int N, K, count, tiles_k;
  const bf16_t* A[RTV_LORA_MAX_ADAPTERS];
  const bf16_t* B[RTV_LORA_MAX_ADAPTERS];
  int rank[RTV_LORA_MAX_ADAPTERS];
  int b_vec[RTV_LORA_MAX_ADAPTERS];      // B rows are 16-byte pieces (rank % 8 == 0, aligned pointer)
  float scale[RTV_LORA_MAX_ADAPTERS];
};

__global__ __launch_bounds__(256, 4) void lora_merge_kernel(const LoraArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[LM_LDS_BYTES];
  bf16_t* const At = (bf16_t*)smem;
  bf16_t* const Bs = At + LM_TK * LM_LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int n0 = (int)(blockIdx.x / a.tiles_k) * LM_TN, k0 = (int)(blockIdx.x % a.tiles_k) * LM_TK;
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
    for (int j0 = 0; j0 < rp; j0 += LM_RC) {
      const int rc = min(LM_RC, rp - j0);      // a multiple of 16
      __syncthreads();                         // the previous chunk's fragments have been read
      // At: task = (pair of rank rows, 8 columns); consecutive lanes take consecutive pairs, so the 4-byte LDS writes of a wave
      // instruction fall on consecutive banks
      const int pairs = rc >> 1;
      for (int t = tid; t < pairs * (LM_TK / 8); t += 256) {
        const int jp = t % pairs, c = t / pairs;
        const int j = j0 + 2 * jp, k = k0 + 8 * c;
        u32x4 v0 = {0, 0, 0, 0}, v1 = {0, 0, 0, 0};
        if (k < K && j < rank) v0 = *(const u32x4*)(A + (int64_t)j * K + k);
        if (k < K && j + 1 < rank) v1 = *(const u32x4*)(A + (int64_t)(j + 1) * K + k);
        uint32_t* dst = (uint32_t*)&At[(8 * c) * LM_LD + 2 * jp];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t x = v0[i], y = v1[i];
          dst[(2 * i) * (LM_LD / 2)] = (x & 0xffffu) | (y << 16);
          dst[(2 * i + 1) * (LM_LD / 2)] = (x >> 16) | (y & 0xffff0000u);
        }
      }
      if (a.b_vec[ad]) {
        const int pieces = rc >> 3;
        for (int t = tid; t < LM_TN * pieces; t += 256) {
          const int jc = t % pieces, nl = t / pieces;
          const int j = j0 + 8 * jc;
          u32x4 v = {0, 0, 0, 0};
          if (n0 + nl < N && j < rank) v = *(const u32x4*)(B + (int64_t)(n0 + nl) * rank + j);
          *(u32x4*)&Bs[nl * LM_LD + 8 * jc] = v;
        }
      } else {
        for (int t = tid; t < LM_TN * rc; t += 256) {
          const int jl = t % rc, nl = t / rc;
          bf16_t v = 0;
          if (n0 + nl < N && j0 + jl < rank) v = B[(int64_t)(n0 + nl) * rank + j0 + jl];
          Bs[nl * LM_LD + jl] = v;
        }
      }
      __syncthreads();
      for (int s = 0; s < rc; s += 16) {
        const u32x4 bfrag = *(const u32x4*)&Bs[(nw + r) * LM_LD + s + 8 * h];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const u32x4 afrag = *(const u32x4*)&At[(kw + 32 * t + r) * LM_LD + s + 8 * h];
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
  float* const D = (float*)smem + wave * (32 * LM_DLD);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *(f32x4*)&D[r * LM_DLD + 32 * t + 8 * g + 4 * h] = f32x4{tot[t][4 * g], tot[t][4 * g + 1], tot[t][4 * g + 2], tot[t][4 * g + 3]};
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    if (!ok[it]) continue;
    const float* d = &D[(8 * it + er) * LM_DLD + 8 * (lane & 7)];
    const f32x4 d0 = *(const f32x4*)d, d1 = *(const f32x4*)(d + 4);
    float f[8];
    unpack_bf16x8(bv[it], f);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float x = i < 4 ? d0[i & 3] : d1[i & 3];
      f[i] = x == 0.f ? f[i] : f[i] + x;      // a zero sum keeps the bits of base (-0 stays -0)
    }
    *(u32x4*)(a.W + (int64_t)(n0 + nw + 8 * it + er) * a.ldw + ek) = pack_bf16x8(f);
  }
}

}  // namespace rtv

using namespace rtv;

extern "C" {

int rtv_lora_merge(const void* base, int ldb, void* W, int ldw, int N, int K, const rtv_lora_adapter* adapters, int count,
                   rtv_stream_t stream) {
  if (!base || !W) return set_error(-1, "lora_merge: null base or W pointer");
  if (N <= 0 || K <= 0) return set_error(-1, "lora_merge: N and K must be positive");
  if (count < 0 || count > RTV_LORA_MAX_ADAPTERS) return set_error(-1, "lora_merge: count outside 0 .. RTV_LORA_MAX_ADAPTERS (4)");
  if (count > 0 && !adapters) return set_error(-1, "lora_merge: null adapter table");
  if (K % 8 || ldb % 8 || ldw % 8) return set_error(-1, "lora_merge: misaligned: K and both strides must be multiples of 8");
  if (ldb < K || ldw < K) return set_error(-1, "lora_merge: row stride below K");
  if (((uintptr_t)base | (uintptr_t)W) & 15) return set_error(-1, "lora_merge: misaligned: base and W must be 16-byte aligned");
  LoraArgs a = {};
  a.base = (const bf16_t*)base, a.W = (bf16_t*)W, a.ldb = ldb, a.ldw = ldw, a.N = N, a.K = K, a.count = count;
  double flop = 0;
  for (int i = 0; i < count; ++i) {
    const rtv_lora_adapter& ad = adapters[i];
    if (!ad.A || !ad.B) return set_error(-1, "lora_merge: null adapter A or B pointer");
    if (ad.rank < 1 || ad.rank > RTV_LORA_MAX_RANK) return set_error(-1, "lora_merge: rank outside 1 .. RTV_LORA_MAX_RANK (256)");
    if (!isfinite(ad.scale)) return set_error(-1, "lora_merge: non-finite scale");
    if ((uintptr_t)ad.A & 15) return set_error(-1, "lora_merge: misaligned: adapter A must be 16-byte aligned");
    if ((uintptr_t)ad.B & 1) return set_error(-1, "lora_merge: misaligned: adapter B must be 2-byte aligned");
    a.A[i] = (const bf16_t*)ad.A, a.B[i] = (const bf16_t*)ad.B, a.rank[i] = ad.rank, a.scale[i] = ad.scale;
    a.b_vec[i] = ad.rank % 8 == 0 && ((uintptr_t)ad.B & 15) == 0;
    flop += 2.0 * N * K * ad.rank;
  }
  a.tiles_k = (K + LM_TK - 1) / LM_TK;
  const int64_t tiles = (int64_t)a.tiles_k * ((N + LM_TN - 1) / LM_TN);
  if (tiles > 0x7fffffff) return set_error(-1, "lora_merge: matrix too large for one launch");
  ProfScope prof(PROF_MISC, (hipStream_t)stream, flop);
  hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("lora_merge");
}

}  // extern "C"
