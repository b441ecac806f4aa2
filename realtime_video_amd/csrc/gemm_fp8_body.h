// The body of the two FP8 (OCP e4m3) projection GEMMs for gfx950: gemm_fp8_kernel (gemm_fp8.hip, one scale per tensor) and
// gemm_fp8_rows_kernel (gemm_fp8_rows.hip, one scale per row).  They differ in the de-quantise step behind the K loop and in
// nothing else, so everything else - tile map, staging, schedule, split-K hand-off, store - is written here once, as a
// force-inlined function template over that step.  Each kernel instantiates it in a translation unit of its own: a second
// instantiation next to gemm8's kernel once cost a neighbouring shape 3.8 %, so never include this header from a file
// that defines another kernel with it.
//
// The GEMM is gemm8.hip's 256x256 ping-pong schedule with one change of unit: a K-tile is 128 fp8 elements, so every
// byte-level quantity (128-byte rows, 16 KiB half-tiles, DMA pieces, swizzle, fragment reads per phase) is identical,
// while each phase issues 4 v_mfma_f32_32x32x64_f8f6f4 (64 cycles, 4x the FLOPs of a 32x32x16 bf16 MFMA) instead of
// 8 bf16 MFMAs: same time per K-tile, twice the work.  Fragment layout (scripts/micro/fp8_mfma.hip): lane l holds row
// l & 31 and the 32 consecutive K bytes 32 * (l >> 5) .. +32 of a 64-deep step = two 16-byte LDS chunks.
#pragma once
#include <string>
#include <type_traits>

#include "gemm_core.h"
#include "gemm_split.h"
#include "rtv_internal.h"

namespace rtv {

namespace gf8 {
constexpr int BM = 256, BN = 256, BK = 128;      // BK in fp8 elements = bytes
constexpr int HALF_ROWS = 128;
constexpr int HALF_BYTES = HALF_ROWS * BK;       // 16 KiB
constexpr int LDS_BYTES = 8 * HALF_BYTES;        // 128 KiB
constexpr int THREADS = 512;

__device__ __forceinline__ int slot_off(int buf, int h) { return (buf * 4 + h) * HALF_BYTES; }
__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

typedef __attribute__((ext_vector_type(8))) int v8i;
typedef __attribute__((ext_vector_type(4))) int v4i;
__device__ __forceinline__ f32x16 mfma_fp8(const v8i& a, const v8i& b, const f32x16& c) {
  // cbsz = blgp = 0: both operands e4m3.  Zero scale operands select the plain v_mfma_f32_32x32x64_f8f6f4 (no block
  // scaling, no scale registers) instead of v_mfma_scale_*.
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0, 0, 0);
}
// one MFMA operand = two 16-byte LDS chunks landing in 8 consecutive registers
__device__ __forceinline__ v8i load_frag(const char* lo, const char* hi) {
  const v4i a = *(const v4i*)lo, b = *(const v4i*)hi;
  return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

// The whole kernel.  Args = the kernel's Fp8Args: f.A, f.W are e4m3 [M][f.lda] and [N][f.ldw], leading dimensions in bytes.
// `dequant(acc, row0, col0)` scales the fp32 sums in place before the shared bf16 epilogue (bias / activation / gate / residual);
// row0 / col0 = this lane's first output row / column.  The MFMAs run with swapped operands (W rows as the MFMA "A": gemm_core.h),
// so in MFMA terms the C/D block is [n][m]: the lane's 32x32 block (mi, ni) holds output row row0 + mi * 32 and, in register r,
// output column col0 + ni * 32 + 8 * (r >> 2) + (r & 3) - what store_tile reads.
template <class Args, class Dequant>
__device__ __forceinline__ void gemm_body(const GemmParams& p, const Args& f, const SplitArgs& sp, Dequant dequant) {
  typedef TileCfg<256, 256, 64, 2, 4> Cfg;  // epilogue geometry: 4 x 2 blocks of 32x32 per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int l31 = lane & 31, g = lane >> 5;

  const int nk_total = p.K / BK;
  int tile_id, seg, unit, kt_begin, kt_end;
  const bool is_split = split_unit_of_block(sp, blockIdx.x, nk_total, &tile_id, &unit, &seg, &kt_begin, &kt_end);
  constexpr int GROUP_M = 8;
  const int per_group = GROUP_M * p.tiles_n;
  const int group = tile_id / per_group;
  const int first_m = group * GROUP_M;
  const int gm = min(p.tiles_m - first_m, GROUP_M);
  const int in_group = tile_id - group * per_group;
  const int m0 = (first_m + in_group % gm) * BM;
  const int n0 = (in_group / gm) * BN;

  // ---- DMA geometry (bytes): a half-tile is 2 wave-wide pieces per wave; piece j of wave w fills rows
  //      j*64 + w*8 .. +8 (lane -> row + lane/8, chunk slot lane%8), source chunk pre-swizzled.
  uint32_t src_off[4][2];
  {
    const int rsub = lane >> 3, cpos = lane & 7;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = j * 64 + wave * 8 + rsub;
      const int ch = swz(row, cpos) * 16;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int gm_row = min(m0 + h * HALF_ROWS + row, p.M - 1);
        const int gn_row = min(n0 + h * HALF_ROWS + row, p.N - 1);
        src_off[h][j] = (uint32_t)gm_row * (uint32_t)f.lda + ch;
        src_off[2 + h][j] = (uint32_t)gn_row * (uint32_t)f.ldw + ch;
      }
    }
  }
  // chk: std::true_type only in the last two K-tiles (gemm8.hip: the steady-state loop stages without bounds checks)
  auto stage_piece = [&](int kt, int h, int j, auto chk) {
    if (decltype(chk)::value && kt >= kt_end) return;
    const uint8_t* base = (h < 2 ? f.A : f.W) + (size_t)kt * BK;
    dma16(base + src_off[h][j], smem + slot_off(kt & 1, h) + (j * 64 + wave * 8) * 128);
  };
  auto stage_half = [&](int kt, int h) {
    stage_piece(kt, h, 0, std::true_type{});
    stage_piece(kt, h, 1, std::true_type{});
  };

  // ---- fragments:
  //      the operand of 64-deep step st = bytes [64 st + 32 g, +32) of the row = LDS chunks 4 st + 2 g and + 1
  const int a_slot = wr;
  const int b_slot = 2 + (wc >> 1);
  const int b_row0 = (wc & 1) * 64;
  v8i af[2][2], bfr[2][2], bnext[2];   // [block][64-deep step]
  auto frag = [&](const char* s, int row, int st) {
    const int c0 = st * 4 + g * 2;
    return load_frag(s + row * 128 + (swz(row, c0) << 4), s + row * 128 + (swz(row, c0 + 1) << 4));
  };
  auto read_a = [&](int buf, int mq) {
    const char* s = smem + slot_off(buf, a_slot);
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int st = 0; st < 2; ++st) af[mb][st] = frag(s, mq * 64 + mb * 32 + l31, st);
  };
  auto read_w = [&](int buf, int nq, v8i (&dst)[2]) {
    const char* s = smem + slot_off(buf, b_slot);
#pragma unroll
    for (int st = 0; st < 2; ++st) dst[st] = frag(s, b_row0 + nq * 32 + l31, st);
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

#define GF_FENCE() __builtin_amdgcn_sched_barrier(0)
#define GF_BARRIER()                  \
  do {                                \
    GF_FENCE();                       \
    __builtin_amdgcn_s_barrier();     \
    GF_FENCE();                       \
  } while (0)
#define GF_PHASE_SYNC()                                 \
  do {                                                  \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  \
    GF_BARRIER();                                       \
  } while (0)

  // MFMA segment of one phase: 4 MFMA 32x32x64 on one 64x32 quadrant, the phase's 2 DMA pieces between them
  auto mma_quadrant = [&](int mq, int nq, int st_kt, int st_h, auto chk) {
    __builtin_amdgcn_s_setprio(1);
    int n = 0;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) {
        acc[mq * 2 + mb][nq] = mfma_fp8(bfr[nq][s], af[mb][s], acc[mq * 2 + mb][nq]);
        ++n;
        if (n == 1 || n == 3) {
          GF_FENCE();
          stage_piece(st_kt, st_h, n == 1 ? 0 : 1, chk);
          GF_FENCE();
        }
      }
    __builtin_amdgcn_s_setprio(0);
  };

  // ---- prologue / K loop: gemm8.hip's schedule (phases, counted vmcnt(2), one-barrier stagger of the wave groups)
  stage_half(kt_begin, 2);
  stage_half(kt_begin, 3);
  stage_half(kt_begin, 0);
  stage_half(kt_begin, 1);
  stage_half(kt_begin + 1, 2);
  stage_half(kt_begin + 1, 3);
  if (kt_begin + 1 < kt_end) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  GF_BARRIER();
  if (wr == 1) GF_BARRIER();
  read_w(kt_begin & 1, 0, bnext);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  GF_FENCE();

  auto k_tile = [&](const int kt, auto chk) {
    constexpr bool CHK = decltype(chk)::value;
    const int buf = kt & 1;
#pragma unroll
    for (int j = 0; j < 2; ++j) bfr[0][j] = bnext[j];
    read_a(buf, 0);
    GF_PHASE_SYNC();
    mma_quadrant(0, 0, kt + 1, 0, chk);
    GF_BARRIER();
    read_w(buf, 1, bfr[1]);
    if (!CHK || kt + 1 < kt_end) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    GF_PHASE_SYNC();
    mma_quadrant(0, 1, kt + 1, 1, chk);
    GF_BARRIER();
    read_a(buf, 1);
    GF_PHASE_SYNC();
    mma_quadrant(1, 1, kt + 2, 2, chk);
    GF_BARRIER();
    if (!CHK || kt + 1 < kt_end) read_w(buf ^ 1, 0, bnext);
    if (!CHK || kt + 2 < kt_end) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    GF_PHASE_SYNC();
    mma_quadrant(1, 0, kt + 2, 3, chk);
    GF_BARRIER();
  };
  int kt = kt_begin;
  for (; kt + 2 < kt_end; ++kt) k_tile(kt, std::false_type{});
  for (; kt < kt_end; ++kt) k_tile(kt, std::true_type{});
  if (wr == 0) GF_BARRIER();
#undef GF_FENCE
#undef GF_BARRIER
#undef GF_PHASE_SYNC

  if (is_split && !split_k_reduce<4>(acc, sp, unit, seg, tile_id, smem, tid, wave, lane)) return;

  dequant(acc, m0 + wr * 128 + l31, n0 + wc * 64 + g * 4);
  const bool wide = !((p.ldc | (p.residual ? p.ldr : 0)) & 7) && !(((uintptr_t)p.C | (uintptr_t)p.residual) & 15);
  if (wide) {
    if (is_split) __syncthreads();
    store_tile_lds<false, 4>(p, m0 + wr * 128, n0 + wc * 64, lane, smem + wave * (128 * 128), acc);   // gemm_core.h
  } else {
    store_tile<false, Cfg>(p, m0 + wr * 128, n0 + wc * 64, lane, acc);
  }
}

// Argument checks and tile counts that the launchers of both kernels share; `who` prefixes the messages.
inline int prepare_launch(GemmParams& p, int lda, int ldw, const char* who) {
  auto fail = [&](const char* what) { return set_error(-1, (std::string(who) + ": " + what).c_str()); };
  if (p.M <= 0 || p.N <= 0 || p.K <= 0) return fail("empty problem");
  if (p.K % BK) return fail("K must be a multiple of 128");
  if (p.N % 8) return fail("N must be a multiple of 8");
  if ((lda % 16) || (ldw % 16) || (p.ldc % 4) || (p.residual && (p.ldr % 4)))
    return fail("leading dimensions must keep 16-byte (A,W) / 8-byte (C,res) alignment");
  if (p.gate && p.rows_per_frame <= 0) return fail("gate needs rows_per_frame");
  p.tiles_m = (p.M + BM - 1) / BM;
  p.tiles_n = (p.N + BN - 1) / BN;
  return 0;
}
}  // namespace gf8

}  // namespace rtv
