// MXFP4 projection GEMM for gfx950 (include/rtv_hip_mxfp4.h): e2m1 codes, one e8m0 scale per 32 elements of K on both operands,
// multiplied by v_mfma_scale_f32_32x32x64_f8f6f4 cbsz:4 blgp:4, which applies 2^(ea + ew) per block inside the MFMA - there is no
// de-quantise step behind the K loop.  The quantisers are in mxfp4.hip.
//
// The schedule is gemm_fp8_body.h's (256x256 tile, 512 threads, four-phase ping-pong, counted vmcnt, one-barrier stagger of the wave
// groups, split-K hand-off of gemm_split.h, store_tile_lds / store_tile) with one change of unit: a K-tile is 256 e2m1 elements, so
// every byte-level quantity (128-byte rows, 16 KiB half-tiles, DMA pieces, swizzle) is the fp8 kernel's, while a phase issues
// 8 MFMAs of 32 cycles where fp8 issues 4 of 64: same time per K-tile, twice the work.  It is a sibling text and not an instantiation
// of that header because the fragment type (4 registers, one LDS chunk), the MFMA count per phase and the scale operands differ in
// the loop itself; gemm_fp8_body.h and its two kernels are untouched.  One kernel per translation unit (a neighbour once
// cost 3.8 %).
//
// Fragment layout (scripts/micro/mxfp4_mfma.hip): in the 64-deep step st of a K-tile lane l holds row l & 31 and block 2 st + g,
// g = l >> 5: 16 bytes = LDS chunk 2 st + g, one ds_read_b128.  The block's scale is byte st of the dword at byte 8 kt + 4 g of the
// row's scales (the header's storage order), selected by the MFMA's opsel.
//
// Scale dwords go from global memory straight to registers, one K-tile ahead: 4 per lane for its 128 activation rows, 2 for its 64
// weight rows.  They are asm loads (hipcc would wait vmcnt(0) at the use of an ordinary load while DMA is in flight), each issued in
// front of the two DMA pieces of some phase, so that the counted vmcnt(2) behind that phase - which leaves only the two newest
// operations in flight - retires it: no count of the DMA discipline changes.  Nothing reads a destination before a statement behind
// that wait names it "+v".  The registers are loaded in place, each where its previous value has been used for the last time (the
// kernel is at the register limit of two waves per SIMD).  What this rests on and cannot state in the source: the compiler takes
// an asm output as written at the asm statement, so a copy or a live-range split of a destination between its load and that "+v"
// statement would read the register before the data has landed.  The code object of the installed compiler has none (the loop keeps
// every destination in one register from load to use), but nothing in the language forbids one: the guard against a compiler that
// starts to make them is the bit-exact GEMM cases of tests/test_mxfp4_gpu.py, whose scales differ from row to row and from block to
// block over one to eight K-tiles - a stale scale register changes their output.
#include <string>
#include <type_traits>

#include "../../include/rtv_hip_mxfp4.h"
#include "gemm_core.h"
#include "gemm_split.h"
#include "rtv_internal.h"

namespace rtv {

namespace gm4 {
constexpr int BM = 256, BN = 256, BK = 128;      // BK in bytes = 256 e2m1 elements
constexpr int BK_ELEMS = 256;
constexpr int HALF_ROWS = 128;
constexpr int HALF_BYTES = HALF_ROWS * BK;       // 16 KiB
constexpr int DUMP_OFF = 8 * HALF_BYTES;         // behind the two tile buffers: where the DMA pieces of K-tiles past the end land
constexpr int LDS_BYTES = DUMP_OFF + 8 * 1024;   // 128 KiB + one 1 KiB piece per wave
constexpr int THREADS = 512;

__device__ __forceinline__ int slot_off(int buf, int h) { return (buf * 4 + h) * HALF_BYTES; }
__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

typedef __attribute__((ext_vector_type(8))) int v8i;
typedef __attribute__((ext_vector_type(4))) int v4i;
// cbsz = blgp = 4: both operands e2m1, 4 registers each (the builtin's type is the 8-register one; the upper half is not read).
// The scale of a lane's block is byte ST of sa / sb.
template <int ST>
__device__ __forceinline__ f32x16 mfma_mx(const v4i& a, const v4i& b, const f32x16& c, int sa, int sb) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(__builtin_shufflevector(a, a, 0, 1, 2, 3, -1, -1, -1, -1),
                                                         __builtin_shufflevector(b, b, 0, 1, 2, 3, -1, -1, -1, -1), c, 4, 4, ST, sa, ST, sb);
}

struct Args {
  const uint8_t* A;          // [M][lda] bytes of codes
  const uint8_t* W;          // [N][ldw]
  int lda, ldw;              // bytes
  const uint8_t* a_scales;   // [M][K / 32]
  const uint8_t* w_scales;   // [N][K / 32]
};
}  // namespace gm4

// The MFMAs run with swapped operands (W rows as the MFMA "A": gemm_core.h), so in MFMA terms the C/D block is [n][m]: the lane's
// 32x32 block (mi, ni) holds output row row0 + mi * 32 and, in register r, output column col0 + ni * 32 + 8 * (r >> 2) + (r & 3).
__global__ __launch_bounds__(gm4::THREADS, 2) void gemm_mxfp4_kernel(GemmParams p, gm4::Args f, SplitArgs sp) {
  using namespace gm4;
  typedef TileCfg<256, 256, 64, 2, 4> Cfg;  // epilogue geometry: 4 x 2 blocks of 32x32 per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int l31 = lane & 31, g = lane >> 5;

  const int nk_total = p.K / BK_ELEMS;
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
  // The K loop is free of branches: a piece of a K-tile past the end of this block's range is not skipped but read again from the
  // last tile and written to a dump area nothing reads (with branches around the pieces the register allocator spilled
  // accumulators).  So every count of the vmcnt discipline holds in every tile, the last ones included, and one vmcnt(0) behind
  // the loop retires what is left.
  auto stage_piece = [&](int kt, int h, int j) {
    const bool live = kt < kt_end;
    const uint8_t* base = (h < 2 ? f.A : f.W) + (size_t)min(kt, kt_end - 1) * BK;
    // (the lane's 32-bit offset is made opaque at each use: the compiler otherwise keeps its eight 64-bit extensions in registers
    // across the loop; as it is, base + offset selects the scalar-base form of the DMA and costs no register)
    uint32_t off = src_off[h][j];
    asm volatile("" : "+v"(off));
    dma16(base + off, smem + (live ? slot_off(kt & 1, h) + (j * 64 + wave * 8) * 128 : DUMP_OFF + wave * 1024));
  };
  auto stage_half = [&](int kt, int h) {
    stage_piece(kt, h, 0);
    stage_piece(kt, h, 1);
  };

  // ---- block scales: byte offsets of this lane's dwords inside a K-tile's 8 bytes of its 4 activation rows and 2 weight rows
  //      (rows past the edge are clamped into the arrays: their results are never stored)
  const uint32_t srow = (uint32_t)(p.K / RTV_MXFP4_BLOCK);
  uint32_t sa_off[4], sw_off[2];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) sa_off[mi] = (uint32_t)min(m0 + wr * 128 + mi * 32 + l31, p.M - 1) * srow + g * 4;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) sw_off[ni] = (uint32_t)min(n0 + wc * 64 + ni * 32 + l31, p.N - 1) * srow + g * 4;
  // Eight registers.  The activation scales are loaded in place where a pair is free; a weight scale is in use from phase 3 (sw[0])
  // or phase 1 (sw[1]) of a tile into the next tile, so the next tile's pair goes to sw_next and is copied behind phase 3:
  //   sa[2..3] (rows of quadrants (1, *): phases 2, 3)  this tile's at the top of the tile, retired by the wait behind phase 0
  //   sw_next                                            next tile's at the top of the tile, retired by the same wait
  //   sa[0..1] (rows of quadrants (0, *): phases 0, 1)  next tile's at the top of phase 2, retired by the wait in front of phase 3
  // Every load of a tile is retired inside that tile.  In the last tile "next" is the tile itself: a load more, a branch less.
  int sa[4], sw[2], sw_next[2];
  auto load_scale = [&](int& dst, uint32_t off, const uint8_t* base, int kt) {   // one load, counted by hand
    const uint8_t* b = base + (size_t)kt * 8;
    asm volatile("global_load_dword %0, %1, %2" : "=v"(dst) : "v"(off), "s"(b) : "memory");
  };
  // behind a counted wait that has retired the loads of these registers: nothing reads them before this statement
#define GM_TAKE2(x, y) asm volatile("" : "+v"(x), "+v"(y))

  // ---- fragments: the operand of 64-deep step st = bytes [32 st + 16 g, +16) of the row = LDS chunk 2 st + g
  const int a_slot = wr;
  const int b_slot = 2 + (wc >> 1);
  const int b_row0 = (wc & 1) * 64;
  // bfr: two sets of W fragments that change roles from one K-tile to the next (`par`, below): a third set to prefetch into, as the
  // fp8 kernel has, does not fit beside the scale registers
  v4i af[2][4], bfr[2][4];   // [block][64-deep step]
  auto frag = [&](const char* s, int row, int st) { return *(const v4i*)(s + row * 128 + (swz(row, st * 2 + g) << 4)); };
  auto read_a = [&](int buf, int mq) {
    const char* s = smem + slot_off(buf, a_slot);
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int st = 0; st < 4; ++st) af[mb][st] = frag(s, mq * 64 + mb * 32 + l31, st);
  };
  auto read_w = [&](int buf, int nq, v4i (&dst)[4]) {
    const char* s = smem + slot_off(buf, b_slot);
#pragma unroll
    for (int st = 0; st < 4; ++st) dst[st] = frag(s, b_row0 + nq * 32 + l31, st);
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

#define GM_FENCE() __builtin_amdgcn_sched_barrier(0)
#define GM_BARRIER()                  \
  do {                                \
    GM_FENCE();                       \
    __builtin_amdgcn_s_barrier();     \
    GM_FENCE();                       \
  } while (0)
#define GM_PHASE_SYNC()                                 \
  do {                                                  \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  \
    GM_BARRIER();                                       \
  } while (0)

  // MFMA segment of one phase: 8 MFMA 32x32x64 on one 64x32 quadrant, the phase's 2 DMA pieces behind the 2nd and the 6th (where
  // the fp8 kernel has them in time: behind 64 and 192 of 256 MFMA cycles)
  auto mma_quadrant = [&](int mq, int nq, int wset, int st_kt, int st_h) {
    __builtin_amdgcn_s_setprio(1);
    auto step = [&](auto ST) {
      constexpr int s = decltype(ST)::value;
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
        acc[mq * 2 + mb][nq] = mfma_mx<s>(bfr[wset][s], af[mb][s], acc[mq * 2 + mb][nq], sw[nq], sa[mq * 2 + mb]);
      if (s == 0 || s == 2) {
        GM_FENCE();
        stage_piece(st_kt, st_h, s == 0 ? 0 : 1);
        GM_FENCE();
      }
    };
    step(std::integral_constant<int, 0>{});
    step(std::integral_constant<int, 1>{});
    step(std::integral_constant<int, 2>{});
    step(std::integral_constant<int, 3>{});
    __builtin_amdgcn_s_setprio(0);
  };

  // ---- prologue / K loop: gemm_fp8_body.h's schedule (phases, counted vmcnt(2), one-barrier stagger of the wave groups); the
  //      first tile's scales are the oldest loads in flight, so the prologue's wait retires them
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) load_scale(sa[mi], sa_off[mi], f.a_scales, kt_begin);
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) load_scale(sw[ni], sw_off[ni], f.w_scales, kt_begin);
  stage_half(kt_begin, 2);
  stage_half(kt_begin, 3);
  stage_half(kt_begin, 0);
  stage_half(kt_begin, 1);
  stage_half(kt_begin + 1, 2);
  stage_half(kt_begin + 1, 3);
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  GM_TAKE2(sa[0], sa[1]);
  GM_TAKE2(sw[0], sw[1]);
  GM_BARRIER();
  if (wr == 1) GM_BARRIER();
  read_w(kt_begin & 1, 0, bfr[0]);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  GM_FENCE();

  // par = parity of the tile counted from kt_begin: the W fragments of quadrant column 0 are in bfr[par] (read in phase 3 of the
  // previous tile, or by the prologue), those of column 1 go to bfr[1 - par], which the previous tile used last in its phase 3;
  // phase 3 reads the next tile's column 0 into bfr[1 - par], free since phase 2 (behind the last tile: whatever the buffer holds)
  auto k_tile = [&](const int kt, auto par) {
    constexpr int W0 = decltype(par)::value, W1 = 1 - W0;
    const int buf = kt & 1;
    const int kt_next = min(kt + 1, kt_end - 1);   // in the last tile "next" is the tile itself: a load more, a branch less
    load_scale(sa[2], sa_off[2], f.a_scales, kt);
    load_scale(sa[3], sa_off[3], f.a_scales, kt);
    load_scale(sw_next[0], sw_off[0], f.w_scales, kt_next);
    load_scale(sw_next[1], sw_off[1], f.w_scales, kt_next);
    GM_FENCE();
    read_a(buf, 0);
    GM_PHASE_SYNC();
    mma_quadrant(0, 0, W0, kt + 1, 0);
    GM_BARRIER();
    read_w(buf, 1, bfr[W1]);
    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");   // leaves phase 0's two pieces in flight; the scale loads of the tile top are older
    GM_TAKE2(sa[2], sa[3]);
    GM_TAKE2(sw_next[0], sw_next[1]);
    GM_PHASE_SYNC();
    mma_quadrant(0, 1, W1, kt + 1, 1);
    GM_BARRIER();
    load_scale(sa[0], sa_off[0], f.a_scales, kt_next);
    load_scale(sa[1], sa_off[1], f.a_scales, kt_next);
    GM_FENCE();
    read_a(buf, 1);
    GM_PHASE_SYNC();
    mma_quadrant(1, 1, W1, kt + 2, 2);
    GM_BARRIER();
    read_w(buf ^ 1, 0, bfr[W1]);
    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");   // leaves phase 2's two pieces in flight: the loads of sa[0..1] are older
    GM_TAKE2(sa[0], sa[1]);
    GM_PHASE_SYNC();
    mma_quadrant(1, 0, W0, kt + 2, 3);
    GM_FENCE();
    sw[0] = sw_next[0];
    sw[1] = sw_next[1];
    GM_BARRIER();
  };
  for (int kt = kt_begin; kt < kt_end; kt += 2) {
    k_tile(kt, std::integral_constant<int, 0>{});
    if (kt + 1 >= kt_end) break;
    k_tile(kt + 1, std::integral_constant<int, 1>{});
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the pieces of the last phases (dump area, or nothing)
  if (wr == 0) GM_BARRIER();
#undef GM_FENCE
#undef GM_BARRIER
#undef GM_PHASE_SYNC
#undef GM_TAKE2

  if (is_split && !split_k_reduce<4>(acc, sp, unit, seg, tile_id, smem, tid, wave, lane)) return;

  const bool wide = !((p.ldc | (p.residual ? p.ldr : 0)) & 7) && !(((uintptr_t)p.C | (uintptr_t)p.residual) & 15);
  if (wide) {
    if (is_split) __syncthreads();
    store_tile_lds<false, 4>(p, m0 + wr * 128, n0 + wc * 64, lane, smem + wave * (128 * 128), acc);   // gemm_core.h
  } else {
    store_tile<false, Cfg>(p, m0 + wr * 128, n0 + wc * 64, lane, acc);
  }
}

static int launch_gemm_mxfp4(GemmParams p, const gm4::Args& f, hipStream_t stream) {
  auto fail = [&](const char* what) { return set_error(-1, (std::string("gemm_mxfp4: ") + what).c_str()); };
  if (p.M <= 0 || p.N <= 0 || p.K <= 0) return fail("empty problem");
  if (p.K % gm4::BK_ELEMS) return fail("K must be a multiple of 256");
  if (p.N % 8) return fail("N must be a multiple of 8");
  if ((f.lda % 16) || (f.ldw % 16) || f.lda < p.K / 2 || f.ldw < p.K / 2 || (p.ldc % 4) || (p.residual && (p.ldr % 4)))
    return fail("leading dimensions must be >= K / 2 bytes and keep 16-byte (A,W) / 8-byte (C,res) alignment");
  if (((uintptr_t)f.A & 15) || ((uintptr_t)f.W & 15)) return fail("A_codes and W_codes must be 16-byte aligned");
  if (((uintptr_t)f.a_scales & 3) || ((uintptr_t)f.w_scales & 3)) return fail("a_scales and w_scales must be 4-byte aligned");
  // the kernel addresses codes and scales with 32-bit offsets from the operand bases
  if ((uint64_t)p.M * (uint64_t)f.lda >= (1ull << 32) || (uint64_t)p.N * (uint64_t)f.ldw >= (1ull << 32)) return fail("operand larger than 4 GiB");
  if (p.gate && p.rows_per_frame <= 0) return fail("gate needs rows_per_frame");
  p.tiles_m = (p.M + gm4::BM - 1) / gm4::BM;
  p.tiles_n = (p.N + gm4::BN - 1) / gm4::BN;
  static LdsAttr lds_attr;   // per device (a second GPU used from this process needs the attribute as well)
  if (int st = ensure_dynamic_lds((const void*)gemm_mxfp4_kernel, gm4::LDS_BYTES, &lds_attr, "gemm_mxfp4")) return st;
  SplitArgs sp;
  int grid = 0;
  if (int st = plan_split_k(p.tiles_m * p.tiles_n, p.K / gm4::BK_ELEMS, true, &sp, &grid, stream)) return st;
  ProfScope prof(PROF_GEMM, stream, 2.0 * p.M * (double)p.N * p.K);
  note_kernel(DK_GEMM_MXFP4_256x256);
  hipLaunchKernelGGL(gemm_mxfp4_kernel, dim3(grid), dim3(gm4::THREADS), gm4::LDS_BYTES, stream, p, f, sp);
  return check_launch("gemm_mxfp4");
}

}  // namespace rtv

using namespace rtv;

extern "C" int rtv_gemm_mxfp4(const void* A_codes, int lda, const void* W_codes, int ldw, const void* a_scales, const void* w_scales,
                              void* C, int ldc, int M, int N, int K, const void* bias, int act, const void* gate, int gate_stride,
                              int rows_per_frame, int row_offset, const void* residual, int ldr, rtv_stream_t stream) {
  if (!A_codes || !W_codes || !C || !a_scales || !w_scales) return set_error(-1, "gemm_mxfp4: null pointer");
  const GemmParams p = gemm_params(nullptr, lda, nullptr, ldw, C, ldc, M, N, K, bias, act, gate, gate_stride, rows_per_frame, row_offset,
                                   residual, ldr);
  const gm4::Args f{(const uint8_t*)A_codes, (const uint8_t*)W_codes, lda, ldw, (const uint8_t*)a_scales, (const uint8_t*)w_scales};
  return launch_gemm_mxfp4(p, f, (hipStream_t)stream);
}
