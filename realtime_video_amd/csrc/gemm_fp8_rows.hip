// FP8 (OCP e4m3) projection GEMM with PER-ROW scales for gfx950 (include/rtv_hip_fp8_rows.h; torchao's PerRow granularity
// restated): y[m, n] = bf16( (q(x) . q(W)^T)[m, n] * s_x[m] * s_w[n] + bias[n] ), one scale per activation row and one per
// weight row (output channel); the quantisers are in fp8_rows.hip.
//
// The kernel is gemm_fp8.hip's gemm_fp8_kernel - same tiling, staging, schedule and split-K - with one change, in the de-quantise
// step behind the K loop: each accumulator is multiplied by s_x[row] and s_w[column] instead of one scalar.  It is a COPY in a
// translation unit of its own, not a second instantiation of a shared body: a new instantiation next to gemm8's kernel once cost a
// neighbouring shape 3.8 %, and the per-tensor kernel's code must stay what it was
// (profiles/r13_fp8_rows_isa_identity.txt).  Read gemm_fp8.hip for the schedule; only the epilogue is commented here.
#include <type_traits>

#include "gemm_core.h"
#include "gemm_split.h"
#include "rtv_internal.h"

namespace rtv {

namespace gf8r {
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

struct Fp8Args {
  const uint8_t* A;      // [M][lda] e4m3
  const uint8_t* W;      // [N][ldw] e4m3
  int lda, ldw;          // bytes
  const float* a_scales;  // [M] device: s_x per row of this call (written by the quantisation kernel)
  const float* w_scales;  // [N] device: s_w per weight row = output column (16-byte aligned)
};
}  // namespace gf8r

__global__ __launch_bounds__(gf8r::THREADS, 2) void gemm_fp8_rows_kernel(GemmParams p, gf8r::Fp8Args f, SplitArgs sp) {
  using namespace gf8r;
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

  // de-quantise: (q(x) . q(W)^T)[m, n] * s_x[m] * s_w[n], then the shared bf16 epilogue (bias / activation / gate / residual).
  // The MFMAs run with swapped operands (W rows as the MFMA "A": gemm_core.h), so in MFMA terms the C/D block is [n][m]: this
  // lane's 32x32 block (mi, ni) holds output row m = mi * 32 + (lane & 31) and, in register r, output column
  // n = ni * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3) - what store_tile reads.  Rows >= M and columns >= N of edge tiles are
  // never stored; their scale reads are clamped into the arrays (N % 8 == 0, so a quad of columns is inside or outside as a whole).
  // Two multiplications per element, not one by a product: the compiler sinks this step into the six epilogue branches below, and
  // what stays live across them is then the 4 + 32 scales of a lane instead of their 128 products (which spilled).
  {
    const int mb = m0 + wr * 128 + l31, nb = n0 + wc * 64 + g * 4;
    float sx[4];
    f32x4 sw[2][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) sx[mi] = f.a_scales[min(mb + mi * 32, p.M - 1)];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) sw[ni][rq] = *(const f32x4*)(f.w_scales + min(nb + ni * 32 + rq * 8, p.N - 4));
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] = acc[mi][ni][r] * sx[mi] * sw[ni][r >> 2][r & 3];
  }
  const bool wide = !((p.ldc | (p.residual ? p.ldr : 0)) & 7) && !(((uintptr_t)p.C | (uintptr_t)p.residual) & 15);
  if (wide) {
    if (is_split) __syncthreads();
    store_tile_lds<false, 4>(p, m0 + wr * 128, n0 + wc * 64, lane, smem + wave * (128 * 128), acc);   // gemm_core.h
  } else {
    store_tile<false, Cfg>(p, m0 + wr * 128, n0 + wc * 64, lane, acc);
  }
}

int launch_gemm_fp8_rows(GemmParams p, const uint8_t* A, int lda, const uint8_t* W, int ldw, const float* a_scales,
                         const float* w_scales, hipStream_t stream) {
  if (p.M <= 0 || p.N <= 0 || p.K <= 0) return set_error(-1, "gemm_fp8_rows: empty problem");
  if (p.K % gf8r::BK) return set_error(-1, "gemm_fp8_rows: K must be a multiple of 128");
  if (p.N % 8) return set_error(-1, "gemm_fp8_rows: N must be a multiple of 8");
  if ((lda % 16) || (ldw % 16) || (p.ldc % 4) || (p.residual && (p.ldr % 4)))
    return set_error(-1, "gemm_fp8_rows: leading dimensions must keep 16-byte (A,W) / 8-byte (C,res) alignment");
  if (((uintptr_t)a_scales & 3) || ((uintptr_t)w_scales & 15))
    return set_error(-1, "gemm_fp8_rows: a_row_scales must be 4-byte aligned, w_row_scales 16-byte aligned");
  if (p.gate && p.rows_per_frame <= 0) return set_error(-1, "gemm_fp8_rows: gate needs rows_per_frame");
  p.tiles_m = (p.M + gf8r::BM - 1) / gf8r::BM;
  p.tiles_n = (p.N + gf8r::BN - 1) / gf8r::BN;
  static LdsAttr lds_attr;   // per device (a second GPU used from this process needs the attribute as well)
  if (int st = ensure_dynamic_lds((const void*)gemm_fp8_rows_kernel, gf8r::LDS_BYTES, &lds_attr, "gemm_fp8_rows")) return st;
  SplitArgs sp;
  int grid = 0;
  if (int st = plan_split_k(p.tiles_m * p.tiles_n, p.K / gf8r::BK, true, &sp, &grid, stream)) return st;
  gf8r::Fp8Args f{A, W, lda, ldw, a_scales, w_scales};
  ProfScope prof(PROF_GEMM, stream, 2.0 * p.M * (double)p.N * p.K);
  note_kernel(DK_GEMM_FP8_256x256);
  hipLaunchKernelGGL(gemm_fp8_rows_kernel, dim3(grid), dim3(gf8r::THREADS), gf8r::LDS_BYTES, stream, p, f, sp);
  return check_launch("gemm_fp8_rows");
}

}  // namespace rtv

using namespace rtv;

extern "C" int rtv_gemm_fp8_rows(const void* A, int lda, const void* W, int ldw, const float* a_row_scales,
                                 const float* w_row_scales, void* C, int ldc, int M, int N, int K, const void* bias, int act,
                                 const void* gate, int gate_stride, int rows_per_frame, int row_offset, const void* residual,
                                 int ldr, rtv_stream_t stream) {
  if (!A || !W || !C || !a_row_scales || !w_row_scales) return set_error(-1, "gemm_fp8_rows: null pointer");
  GemmParams p;
  p.A = nullptr;
  p.W = nullptr;
  p.C = (uint16_t*)C;
  p.lda = lda;
  p.ldw = ldw;
  p.ldc = ldc;
  p.M = M;
  p.N = N;
  p.K = K;
  p.bias = (const uint16_t*)bias;
  p.act = act;
  p.gate = (const uint16_t*)gate;
  p.gate_stride = gate_stride;
  p.rows_per_frame = rows_per_frame;
  p.row_offset = row_offset;
  p.residual = (const uint16_t*)residual;
  p.ldr = ldr;
  p.tiles_m = p.tiles_n = 0;
  return launch_gemm_fp8_rows(p, (const uint8_t*)A, lda, (const uint8_t*)W, ldw, a_row_scales, w_row_scales, (hipStream_t)stream);
}
