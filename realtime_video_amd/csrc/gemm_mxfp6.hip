// MXFP6 projection GEMM for gfx950 (include/rtv_hip_mxfp6.h): e2m3 codes, one e8m0 scale per 32 elements of K on both operands,
// multiplied by v_mfma_scale_f32_32x32x64_f8f6f4 cbsz:2 blgp:2, which applies 2^(ea + ew) per block inside the MFMA - there is no
// de-quantise step behind the K loop.  The quantisers are in mxfp6.hip.
//
// The schedule is gemm_mxfp4.hip's (256x256 tile, 512 threads, four-phase ping-pong, counted vmcnt, one-barrier stagger of the wave
// groups, split-K hand-off of gemm_split.h, store_tile_lds / store_tile, branch-free K loop with a dump area).  What differs is
// the operand geometry, because a 32-element block is 24 bytes, and the way the scales come in:
//
// LDS budget.  A K-tile is 128 elements = 96 bytes of a row = two 64-deep MFMA steps (a 256-element tile would be 96 KiB per buffer,
//   and two do not fit 160 KiB).  An operand's tile is 256 rows x 96 bytes = 24 KiB, linear; two buffers of two operands are 96 KiB.
//   The epilogue image needs 128 KiB, the dump area sits behind that, as in the sibling, and two buffers of scales behind it: 140 KiB.
//   A phase issues 4 MFMAs; the fragments are 2 x (2 x 2 + 2 x 2) x 6 = 48 registers.
// DMA.  global_load_lds writes wave base + lane * 16 linearly, and a 1 KiB piece is 10 2/3 rows, so a piece does not cover whole
//   rows: LDS stays linear and the map is on the source side.  Chunk ci = 64 * piece + lane of an operand tile is (row ci / 6, slot
//   ci % 6); a lane fetches the 16 source bytes that belong there.  An operand tile is 24 pieces, 3 per wave (piece i of wave w is
//   8 i + w); A's go out in phases 0 (two) and 1 (one), W's in phases 2 (two) and 3 (one), so both counted waits stay vmcnt(2) and
//   every piece has the place in time that the sibling's halves have (A one tile ahead, W two).  Rows past the edge are clamped
//   into the arrays, K-tiles past the end re-read the last one into the dump area: no lane forms an address outside an operand.
// Fragment reads.  Lane l holds row l & 31 and block 2 st + g, g = l >> 5, of step st: 24 bytes at 8-byte alignment, read with three
//   ds_read_b64 (a ds_read_b128 would be misaligned for odd blocks, and both lane halves run one instruction).  ds_read_b64 serves a
//   32-lane half at a time over 64 banks = 32 eight-byte positions; the 32 rows of a half-wave read the same 8-byte unit of their
//   rows.  Linear 96-byte rows put row r at position 12 r mod 32: eight values, 4-way conflicts.  The source-side swizzle stores
//   chunk c of row r in slot c ^ ((r >> 3) & 1): rows r and r + 8 then differ by 2 positions and the half-wave covers 16 positions
//   twice (rows r and r + 16 meet).  That 2-way conflict is what is left, and it is the floor of this image: a DMA places 16-byte
//   chunks, so the half of a chunk that a unit sits in is the same in every row, and reads of one unit reach only every other
//   position.
//
// Scales go through LDS too: a K-tile's 4 scale bytes of the tile's 512 rows are 2 KiB, fetched by one 4-byte DMA per wave (lane =
// row) one K-tile ahead, issued in front of the two DMA pieces of phase 0 so that the counted vmcnt(2) behind that phase retires it;
// a lane then reads one 16-bit word per row (the header's order: byte st of the word at byte 2 g of the row's 4, selected by the
// MFMA's opsel).  The sibling loads scales straight to registers; with this K-tile that would be twelve 64-line loads per wave and
// 256 elements of K, and the counters showed the address path, not the MFMA, to be what the loop waits for.
#include <string>
#include <type_traits>

#include "../../include/rtv_hip_mxfp6.h"
#include "gemm_core.h"
#include "gemm_split.h"
#include "rtv_internal.h"

namespace rtv {

namespace gm6 {
constexpr int BM = 256, BN = 256;
constexpr int BK_ELEMS = 128;
constexpr int BK = BK_ELEMS / 4 * 3;             // 96 bytes of a row
constexpr int OP_BYTES = 256 * BK;               // 24 KiB: one operand's rows of a K-tile, linear
constexpr int EPI_BYTES = 8 * 128 * 128;         // store_tile_lds: 16 KiB per wave
constexpr int DUMP_OFF = EPI_BYTES;              // behind everything else: where the DMA pieces of K-tiles past the end land
constexpr int SCALE_OFF = DUMP_OFF + 8 * 1024;   // behind the dump area (one 1 KiB piece per wave): two buffers of block scales,
constexpr int SCALE_BYTES = 512 * 4;             // a K-tile's 4 bytes for each of the tile's 512 rows
constexpr int LDS_BYTES = SCALE_OFF + 2 * SCALE_BYTES;   // 140 KiB
constexpr int THREADS = 512;
static_assert(4 * OP_BYTES <= EPI_BYTES, "two buffers of two operands must end in front of the dump area");

__device__ __forceinline__ int slot_off(int buf, int op) { return (buf * 2 + op) * OP_BYTES; }
// slot of 16-byte chunk `chunk` (0..5) inside the 96 bytes of row `row` (an involution)
__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 3) & 1); }

typedef __attribute__((ext_vector_type(8))) int v8i;
typedef __attribute__((ext_vector_type(2))) int v2i;
struct Frag {   // a block: 24 bytes = operand registers 0-5
  v2i u[3];
};
// cbsz = blgp = 2: both operands e2m3, 6 registers each (the builtin's type is the 8-register one; the upper two are not read).
// The scale of a lane's block is byte ST of sa / sb.
template <int ST>
__device__ __forceinline__ f32x16 mfma_mx(const Frag& a, const Frag& b, const f32x16& c, int sa, int sb) {
  const v8i av = {a.u[0][0], a.u[0][1], a.u[1][0], a.u[1][1], a.u[2][0], a.u[2][1], 0, 0};
  const v8i bv = {b.u[0][0], b.u[0][1], b.u[1][0], b.u[1][1], b.u[2][0], b.u[2][1], 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, c, 2, 2, ST, sa, ST, sb);
}

// The three 8-byte reads of a block: addresses b[u] + OFF.  (asm reads: the compiler pairs ordinary 8-byte reads of two row blocks
// into ds_read2st64_b64, which is banked over 128 bytes and runs at half the rate, and then moves the halves apart.  Every read is
// followed by an explicit lgkmcnt(0) in front of the first use of its destination: GM_PHASE_SYNC, or the prologue's wait.)
template <int OFF>
__device__ __forceinline__ void read_frag(Frag& r, const uint32_t (&b)[3]) {
  static_assert(OFF >= 0 && OFF < 65536, "ds offset field");
#pragma unroll
  for (int u = 0; u < 3; ++u) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(r.u[u]) : "v"(b[u]), "n"(OFF) : "memory");
}

// A lane's scales of a K-tile: the 16-bit word at byte 2 g of its row's 4 bytes, for its 4 activation rows (32 rows apart) and its 2
// weight rows.  (asm reads, as the fragments: waited for by the GM_PHASE_SYNC that follows.)
template <int OFF>
__device__ __forceinline__ void read_scale_words(int (&sa)[4], int (&sw)[2], uint32_t sa_base, uint32_t sw_base) {
  asm volatile("ds_read_u16 %0, %1 offset:%2" : "=v"(sa[0]) : "v"(sa_base), "n"(OFF) : "memory");
  asm volatile("ds_read_u16 %0, %1 offset:%2" : "=v"(sa[1]) : "v"(sa_base), "n"(OFF + 32 * 4) : "memory");
  asm volatile("ds_read_u16 %0, %1 offset:%2" : "=v"(sa[2]) : "v"(sa_base), "n"(OFF + 64 * 4) : "memory");
  asm volatile("ds_read_u16 %0, %1 offset:%2" : "=v"(sa[3]) : "v"(sa_base), "n"(OFF + 96 * 4) : "memory");
  asm volatile("ds_read_u16 %0, %1 offset:%2" : "=v"(sw[0]) : "v"(sw_base), "n"(OFF) : "memory");
  asm volatile("ds_read_u16 %0, %1 offset:%2" : "=v"(sw[1]) : "v"(sw_base), "n"(OFF + 32 * 4) : "memory");
}

struct Args {
  const uint8_t* A;          // [M][lda] bytes of codes
  const uint8_t* W;          // [N][ldw]
  int lda, ldw;              // bytes
  const uint8_t* a_scales;   // [M][K / 32]
  const uint8_t* w_scales;   // [N][K / 32]
};
}  // namespace gm6

// The MFMAs run with swapped operands (W rows as the MFMA "A": gemm_core.h), so in MFMA terms the C/D block is [n][m]: the lane's
// 32x32 block (mi, ni) holds output row row0 + mi * 32 and, in register r, output column col0 + ni * 32 + 8 * (r >> 2) + (r & 3).
__global__ __launch_bounds__(gm6::THREADS, 2) void gemm_mxfp6_kernel(GemmParams p, gm6::Args f, SplitArgs sp) {
  using namespace gm6;
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

  // ---- DMA geometry: piece i of wave w fills bytes [(8 i + w) * 1024, + 1024) of an operand tile; this lane's 16 bytes there are
  //      slot ci % 6 of row ci / 6, ci = (8 i + w) * 64 + lane, and hold source chunk swz(row, slot) of that row
  uint32_t src_off[2][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int ci = (i * 8 + wave) * 64 + lane;
    const int row = ci / 6, slot = ci - row * 6;   // row < 256
    const int ch = swz(row, slot) * 16;
    src_off[0][i] = (uint32_t)min(m0 + row, p.M - 1) * (uint32_t)f.lda + ch;
    src_off[1][i] = (uint32_t)min(n0 + row, p.N - 1) * (uint32_t)f.ldw + ch;
  }
  // The K loop is free of branches: a piece of a K-tile past the end of this block's range is not skipped but read again from the
  // last tile and written to a dump area nothing reads.  So every count of the vmcnt discipline holds in every tile, the last ones
  // included, and one vmcnt(0) behind the loop retires what is left.
  auto stage_piece = [&](int kt, int op, int i) {
    const int live = -(int)(kt < kt_end);   // all ones / zero: the destination is selected by arithmetic, the loop keeps one basic block
    const uint8_t* base = (op == 0 ? f.A : f.W) + (size_t)min(kt, kt_end - 1) * BK;
    // (the lane's 32-bit offset is made opaque at each use, as in the sibling: base + offset selects the scalar-base form of the DMA)
    uint32_t off = src_off[op][i];
    asm volatile("" : "+v"(off));
    const int dump = DUMP_OFF + wave * 1024;
    dma16(base + off, smem + dump + (live & (slot_off((kt - kt_begin) & 1, op) + (i * 8 + wave) * 1024 - dump)));
  };
  auto stage_op = [&](int kt, int op) {
    stage_piece(kt, op, 0);
    stage_piece(kt, op, 1);
    stage_piece(kt, op, 2);
  };

  // ---- block scales, through LDS: a K-tile's scales are 4 bytes per row, 2 KiB for the 512 rows of the tile (A's 256, then W's);
  //      wave w fetches the 64 rows 64 w .. + 64 with ONE 4-byte DMA (lane = row), one K-tile ahead, into the buffer of that tile's
  //      parity.  (Loaded straight to registers, as the sibling does, each wave issues 6 loads per K-tile whose 64 lanes touch 64
  //      different lines - twelve such loads per 256 elements of K with this K-tile; this is one per wave and K-tile.)  The piece is
  //      issued in front of the two DMA pieces of phase 0, so the counted vmcnt(2) behind that phase retires it, and the barriers of
  //      the tile make it visible before the next tile reads it.  Rows past the edge are clamped into the arrays.
  const uint32_t srow = (uint32_t)(p.K / RTV_MXFP6_BLOCK);
  const int sc_row = wave * 64 + lane;   // row of the 512: waves 0-3 hold A's, 4-7 W's
  const uint32_t sc_src = wave < 4 ? (uint32_t)min(m0 + sc_row, p.M - 1) * srow : (uint32_t)min(n0 + sc_row - 256, p.N - 1) * srow;
  auto stage_scales = [&](int kt) {
    const int live = -(int)(kt < kt_end);
    const uint8_t* base = (wave < 4 ? f.a_scales : f.w_scales) + (size_t)min(kt, kt_end - 1) * 4;
    uint32_t off = sc_src;
    asm volatile("" : "+v"(off));
    const int dump = DUMP_OFF + wave * 1024;
    __builtin_amdgcn_global_load_lds((const RTV_GLOBAL void*)(base + off),
                                     (RTV_LDS void*)(smem + dump + (live & (SCALE_OFF + ((kt - kt_begin) & 1) * SCALE_BYTES + wave * 256 - dump))), 4,
                                     0, 0);
  };
  // a lane's scales of a tile: the 16-bit word at byte 2 g of its row's 4 (the header's order: byte st of it is block 2 st + g)
  int sa[4], sw[2];

  // ---- fragments: block 2 st + g of the row = its 8-byte units 3 (2 st + g) + u, u = 0..2; unit U is half U & 1 of chunk U >> 1.
  //      swz depends on bit 3 of the row only and every row base is a multiple of 32, so a lane has six offsets per operand (its
  //      wave's rows included); buffer, quadrant and row block are immediates of the reads.
  uint32_t a_base[2][3], w_base[2][3], sa_base, sw_base;
  {
    const uint32_t lds0 = (uint32_t)(uintptr_t)(RTV_LDS const char*)smem;
    sa_base = lds0 + SCALE_OFF + (wr * 128 + l31) * 4 + g * 2;
    sw_base = lds0 + SCALE_OFF + (256 + wc * 64 + l31) * 4 + g * 2;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int U = 3 * (2 * st + g) + u;
        const uint32_t off = lds0 + l31 * BK + swz(l31, U >> 1) * 16 + (U & 1) * 8;
        a_base[st][u] = off + wr * 128 * BK;
        w_base[st][u] = off + OP_BYTES + wc * 64 * BK;
      }
  }
  // bfr: two sets of W fragments that change roles from one K-tile to the next (`par`, below)
  Frag af[2][2], bfr[2][2];   // [block][64-deep step]
  auto read_a = [&](auto buf, auto mq) {
    constexpr int OFF = decltype(buf)::value * 2 * OP_BYTES + decltype(mq)::value * 64 * BK;
    read_frag<OFF>(af[0][0], a_base[0]);
    read_frag<OFF>(af[0][1], a_base[1]);
    read_frag<OFF + 32 * BK>(af[1][0], a_base[0]);
    read_frag<OFF + 32 * BK>(af[1][1], a_base[1]);
  };
  auto read_scales = [&](auto buf) { read_scale_words<decltype(buf)::value * SCALE_BYTES>(sa, sw, sa_base, sw_base); };
  auto read_w = [&](auto buf, auto nq, Frag (&dst)[2]) {
    constexpr int OFF = decltype(buf)::value * 2 * OP_BYTES + decltype(nq)::value * 32 * BK;
    read_frag<OFF>(dst[0], w_base[0]);
    read_frag<OFF>(dst[1], w_base[1]);
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

  // MFMA segment of one phase: 4 MFMA 32x32x64 on one 64x32 quadrant; the phase's DMA pieces (pieces i0 .. i0 + NP of operand
  // st_op, K-tile st_kt) behind the 2nd and the 3rd
  auto mma_quadrant = [&](int mq, int nq, int wset, int st_kt, int st_op, int i0, auto np) {
    constexpr int NP = decltype(np)::value;
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
      acc[mq * 2 + mb][nq] = mfma_mx<0>(bfr[wset][0], af[mb][0], acc[mq * 2 + mb][nq], sw[nq], sa[mq * 2 + mb]);
    GM_FENCE();
    stage_piece(st_kt, st_op, i0);
    GM_FENCE();
    acc[mq * 2][nq] = mfma_mx<1>(bfr[wset][1], af[0][1], acc[mq * 2][nq], sw[nq], sa[mq * 2]);
    if (NP == 2) {
      GM_FENCE();
      stage_piece(st_kt, st_op, i0 + 1);
      GM_FENCE();
    }
    acc[mq * 2 + 1][nq] = mfma_mx<1>(bfr[wset][1], af[1][1], acc[mq * 2 + 1][nq], sw[nq], sa[mq * 2 + 1]);
    // (pins the phase's MFMAs in front of the statements that follow: with the fragments read by asm, nothing else ties an MFMA to
    // its phase, and the compiler otherwise sinks all sixteen of a tile behind its last barrier)
    asm volatile("" : "+v"(acc[mq * 2][nq]), "+v"(acc[mq * 2 + 1][nq]));
    __builtin_amdgcn_s_setprio(0);
  };
  const std::integral_constant<int, 0> I0{};
  const std::integral_constant<int, 1> ONE{};
  const std::integral_constant<int, 2> TWO{};

  // ---- prologue / K loop: the sibling's schedule (phases, counted vmcnt(2), one-barrier stagger of the wave groups); the first
  //      tile's scales are the oldest piece in flight, so the prologue's wait retires it
  stage_scales(kt_begin);
  stage_op(kt_begin, 1);
  stage_op(kt_begin, 0);
  stage_op(kt_begin + 1, 1);
  asm volatile("s_waitcnt vmcnt(3)" ::: "memory");   // leaves the second tile's W in flight
  GM_BARRIER();
  if (wr == 1) GM_BARRIER();
  read_w(I0, I0, bfr[0]);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  GM_FENCE();

  // par = parity of the tile counted from kt_begin: the W fragments of quadrant column 0 are in bfr[par] (read in phase 3 of the
  // previous tile, or by the prologue), those of column 1 go to bfr[1 - par], which the previous tile used last in its phase 3;
  // phase 3 reads the next tile's column 0 into bfr[1 - par], free since phase 2 (behind the last tile: whatever the buffer holds)
  auto k_tile = [&](const int kt, auto par) {
    constexpr int W0 = decltype(par)::value, W1 = 1 - W0;
    const std::integral_constant<int, W0> buf{};       // the tile's LDS buffer is its parity as well
    const std::integral_constant<int, W1> buf_next{};
    stage_scales(kt + 1);
    GM_FENCE();
    read_scales(buf);
    read_a(buf, I0);
    GM_PHASE_SYNC();
    mma_quadrant(0, 0, W0, kt + 1, 0, 0, TWO);
    GM_BARRIER();
    read_w(buf, ONE, bfr[W1]);
    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");   // leaves phase 0's two pieces in flight; the scale piece of the tile top is older
    GM_PHASE_SYNC();
    mma_quadrant(0, 1, W1, kt + 1, 0, 2, ONE);
    GM_BARRIER();
    read_a(buf, ONE);
    GM_PHASE_SYNC();
    mma_quadrant(1, 1, W1, kt + 2, 1, 0, TWO);
    GM_BARRIER();
    read_w(buf_next, I0, bfr[W1]);
    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");   // leaves phase 2's two pieces in flight: phase 1's piece is older
    GM_PHASE_SYNC();
    mma_quadrant(1, 0, W0, kt + 2, 1, 2, ONE);
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

  if (is_split && !split_k_reduce<4>(acc, sp, unit, seg, tile_id, smem, tid, wave, lane)) return;

  const bool wide = !((p.ldc | (p.residual ? p.ldr : 0)) & 7) && !(((uintptr_t)p.C | (uintptr_t)p.residual) & 15);
  if (wide) {
    if (is_split) __syncthreads();
    store_tile_lds<false, 4>(p, m0 + wr * 128, n0 + wc * 64, lane, smem + wave * (128 * 128), acc);   // gemm_core.h
  } else {
    store_tile<false, Cfg>(p, m0 + wr * 128, n0 + wc * 64, lane, acc);
  }
}

static int launch_gemm_mxfp6(GemmParams p, const gm6::Args& f, hipStream_t stream) {
  auto fail = [&](const char* what) { return set_error(-1, (std::string("gemm_mxfp6: ") + what).c_str()); };
  if (p.M <= 0 || p.N <= 0 || p.K <= 0) return fail("empty problem");
  if (p.K % gm6::BK_ELEMS) return fail("K must be a multiple of 128");
  if (p.N % 8) return fail("N must be a multiple of 8");
  const int row_bytes = RTV_MXFP6_CODE_BYTES(p.K);
  if ((f.lda % 16) || (f.ldw % 16) || f.lda < row_bytes || f.ldw < row_bytes || (p.ldc % 4) || (p.residual && (p.ldr % 4)))
    return fail("leading dimensions must be >= 3 K / 4 bytes and keep 16-byte (A,W) / 8-byte (C,res) alignment");
  if (((uintptr_t)f.A & 15) || ((uintptr_t)f.W & 15)) return fail("A_codes and W_codes must be 16-byte aligned");
  if (((uintptr_t)f.a_scales & 3) || ((uintptr_t)f.w_scales & 3)) return fail("a_scales and w_scales must be 4-byte aligned");
  // the kernel addresses codes and scales with 32-bit offsets from the operand bases
  if ((uint64_t)p.M * (uint64_t)f.lda >= (1ull << 32) || (uint64_t)p.N * (uint64_t)f.ldw >= (1ull << 32)) return fail("operand larger than 4 GiB");
  if (p.gate && p.rows_per_frame <= 0) return fail("gate needs rows_per_frame");
  p.tiles_m = (p.M + gm6::BM - 1) / gm6::BM;
  p.tiles_n = (p.N + gm6::BN - 1) / gm6::BN;
  static LdsAttr lds_attr;   // per device (a second GPU used from this process needs the attribute as well)
  if (int st = ensure_dynamic_lds((const void*)gemm_mxfp6_kernel, gm6::LDS_BYTES, &lds_attr, "gemm_mxfp6")) return st;
  SplitArgs sp;
  int grid = 0;
  // the planner keeps >= 4 of the K-tiles it is told of per segment: told of 256-element tiles, as the MXFP4 kernel tells it, a
  // segment is >= 8 of this kernel's tiles and K = 2048 stays the smallest K that splits (the kernel cuts its own K / 128 tiles)
  if (int st = plan_split_k(p.tiles_m * p.tiles_n, p.K / 256, true, &sp, &grid, stream)) return st;
  ProfScope prof(PROF_GEMM, stream, 2.0 * p.M * (double)p.N * p.K);
  note_kernel(DK_GEMM_MXFP6_256x256);
  hipLaunchKernelGGL(gemm_mxfp6_kernel, dim3(grid), dim3(gm6::THREADS), gm6::LDS_BYTES, stream, p, f, sp);
  return check_launch("gemm_mxfp6");
}

}  // namespace rtv

using namespace rtv;

extern "C" int rtv_gemm_mxfp6(const void* A_codes, int lda, const void* W_codes, int ldw, const void* a_scales, const void* w_scales,
                              void* C, int ldc, int M, int N, int K, const void* bias, int act, const void* gate, int gate_stride,
                              int rows_per_frame, int row_offset, const void* residual, int ldr, rtv_stream_t stream) {
  if (!A_codes || !W_codes || !C || !a_scales || !w_scales) return set_error(-1, "gemm_mxfp6: null pointer");
  const GemmParams p = gemm_params(nullptr, lda, nullptr, ldw, C, ldc, M, N, K, bias, act, gate, gate_stride, rows_per_frame, row_offset,
                                   residual, ldr);
  const gm6::Args f{(const uint8_t*)A_codes, (const uint8_t*)W_codes, lda, ldw, (const uint8_t*)a_scales, (const uint8_t*)w_scales};
  return launch_gemm_mxfp6(p, f, (hipStream_t)stream);
}
