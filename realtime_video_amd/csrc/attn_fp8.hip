// fp8 self-attention for gfx950 on an e4m3 shadow of the bf16 KV cache (include/rtv_hip_attn_fp8.h): the precision of the
// reference's SageAttention backend (wan/modules/sage.py: 8-bit Q K^T, fp8 P V) at the plug-in point attn_fwd.hip serves in bf16.
//
//   attn_quantize_kv_kernel   rows of the bf16 cache -> k8 (row-major e4m3) and v8t (e4m3, transposed per 64-row storage tile, keys
//                             in the slot order of the header); its CENTER instantiation codes k - c (rtv_hip_attn_fp8_center.h)
//   attn_kv_center_*_kernel   c = the fp32 column means of K over a key window, in two stages without atomics
//   attn_fwd_fp8_kernel       the structure of attn_fwd_kernel (attn_fwd.hip): 8 waves x 32 query rows of one head, 64-key tiles
//                             through double-buffered LDS, compiler-scheduled.  S^T = K . Q^T and O^T += V^T . P^T both on
//                             v_mfma_f32_32x32x64_f8f6f4: 4 + 4 MFMAs of 64 cycles per tile instead of 16 + 16 of 32.
//     * a tile is a STORAGE tile (physical rows 64 T .. 64 T + 63), so that a v8t tile of one head is one contiguous 8 KiB run;
//       the first and last tile of each range of the key window are in general partial: their keys outside the window get the
//       score -inf and their bytes of the V^T operand are replaced by zero (0 x NaN is NaN in the MFMA);
//     * a lane owns one query column; its 32 probabilities of a tile, in register order, are its 32 k-bytes of the P^T operand
//       (the slot order of v8t is chosen for exactly that), so nothing moves between lanes from the first product to the second;
//     * Q is quantised in the prologue, one scale per (row, head): the lane and its partner lane ^ 32 hold the row.
#include <cmath>

#include <string>
#include <type_traits>

#include "../../include/rtv_hip_attn_fp8.h"
#include "../../include/rtv_hip_attn_fp8_center.h"
#include "../../include/rtv_hip_attn_fp8_cp.h"
#include "attn_common.h"
#include "fp8_quant.h"

namespace rtv {

namespace af8 {
typedef __attribute__((ext_vector_type(8))) int v8i;
typedef __attribute__((ext_vector_type(4))) int v4i;
constexpr int TILE_BYTES = ATT_KT * ATT_D;   // 8 KiB: a K tile [64 keys][128 B] and a V^T tile [128 dims][64 B]
constexpr int NW = 8;                        // waves per workgroup
constexpr int QT = NW * ATT_QW;              // query rows per workgroup

__device__ __forceinline__ f32x16 mfma_fp8(const v8i& a, const v8i& b, const f32x16& c) {
  // cbsz = blgp = 0: both operands e4m3; zero scale operands select the plain v_mfma_f32_32x32x64_f8f6f4 (gemm_fp8_body.h)
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0, 0, 0);
}
__device__ __forceinline__ v8i load_frag(const char* lo, const char* hi) {
  const v4i a = *(const v4i*)lo, b = *(const v4i*)hi;
  return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}
// LDS images.  K tile: row = key, 8 chunks of 16 B, chunk ^ ((row >> 1) & 7) (the fragment read of gemm_fp8_body.h: lane = row,
// two neighbouring chunks).  V^T tile: row = dim, 4 chunks of 16 B, chunk ^ ((dim >> 2) & 3): the 16 dims a quarter wave reads
// together land in 16 different 16-byte bank groups.
__device__ __forceinline__ int k_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
__device__ __forceinline__ int v_off(int dim, int chunk) { return dim * 64 + ((chunk ^ ((dim >> 2) & 3)) << 4); }

struct QuantParams {
  const uint16_t* k;
  const uint16_t* v;
  int64_t rs;
  int row0, rows, H, tile0;
  uint8_t* k8;
  uint8_t* v8t;
  float k_scale, v_scale;
  unsigned* amax;
};
struct QuantParamsCentered : QuantParams {
  const float* center;   // [H][128] fp32
};

struct CenterParams {
  const uint16_t* k;
  int64_t rs;
  int row0, n0, row1, n1, H;
  float* part;     // [chunks][H][128] fp32
  float* center;   // [H][128] fp32
  int chunks;
};

struct FwdParams {
  const uint16_t* q;
  const uint8_t* k8;
  const uint8_t* v8t;
  uint16_t* o;
  int Lq, H, cache_rows;
  int row0, n0, row1, n1;
  int64_t q_rs, o_rs;
  float mult;      // scale * log2(e) * k_scale: the lane multiplies it by its row's s_q
  float v_scale;
  int causal_block, q_offset;
  int n_qtiles;
};
// KV split (rtv_hip_attn_fp8_cp.h): blockIdx.y = range s of kv_splits; the partials in the layout of attn_common.h's store_partial
struct FwdParamsSplit : FwdParams {
  int kv_splits;
  float* part_o;    // [S][H][Lq][128] unnormalised fp32 O, without v_scale
  float* part_ml;   // [S][H][Lq][2] = (m, l), m in the row's scaled log2 domain
};
}  // namespace af8

// One workgroup = one (storage tile, head): thread (kq, dc) converts keys 4 kq .. 4 kq + 3 of the tile, dims 8 dc .. 8 dc + 7, of K
// and of V.  K codes leave at once (8 bytes per key); the V codes of the four keys make one 32-bit word per dim - four neighbouring
// slots - which goes through LDS so that the tile leaves as whole 16-byte pieces of its [dim][64 slots] rows.  Only bytes of rows
// inside [row0, row0 + rows) are written: a partly covered tile falls back to 4-byte words and single bytes.
// CENTER: the K codes are those of k - c; the thread's 8 channels of c stay in registers over its four keys.
template <bool CENTER>
__global__ __launch_bounds__(256) void attn_quantize_kv_kernel(std::conditional_t<CENTER, af8::QuantParamsCentered, af8::QuantParams> p) {
  constexpr int LD = 17;   // words per dim row of the LDS image (16 + 1: the dims of a wave do not all start in one bank)
  __shared__ __attribute__((aligned(16))) uint32_t sV[ATT_D * LD];
  __shared__ float s_max[2][4];
  const int tid = threadIdx.x;
  const int T = p.tile0 + blockIdx.x, h = blockIdx.y;
  const int dc = tid & 15, kq = tid >> 4;
  const int r_lo = max(p.row0 - T * ATT_KT, 0), r_hi = min(p.row0 + p.rows - T * ATT_KT, ATT_KT);   // tile-local rows to convert
  float kmax = 0.f, vmax = 0.f;
  uint32_t vw[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  float cen[8];
  if constexpr (CENTER) {
    const f32x4 c0 = *(const f32x4*)(p.center + (size_t)h * ATT_D + dc * 8), c1 = *(const f32x4*)(p.center + (size_t)h * ATT_D + dc * 8 + 4);
#pragma unroll
    for (int d = 0; d < 4; ++d) cen[d] = c0[d], cen[4 + d] = c1[d];
  }
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int key = 4 * kq + jj;
    if (key < r_lo || key >= r_hi) continue;
    const int64_t phys = (int64_t)T * ATT_KT + key;
    const size_t src = (size_t)(phys * p.rs) + (size_t)h * ATT_D + dc * 8;
    const u32x4 kr = *(const u32x4*)(p.k + src), vr = *(const u32x4*)(p.v + src);
    float x[8];
    unpack_bf16x8(kr, x);
    if constexpr (CENTER) {
#pragma unroll
      for (int d = 0; d < 8; ++d) x[d] -= cen[d];   // fp32, rounded once, before the division
    }
#pragma unroll
    for (int d = 0; d < 8; ++d) kmax = fmaxf(kmax, fabsf(x[d]));
    *(u32x2*)(p.k8 + ((size_t)phys * p.H + h) * ATT_D + dc * 8) = quantize8(x, p.k_scale);
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
    kmax = wave_max(kmax);
    vmax = wave_max(vmax);
    if ((tid & 63) == 0) {
      s_max[0][tid >> 6] = kmax;
      s_max[1][tid >> 6] = vmax;
    }
  }
  __syncthreads();
  if (p.amax != nullptr && tid < 2) {
    // non-negative floats order like their bit patterns; most workgroups find the maximum already there and only read
    const float m = fmaxf(fmaxf(s_max[tid][0], s_max[tid][1]), fmaxf(s_max[tid][2], s_max[tid][3]));
    const unsigned bits = __float_as_uint(m);
    if (bits > __atomic_load_n(p.amax + tid, __ATOMIC_RELAXED)) atomicMax(p.amax + tid, bits);
  }
  uint8_t* const tile = p.v8t + ((size_t)T * p.H + h) * af8::TILE_BYTES;
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

// Column means of K, stage 1.  One workgroup = one (chunk of RTV_ATTN_CENTER_CHUNK window rows, head): thread (rq, dc) adds the
// rows rq, rq + 16, ... of the chunk, dims 8 dc .. 8 dc + 7, in ascending order; the 16 row groups are then added in ascending
// order through LDS.  Window row j is physical row row0 + j, or row1 + (j - n0) behind the first range.
__global__ __launch_bounds__(256) void attn_kv_center_partial_kernel(af8::CenterParams p) {
  __shared__ float sP[16][ATT_D + 4];
  const int tid = threadIdx.x, dc = tid & 15, rq = tid >> 4, h = blockIdx.y;
  const int n = p.n0 + p.n1;
  const int j0 = blockIdx.x * RTV_ATTN_CENTER_CHUNK, j1 = min(j0 + RTV_ATTN_CENTER_CHUNK, n);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j = j0 + rq; j < j1; j += 16) {
    const int64_t phys = j < p.n0 ? (int64_t)p.row0 + j : (int64_t)p.row1 + (j - p.n0);
    const u32x4 kr = *(const u32x4*)(p.k + (size_t)(phys * p.rs) + (size_t)h * ATT_D + dc * 8);
    float x[8];
    unpack_bf16x8(kr, x);
#pragma unroll
    for (int d = 0; d < 8; ++d) acc[d] += x[d];
  }
#pragma unroll
  for (int d = 0; d < 8; ++d) sP[rq][dc * 8 + d] = acc[d];
  __syncthreads();
  if (tid < ATT_D) {
    float s = sP[0][tid];
#pragma unroll
    for (int r = 1; r < 16; ++r) s += sP[r][tid];
    p.part[((size_t)blockIdx.x * p.H + h) * ATT_D + tid] = s;
  }
}

// Stage 2.  One workgroup = one head, one thread = one channel: the chunks in ascending order, then one division.
__global__ __launch_bounds__(ATT_D) void attn_kv_center_reduce_kernel(af8::CenterParams p) {
  const int d = threadIdx.x, h = blockIdx.x;
  float s = 0.f;
  for (int c = 0; c < p.chunks; ++c) s += p.part[((size_t)c * p.H + h) * ATT_D + d];
  p.center[(size_t)h * ATT_D + d] = s / (float)(p.n0 + p.n1);
}

// SPLIT: the workgroup (blockIdx.x as before, range s = blockIdx.y of S) works on the storage tiles [ntiles s / S, ntiles (s + 1) / S)
// of its own tile list - split_tile_range's rule - and leaves (m, l, unnormalised O) through store_partial; attn_fp8_combine_kernel
// merges.  An empty range loads nothing, touches no LDS and leaves (-1e30, 0, 0), as a row does whose keys in the range are all masked.
template <bool SPLIT>
__global__ __launch_bounds__(af8::NW * 64) void attn_fwd_fp8_kernel(std::conditional_t<SPLIT, af8::FwdParamsSplit, af8::FwdParams> p) {
  using namespace af8;
  // smem: K[2][8 KiB] | V^T[2][8 KiB]
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE_BYTES];
  char* const sK = smem;
  char* const sV = smem + 2 * TILE_BYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, g = lane >> 5;

  // ---- workgroup -> (head, q tile): with H % 8 == 0 all q tiles of a head run on ONE XCD (attn_fwd.hip)
  int h, qt;
  {
    const int bid = blockIdx.x;
    if (p.H % 8 == 0) {
      const int xcd = bid & 7, slot = bid >> 3;
      h = xcd + 8 * (slot / p.n_qtiles);
      qt = slot % p.n_qtiles;
    } else {
      h = bid / p.n_qtiles;
      qt = bid % p.n_qtiles;
    }
  }
  const int q0 = qt * QT;
  const int q_row = q0 + wave * ATT_QW + l31;
  const int q_row_c = min(q_row, p.Lq - 1);

  // ---- key-prefix limits (block-causal rule of attn_fwd.hip; n1 == 0 then), in keys of the window
  int kv_lim = p.n0, wave_min_lim = p.n0, wg_max_lim = p.n0;
  if (p.causal_block > 0) {
    const int cb = p.causal_block;
    kv_lim = min(p.n0, ((p.q_offset + q_row_c) / cb + 1) * cb);
    const int first = min(q0 + wave * ATT_QW, p.Lq - 1);
    wave_min_lim = min(p.n0, ((p.q_offset + first) / cb + 1) * cb);
    const int last = min(q0 + QT - 1, p.Lq - 1);
    wg_max_lim = min(p.n0, ((p.q_offset + last) / cb + 1) * cb);
  }
  // storage tiles of the two ranges (the first one cut at the workgroup's largest limit)
  const int ta0 = p.row0 >> 6, nt0 = ((p.row0 + wg_max_lim - 1) >> 6) - ta0 + 1;
  const int ta1 = p.row1 >> 6, nt1 = p.n1 > 0 ? ((p.row1 + p.n1 - 1) >> 6) - ta1 + 1 : 0;
  const int ntiles = nt0 + nt1;
  auto tile_of = [&](int j) { return j < nt0 ? ta0 + j : ta1 + (j - nt0); };
  int t_lo = 0, t_hi = ntiles;   // this workgroup's share of its tile list (workgroup-uniform)
  if constexpr (SPLIT) {
    t_lo = ntiles * (int)blockIdx.y / p.kv_splits;
    t_hi = ntiles * ((int)blockIdx.y + 1) / p.kv_splits;
  }
  const bool work = !SPLIT || t_lo < t_hi;

  // ---- staging: one 16-byte chunk of K and one of V^T per thread and tile.  K rows beyond the cache (the last storage tile) are
  //      clamped: they are outside every window.  A v8t tile is whole by construction.
  u32x4 kreg, vreg;
  const int st_r = tid >> 3, st_c = tid & 7;
  auto load_tile = [&](int j) {
    const int T = tile_of(j);
    const int row = min(T * ATT_KT + st_r, p.cache_rows - 1);
    kreg = *(const u32x4*)(p.k8 + ((size_t)row * p.H + h) * ATT_D + st_c * 16);
    vreg = *(const u32x4*)(p.v8t + ((size_t)T * p.H + h) * TILE_BYTES + tid * 16);
  };
  char* const k_wr = sK + k_off(st_r, st_c);
  char* const v_wr = sV + v_off(tid >> 2, tid & 3);
  auto write_tile = [&](int buf) {
    *(u32x4*)(k_wr + buf * TILE_BYTES) = kreg;
    *(u32x4*)(v_wr + buf * TILE_BYTES) = vreg;
  };
  if (work) load_tile(t_lo);

  // ---- Q^T fragments (MFMA B operand): lane holds the codes of Q[q][64 st + 32 g .. + 32], st = 0, 1; the row's scale comes from
  //      the maximum over this lane's 64 values and those of lane ^ 32
  v8i qf[2];
  float c;   // this row's score multiplier: s_q * k_scale * scale * log2(e)
  {
    const uint16_t* qp = p.q + (size_t)q_row_c * p.q_rs + (size_t)h * ATT_D + g * 32;
    u32x4 raw[2][4];
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int i = 0; i < 4; ++i) raw[st][i] = *(const u32x4*)(qp + st * 64 + i * 8);
    float amax = 0.f;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float x[8];
        unpack_bf16x8(raw[st][i], x);
#pragma unroll
        for (int d = 0; d < 8; ++d) amax = fmaxf(amax, fabsf(x[d]));
      }
    amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
    const float s_q = fp8_scale(amax);
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float x[8];
        unpack_bf16x8(raw[st][i], x);
        const u32x2 w = quantize8(x, s_q);
        qf[st][2 * i] = (int)w[0];
        qf[st][2 * i + 1] = (int)w[1];
      }
    c = s_q * p.mult;
  }

  // ---- per-lane LDS read addresses.  K operand (A): row = 32 kb + l31, chunks 4 st + 2 g and + 1.  V^T operand (A): row = dim
  //      32 db + l31, chunks 2 g and 2 g + 1 = slots 32 g .. 32 g + 31.
  const char* k_rd[2][2][2];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int e = 0; e < 2; ++e) k_rd[kb][st][e] = sK + k_off(kb * 32 + l31, st * 4 + g * 2 + e);
  const char* v_rd[4][2];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int e = 0; e < 2; ++e) v_rd[db][e] = sV + v_off(db * 32 + l31, g * 2 + e);

  f32x16 oacc[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[db][r] = 0.f;
  float m_run = -1e30f;  // reference point of the exponentials (>= running max - RESCALE_SLACK), log2 domain
  float l_run = 0.f;     // this lane's partial row sum
  const f32x2 c2 = {c, c};
  constexpr float RESCALE_SLACK = 8.f;   // lazy rescaling as in attn_fwd.hip: P <= 2^8 < 448, the e4m3 maximum

  auto tile = [&](const int j, auto bufc) {
    constexpr int buf = decltype(bufc)::value;
    const bool has_next = (j + 1 < t_hi);
    if (has_next) load_tile(j + 1);  // in flight during the MFMAs below

    // ---------------- S^T = K . Q^T   (two independent accumulator chains)
    f32x16 sacc[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[kb][r] = 0.f;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        const v8i kf = load_frag(k_rd[kb][st][0] + buf * TILE_BYTES, k_rd[kb][st][1] + buf * TILE_BYTES);
        sacc[kb] = mfma_fp8(kf, qf[st], sacc[kb]);
      }

    // ---------------- the tile's share of the window (workgroup-uniform): local keys [vlo, vhi)
    const int T = tile_of(j);
    const int rlo = j < nt0 ? p.row0 : p.row1, rhi = j < nt0 ? p.row0 + wg_max_lim : p.row1 + p.n1;
    const int vlo = max(rlo - T * ATT_KT, 0), vhi = min(rhi - T * ATT_KT, ATT_KT);
    const bool edge = vlo > 0 || vhi < ATT_KT;
    // ---------------- mask (edge tiles and tiles that cross a causal limit of this wave); a select, so a NaN score of a row
    //                  outside the window does not survive it
    const bool causal = p.causal_block > 0;   // (causal launches have one range: every tile belongs to [row0, row0 + n0))
    if (edge || (causal && p.row0 + wave_min_lim < (T + 1) * ATT_KT)) {
      const int lane_hi = causal ? min(vhi, p.row0 + kv_lim - T * ATT_KT) : vhi;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kl = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
          if (kl < vlo || kl >= lane_hi) sacc[kb][r] = -INFINITY;
        }
    }

    // ---------------- online softmax (row = lane's query; the row is split over lanes l and l^32)
    float mx = sacc[0][0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sacc[0][r]);
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[1][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_cand = fmaxf(m_run, mx * c);
    const bool need = m_cand - m_run > RESCALE_SLACK;
    if (__builtin_amdgcn_ballot_w64(need) != 0) {
      // wave-uniform branch, per-row decision (attn_fwd.hip): rows that do not need it multiply by exp2(0) = 1 exactly
      const float m_new = need ? m_cand : m_run;
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      l_run *= alpha;
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[db][r] *= alpha;
    }
    const f32x2 nm2 = {-m_run, -m_run};
    f32x2 ps2 = {0.f, 0.f};
    v8i pf;   // P^T operand: word w = keys (kb, r) = (w >> 2, 4 (w & 3) .. + 3) = the lane's k-bytes 4 w .. 4 w + 3
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x2 x0 = {sacc[kb][4 * i], sacc[kb][4 * i + 1]}, x1 = {sacc[kb][4 * i + 2], sacc[kb][4 * i + 3]};
        x0 = __builtin_elementwise_fma(x0, c2, nm2);
        x1 = __builtin_elementwise_fma(x1, c2, nm2);
        const f32x2 e0 = {__builtin_amdgcn_exp2f(x0[0]), __builtin_amdgcn_exp2f(x0[1])};
        const f32x2 e1 = {__builtin_amdgcn_exp2f(x1[0]), __builtin_amdgcn_exp2f(x1[1])};
        ps2 += e0;
        ps2 += e1;
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(e0[0], e0[1], w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(e1[0], e1[1], w, true);
        pf[kb * 4 + i] = w;
      }
    l_run += ps2[0] + ps2[1];

    // ---------------- O^T += V^T . P^T   (four independent accumulator chains)
    v8i vf[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) vf[db] = load_frag(v_rd[db][0] + buf * TILE_BYTES, v_rd[db][1] + buf * TILE_BYTES);
    if (edge) {
      // slot 32 g + 4 w + b of the tile = key 32 (w >> 2) + 8 (w & 3) + 4 g + b: zero the bytes of keys outside the window
#pragma unroll
      for (int w = 0; w < 8; ++w) {
        const int key0 = 32 * (w >> 2) + 8 * (w & 3) + 4 * g;
        uint32_t keep = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (key0 + b >= vlo && key0 + b < vhi) keep |= 0xffu << (8 * b);
#pragma unroll
        for (int db = 0; db < 4; ++db) vf[db][w] &= (int)keep;
      }
    }
#pragma unroll
    for (int db = 0; db < 4; ++db) oacc[db] = mfma_fp8(vf[db], pf, oacc[db]);

    if (has_next) write_tile(buf ^ 1);
    __syncthreads();
  };

  if (work) {
    write_tile(0);
    __syncthreads();
  }
  for (int j = t_lo; j < t_hi; j += 2) {
    tile(j, IntC<0>{});
    if (j + 1 < t_hi) tile(j + 1, IntC<1>{});
  }

  // ---------------- epilogue: O = O^T * v_scale / l, lane owns row q and dims db*32 + 8*i + 4*g + {0..3}
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  if constexpr (SPLIT) {
    AttnParams ap;   // what store_partial reads
    ap.B = 1;
    ap.H = p.H;
    ap.Lq = p.Lq;
    ap.part_o = p.part_o;
    ap.part_ml = p.part_ml;
    store_partial(ap, h, q_row, g, oacc, m_run, l_tot);
    return;
  }
  const float inv = p.v_scale / l_tot;
  if (q_row < p.Lq) {
    uint16_t* op = p.o + (size_t)q_row * p.o_rs + (size_t)h * ATT_D + 4 * g;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        u32x2 w;
        w[0] = pack_bf16x2(oacc[db][4 * i + 0] * inv, oacc[db][4 * i + 1] * inv);
        w[1] = pack_bf16x2(oacc[db][4 * i + 2] * inv, oacc[db][4 * i + 3] * inv);
        *(u32x2*)(op + db * 32 + i * 8) = w;
      }
  }
}

// Merge of the S partial results of a row (the rule of attn_combine_kernel, attn_fwd.hip, with the V scale): m = max m_s,
// w_s = 2^(m_s - m), O = v_scale sum w_s O_s / sum w_s l_s, rounded once to bf16.  16 threads per row (8 dims each), 16 rows per
// workgroup; the ranges in ascending order, no atomics.
__global__ __launch_bounds__(256) void attn_fp8_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                                               uint16_t* __restrict__ o, int S, int H, int Lq, int64_t o_rs,
                                                               float v_scale) {
  const int64_t nrows = (int64_t)H * Lq;
  const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (row >= nrows) return;
  const int c8 = (threadIdx.x & 15) * 8;
  float m = -INFINITY;
  for (int s = 0; s < S; ++s) m = fmaxf(m, part_ml[((int64_t)s * nrows + row) * 2]);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float l = 0.f;
  for (int s = 0; s < S; ++s) {
    const f32x2 ml = *(const f32x2*)(part_ml + ((int64_t)s * nrows + row) * 2);
    const float w = __builtin_amdgcn_exp2f(ml[0] - m);
    l += w * ml[1];
    const float* po = part_o + ((int64_t)s * nrows + row) * ATT_D + c8;
    const f32x4 a = *(const f32x4*)po, b2 = *(const f32x4*)(po + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[i] += w * a[i];
      acc[4 + i] += w * b2[i];
    }
  }
  const float inv = v_scale / l;
  const int h = (int)(row / Lq), q = (int)(row - (int64_t)h * Lq);
  u32x4 out;
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = pack_bf16x2(acc[2 * i] * inv, acc[2 * i + 1] * inv);
  *(u32x4*)(o + (size_t)q * o_rs + (size_t)h * ATT_D + c8) = out;
}

}  // namespace rtv

using namespace rtv;

// The checks and the launch of both quantisers; center != null selects the CENTER instantiation.
static int quantize_kv_launch(const void* k, const void* v, int64_t row_stride, int row0, int rows, int H, void* k8, void* v8t,
                              int cache_rows, float k_scale, float v_scale, void* amax, const float* center, bool centered,
                              rtv_stream_t stream) {
  if (!k || !v || !k8 || !v8t) return set_error(-1, "attn_quantize_kv: null pointer");
  if (((uintptr_t)k | (uintptr_t)v | (uintptr_t)k8 | (uintptr_t)v8t) & 15)
    return set_error(-1, "attn_quantize_kv: k, v, k8 and v8t must be 16-byte aligned");
  if ((uintptr_t)amax & 3) return set_error(-1, "attn_quantize_kv: amax must be 4-byte aligned");
  if (centered && (!center || ((uintptr_t)center & 15)))
    return set_error(-1, "attn_quantize_kv: center must be a 16-byte aligned device float[H][128]");
  if (rows <= 0 || H <= 0 || cache_rows <= 0) return set_error(-1, "attn_quantize_kv: rows, H and cache_rows must be positive");
  if (row0 < 0 || (int64_t)row0 + rows > cache_rows) return set_error(-1, "attn_quantize_kv: row range outside [0, cache_rows)");
  if (row_stride < (int64_t)H * ATT_D || (row_stride & 7))
    return set_error(-1, "attn_quantize_kv: row stride must be a multiple of 8 elements and hold H heads");
  if (!good_scale(k_scale) || !good_scale(v_scale)) return set_error(-1, "attn_quantize_kv: scales must be finite and positive");
  if (H > 65535) return set_error(-1, "attn_quantize_kv: more than 65535 heads");
  af8::QuantParamsCentered p;
  p.k = (const uint16_t*)k;
  p.v = (const uint16_t*)v;
  p.rs = row_stride;
  p.row0 = row0;
  p.rows = rows;
  p.H = H;
  p.tile0 = row0 >> 6;
  p.k8 = (uint8_t*)k8;
  p.v8t = (uint8_t*)v8t;
  p.k_scale = k_scale;
  p.v_scale = v_scale;
  p.amax = (unsigned*)amax;
  p.center = center;
  const int tiles = ((row0 + rows - 1) >> 6) - p.tile0 + 1;
  ProfScope prof(PROF_MISC, (hipStream_t)stream, 0.0);
  if (centered)
    hipLaunchKernelGGL(attn_quantize_kv_kernel<true>, dim3(tiles, H), dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(attn_quantize_kv_kernel<false>, dim3(tiles, H), dim3(256), 0, (hipStream_t)stream, (const af8::QuantParams&)p);
  return check_launch("attn_quantize_kv");
}

extern "C" int rtv_attn_quantize_kv(const void* k, const void* v, int64_t row_stride, int row0, int rows, int H, void* k8,
                                    void* v8t, int cache_rows, float k_scale, float v_scale, void* amax, rtv_stream_t stream) {
  return quantize_kv_launch(k, v, row_stride, row0, rows, H, k8, v8t, cache_rows, k_scale, v_scale, amax, nullptr, false, stream);
}

extern "C" int rtv_attn_quantize_kv_centered(const void* k, const void* v, int64_t row_stride, int row0, int rows, int H, void* k8,
                                             void* v8t, int cache_rows, float k_scale, float v_scale, void* amax,
                                             const float* center, rtv_stream_t stream) {
  return quantize_kv_launch(k, v, row_stride, row0, rows, H, k8, v8t, cache_rows, k_scale, v_scale, amax, center, true, stream);
}

extern "C" size_t rtv_attn_kv_center_workspace_bytes(int rows, int H) {
  if (rows <= 0 || H <= 0) return 0;
  return (((size_t)rows + RTV_ATTN_CENTER_CHUNK - 1) / RTV_ATTN_CENTER_CHUNK) * (size_t)H * ATT_D * sizeof(float);
}

extern "C" int rtv_attn_kv_center(const void* k, int64_t row_stride, int row0, int n0, int row1, int n1, int H, float* center,
                                  void* workspace, size_t workspace_bytes, rtv_stream_t stream) {
  if (!k || !center || !workspace) return set_error(-1, "attn_kv_center: null pointer");
  if (((uintptr_t)k | (uintptr_t)center | (uintptr_t)workspace) & 15)
    return set_error(-1, "attn_kv_center: k, center and workspace must be 16-byte aligned");
  if (n0 <= 0 || H <= 0) return set_error(-1, "attn_kv_center: n0 and H must be positive");
  if (n1 < 0) return set_error(-1, "attn_kv_center: negative segment length");
  if (row0 < 0 || (n1 > 0 && row1 < 0)) return set_error(-1, "attn_kv_center: negative first row");
  if ((int64_t)n0 + n1 > INT32_MAX) return set_error(-1, "attn_kv_center: too many rows");
  if (row_stride < (int64_t)H * ATT_D || (row_stride & 7))
    return set_error(-1, "attn_kv_center: row stride must be a multiple of 8 elements and hold H heads");
  if (H > 65535) return set_error(-1, "attn_kv_center: more than 65535 heads");
  if (workspace_bytes < rtv_attn_kv_center_workspace_bytes(n0 + n1, H))
    return set_error(-1, "attn_kv_center: workspace below rtv_attn_kv_center_workspace_bytes(n0 + n1, H)");
  af8::CenterParams p;
  p.k = (const uint16_t*)k;
  p.rs = row_stride;
  p.row0 = row0;
  p.n0 = n0;
  p.row1 = n1 > 0 ? row1 : 0;
  p.n1 = n1;
  p.H = H;
  p.part = (float*)workspace;
  p.center = center;
  p.chunks = (n0 + n1 + RTV_ATTN_CENTER_CHUNK - 1) / RTV_ATTN_CENTER_CHUNK;
  ProfScope prof(PROF_MISC, (hipStream_t)stream, 0.0);
  hipLaunchKernelGGL(attn_kv_center_partial_kernel, dim3(p.chunks, H), dim3(256), 0, (hipStream_t)stream, p);
  hipLaunchKernelGGL(attn_kv_center_reduce_kernel, dim3(H), dim3(ATT_D), 0, (hipStream_t)stream, p);
  return check_launch("attn_kv_center");
}

// The checks and the launches of rtv_attn_fwd_fp8 (kv_splits == 1, no workspace) and of rtv_attn_fwd_fp8_split.
static int attn_fwd_fp8_launch(const char* who, const void* q, const void* k8, const void* v8t, void* o, int Lq, int H, int cache_rows,
                               int row0, int n0, int row1, int n1, int64_t q_row_stride, int64_t o_row_stride, float scale,
                               float k_scale, float v_scale, int causal_block, int q_offset, int kv_splits, void* workspace,
                               size_t workspace_bytes, rtv_stream_t stream) {
  auto fail = [&](const char* what) { return set_error(-1, (std::string(who) + ": " + what).c_str()); };
  if (!q || !k8 || !v8t || !o) return fail("null pointer");
  if (((uintptr_t)q | (uintptr_t)k8 | (uintptr_t)v8t | (uintptr_t)o) & 15) return fail("base pointers must be 16-byte aligned");
  if (Lq <= 0 || H <= 0 || n0 <= 0 || cache_rows <= 0) return fail("Lq, H, n0 and cache_rows must be positive");
  if (n1 < 0) return fail("negative segment length");
  if (causal_block < 0 || q_offset < 0) return fail("negative mask parameters");
  if (causal_block > 0 && n1 > 0) return fail("the block-causal mask needs a one-segment window");
  if (row0 < 0 || (int64_t)row0 + n0 > cache_rows || (n1 > 0 && (row1 < 0 || (int64_t)row1 + n1 > cache_rows)))
    return fail("key range outside [0, cache_rows)");
  if (q_row_stride < (int64_t)H * ATT_D || o_row_stride < (int64_t)H * ATT_D || ((q_row_stride | o_row_stride) & 7))
    return fail("row strides must be multiples of 8 elements and hold H heads");
  if (!good_scale(scale) || !good_scale(k_scale) || !good_scale(v_scale))
    return fail("scale, k_scale and v_scale must be finite and positive");
  if (kv_splits < 1 || kv_splits > 16) return fail("kv_splits must be 1..16");
  // never more ranges than storage tiles in the window; one range = the plain launch
  const int win_tiles = (((row0 + n0 - 1) >> 6) - (row0 >> 6) + 1) + (n1 > 0 ? ((row1 + n1 - 1) >> 6) - (row1 >> 6) + 1 : 0);
  if (kv_splits > win_tiles) kv_splits = win_tiles;
  af8::FwdParamsSplit p;
  p.q = (const uint16_t*)q;
  p.k8 = (const uint8_t*)k8;
  p.v8t = (const uint8_t*)v8t;
  p.o = (uint16_t*)o;
  p.Lq = Lq;
  p.H = H;
  p.cache_rows = cache_rows;
  p.row0 = row0;
  p.n0 = n0;
  p.row1 = n1 > 0 ? row1 : 0;
  p.n1 = n1;
  p.q_rs = q_row_stride;
  p.o_rs = o_row_stride;
  p.mult = scale * 1.4426950408889634f * k_scale;
  p.v_scale = v_scale;
  p.causal_block = causal_block;
  p.q_offset = q_offset;
  p.n_qtiles = (Lq + af8::QT - 1) / af8::QT;
  p.kv_splits = kv_splits;
  p.part_o = nullptr;
  p.part_ml = nullptr;
  if (kv_splits > 1) {
    const size_t rows = (size_t)kv_splits * H * Lq;
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < rows * (ATT_D + 2) * sizeof(float))
      return fail("split workspace missing, misaligned or too small (rtv_attn_split_workspace_bytes)");
    p.part_o = (float*)workspace;
    p.part_ml = p.part_o + rows * ATT_D;
  }
  const int64_t lkv = (int64_t)n0 + n1;
  ProfScope prof(PROF_ATTN, (hipStream_t)stream, 4.0 * Lq * (double)lkv * ATT_D * H * (causal_block > 0 ? 0.5 : 1.0));
  if (kv_splits == 1) {
    hipLaunchKernelGGL(attn_fwd_fp8_kernel<false>, dim3(H * p.n_qtiles), dim3(af8::NW * 64), 0, (hipStream_t)stream,
                       (const af8::FwdParams&)p);
    return check_launch(who);
  }
  hipLaunchKernelGGL(attn_fwd_fp8_kernel<true>, dim3(H * p.n_qtiles, kv_splits), dim3(af8::NW * 64), 0, (hipStream_t)stream, p);
  if (int st = check_launch(who)) return st;
  const int64_t nrows = (int64_t)H * Lq;
  hipLaunchKernelGGL(attn_fp8_combine_kernel, dim3((unsigned)((nrows + 15) / 16)), dim3(256), 0, (hipStream_t)stream, p.part_o,
                     p.part_ml, p.o, kv_splits, H, Lq, p.o_rs, v_scale);
  return check_launch("attn_fp8_combine");
}

extern "C" int rtv_attn_fwd_fp8(const void* q, const void* k8, const void* v8t, void* o, int Lq, int H, int cache_rows, int row0,
                                int n0, int row1, int n1, int64_t q_row_stride, int64_t o_row_stride, float scale, float k_scale,
                                float v_scale, int causal_block, int q_offset, rtv_stream_t stream) {
  return attn_fwd_fp8_launch("attn_fwd_fp8", q, k8, v8t, o, Lq, H, cache_rows, row0, n0, row1, n1, q_row_stride, o_row_stride, scale,
                             k_scale, v_scale, causal_block, q_offset, 1, nullptr, 0, stream);
}

extern "C" int rtv_attn_fwd_fp8_split(const void* q, const void* k8, const void* v8t, void* o, int Lq, int H, int cache_rows,
                                      int row0, int n0, int row1, int n1, int64_t q_row_stride, int64_t o_row_stride, float scale,
                                      float k_scale, float v_scale, int causal_block, int q_offset, int kv_splits, void* workspace,
                                      size_t workspace_bytes, rtv_stream_t stream) {
  return attn_fwd_fp8_launch("attn_fwd_fp8_split", q, k8, v8t, o, Lq, H, cache_rows, row0, n0, row1, n1, q_row_stride, o_row_stride,
                             scale, k_scale, v_scale, causal_block, q_offset, kv_splits, workspace, workspace_bytes, stream);
}
