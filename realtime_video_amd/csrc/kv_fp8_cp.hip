// The e4m3-only KV cache under the row exchange of context parallelism (include/rtv_hip_attn_fp8_only_cp.h): the exchange carries
// codes.  Two kernels around the all-gather of the staging buffer kv8 [world][2][M / world][H * 128]:
//
//   stage_v_rows_kernel   the V half of STAGE: bf16 V rows of the projection buffer -> e4m3 codes, row-major, with the rounding of
//                         attn_quantize_v_rows_kernel (kv_fp8.hip).  16 values per thread: two 16-byte loads, one 16-byte store.
//                         (The K half is qk_norm_rope_k8_kernel itself, launched with the K rows of the rank's segment as its k8.)
//   commit_kv8_kernel     COMMIT: one workgroup per (storage tile, head) of one physical row segment.  K: the rows' 128 bytes of the
//                         head copied as 16-byte pieces.  V: the thread layout, the LDS image and the partial-tile rule of
//                         attn_quantize_v_rows_kernel, reading codes instead of bf16 values.  A byte mover.
// Both are read-once / write-once kernels (yardstick: the copy rate noted in elementwise.hip).
#include <cmath>

#include "../../include/rtv_hip_attn_fp8_only.h"
#include "../../include/rtv_hip_attn_fp8_only_cp.h"
#include "attn_common.h"
#include "fp8_quant.h"
#include "rtv_common.h"
#include "rtv_internal.h"

namespace rtv {

struct StageVArgs {
  const uint16_t* v;   // source row 0 (the V third of the projection buffer)
  int64_t rs;          // its row stride in elements
  uint8_t* dst;        // destination row 0, row stride d bytes
  int rows, d16;       // d / 16: 16-value pieces per row
  float v_scale;
  unsigned* amax;      // float[2]; [1] is V's
};

__global__ __launch_bounds__(256) void stage_v_rows_kernel(StageVArgs p) {
  __shared__ float s_max[4];
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float vmax = 0.f;
  if (idx < (int64_t)p.rows * p.d16) {
    const int row = (int)(idx / p.d16), c = (int)(idx - (int64_t)row * p.d16);
    const uint16_t* src = p.v + (size_t)row * p.rs + c * 16;
    const u32x4 r0 = *(const u32x4*)src, r1 = *(const u32x4*)(src + 8);
    float x[8], y[8];
    unpack_bf16x8(r0, x);
    unpack_bf16x8(r1, y);
#pragma unroll
    for (int j = 0; j < 8; ++j) vmax = fmaxf(vmax, fmaxf(fabsf(x[j]), fabsf(y[j])));
    const u32x2 c0 = quantize8(x, p.v_scale), c1 = quantize8(y, p.v_scale);
    *(u32x4*)(p.dst + ((size_t)row * p.d16 + c) * 16) = u32x4{c0[0], c0[1], c1[0], c1[1]};
  }
  if (p.amax == nullptr) return;   // kernel-uniform
  block_max_stage(vmax, s_max);
  __syncthreads();
  if (threadIdx.x == 0) block_max_commit(s_max, p.amax + 1);
}

struct CommitArgs {
  const uint8_t* kv8;
  uint8_t* k8;
  uint8_t* v8t;
  int S, H;               // rows per rank segment; heads
  int row0, rows, tile0;  // physical rows [row0, row0 + rows) of the cache; tile0 = row0 >> 6
  int g0;                 // row of the block (0 .. M - 1) that physical row row0 holds
};

// Row g of the block inside kv8, in rows of H * 128 bytes: rank g / S, K rows first, then V rows.
__device__ __forceinline__ size_t staged_k_row(int g, int S) {
  const int r = g / S;
  return (size_t)r * 2 * S + (g - r * S);
}

__global__ __launch_bounds__(256) void commit_kv8_kernel(CommitArgs p) {
  constexpr int LD = 17;   // words per dim row of the LDS image, as in attn_quantize_v_rows_kernel
  __shared__ __attribute__((aligned(16))) uint32_t sV[ATT_D * LD];
  const int tid = threadIdx.x;
  const int T = p.tile0 + blockIdx.x, h = blockIdx.y;
  const size_t d = (size_t)p.H * ATT_D;
  const int r_lo = max(p.row0 - T * ATT_KT, 0), r_hi = min(p.row0 + p.rows - T * ATT_KT, ATT_KT);   // tile-local rows to place
  // K: 64 rows x 8 pieces of 16 bytes
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int id = tid + it * 256, key = id >> 3, piece = id & 7;
    if (key >= r_lo && key < r_hi) {
      const int prow = T * ATT_KT + key;
      const size_t src = staged_k_row(p.g0 + prow - p.row0, p.S) * d + (size_t)h * ATT_D + piece * 16;
      *(u32x4*)(p.k8 + (size_t)prow * d + (size_t)h * ATT_D + piece * 16) = *(const u32x4*)(p.kv8 + src);
    }
  }
  // V: thread (kq, dc) = keys 4 kq .. 4 kq + 3 of the tile, dims 8 dc .. 8 dc + 7
  const int dc = tid & 15, kq = tid >> 4;
  uint32_t vw[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int key = 4 * kq + jj;
    if (key < r_lo || key >= r_hi) continue;
    const size_t src = (staged_k_row(p.g0 + T * ATT_KT + key - p.row0, p.S) + p.S) * d + (size_t)h * ATT_D + dc * 8;
    const u32x2 cv = *(const u32x2*)(p.kv8 + src);
#pragma unroll
    for (int dd = 0; dd < 8; ++dd) {
      const uint32_t w = dd < 4 ? cv[0] : cv[1];
      vw[dd] |= ((w >> (8 * (dd & 3))) & 0xffu) << (8 * jj);
    }
  }
  // keys 4 kq .. + 3 = (kb, i, g) = (kq >> 3, (kq >> 1) & 3, kq & 1), j = 0..3  ->  slots 32 g + 16 kb + 4 i + j = word 8 g + 4 kb + i
  const int word = 8 * (kq & 1) + 4 * (kq >> 3) + ((kq >> 1) & 3);
#pragma unroll
  for (int dd = 0; dd < 8; ++dd) sV[(dc * 8 + dd) * LD + word] = vw[dd];
  __syncthreads();
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

extern "C" int rtv_attn_fp8_stage_kv8(const void* qkv, void* kv8, int world, int row_begin, int row_count, float k_scale, float v_scale,
                                      void* amax, int d, int num_heads, float eps, const void* wk, const void* rope_cs, int F, int gh,
                                      int gw, int start_frame, rtv_stream_t stream) {
  if (!qkv || !kv8 || !wk || !rope_cs) return set_error(-1, "attn_fp8_stage_kv8: null pointer");
  if (((uintptr_t)qkv | (uintptr_t)kv8 | (uintptr_t)wk) & 15) return set_error(-1, "attn_fp8_stage_kv8: qkv, kv8 and wk must be 16-byte aligned");
  if (((uintptr_t)rope_cs & 7) || ((uintptr_t)amax & 3)) return set_error(-1, "attn_fp8_stage_kv8: rope_cs must be 8-byte, amax 4-byte aligned");
  const int64_t M = (int64_t)F * gh * gw;
  if (F <= 0 || gh <= 0 || gw <= 0 || M > INT32_MAX) return set_error(-1, "attn_fp8_stage_kv8: empty token grid");
  if (world <= 0 || M % world) return set_error(-1, "attn_fp8_stage_kv8: M = F * gh * gw must be a multiple of world");
  const int S = (int)(M / world);
  if (row_begin < 0 || row_count <= 0 || (int64_t)row_begin + row_count > M) return set_error(-1, "attn_fp8_stage_kv8: rows outside [0, M)");
  const int seg = row_begin / S;
  if ((row_begin + row_count - 1) / S != seg) return set_error(-1, "attn_fp8_stage_kv8: the rows must lie in one rank's segment");
  if (num_heads <= 0 || num_heads > 65535 || d != num_heads * ATT_D) return set_error(-1, "attn_fp8_stage_kv8: head_dim must be 128");
  if (!good_scale(k_scale) || !good_scale(v_scale)) return set_error(-1, "attn_fp8_stage_kv8: scales must be finite and positive");
  // K: the writer of the unsharded compact forward on a dense k8 of (seg + 1) * S rows that starts seg * S rows into kv8 - its row
  // row_begin + i is row seg * 2 S + (row_begin + i - seg * S) of kv8, the K rows of the segment.  (wq is not read without a q role.)
  uint8_t* const base = (uint8_t*)kv8;
  if (int s = rtv_qk_norm_rope_k8(qkv, nullptr, base + (size_t)seg * S * d, (seg + 1) * S, k_scale, amax, 0, row_count, d, num_heads, eps,
                                  wk, wk, rope_cs, F, gh, gw, start_frame, row_begin, 0, 0, 0, stream))
    return s;
  StageVArgs p;
  p.v = (const uint16_t*)qkv + 2 * d;
  p.rs = 3 * (int64_t)d;
  p.dst = base + ((size_t)seg * 2 * S + S + (row_begin - seg * S)) * d;
  p.rows = row_count;
  p.d16 = d / 16;
  p.v_scale = v_scale;
  p.amax = (unsigned*)amax;
  const int64_t total = (int64_t)row_count * p.d16;
  ProfScope prof(PROF_MISC, (hipStream_t)stream, 3.0 * row_count * d);
  hipLaunchKernelGGL(stage_v_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
  return check_launch("attn_fp8_stage_kv8");
}

extern "C" int rtv_attn_fp8_commit_kv8(const void* kv8, int world, int M, int H, void* k8, void* v8t, int cache_rows, int cache_row0,
                                       int ring_lo, int ring_size, int ring_shift, rtv_stream_t stream) {
  if (!kv8 || !k8 || !v8t) return set_error(-1, "attn_fp8_commit_kv8: null pointer");
  if (((uintptr_t)kv8 | (uintptr_t)k8 | (uintptr_t)v8t) & 15) return set_error(-1, "attn_fp8_commit_kv8: kv8, k8 and v8t must be 16-byte aligned");
  if (world <= 0 || M <= 0 || M % world) return set_error(-1, "attn_fp8_commit_kv8: M must be positive and a multiple of world");
  if (H <= 0 || H > 65535) return set_error(-1, "attn_fp8_commit_kv8: H must be 1..65535");
  if (cache_rows <= 0 || cache_row0 < 0) return set_error(-1, "attn_fp8_commit_kv8: cache_rows must be positive, cache_row0 non-negative");
  if (ring_size < 0 || ring_lo < 0 || ring_shift < 0 || (ring_size > 0 && ring_shift >= ring_size))
    return set_error(-1, "attn_fp8_commit_kv8: bad ring (need ring_lo >= 0, 0 <= ring_shift < ring_size)");
  const int64_t end = (int64_t)cache_row0 + M;
  if (ring_size > 0 ? ((int64_t)ring_lo + ring_size > cache_rows || end > (int64_t)ring_lo + ring_size) : end > cache_rows)
    return set_error(-1, "attn_fp8_commit_kv8: row range outside [0, cache_rows)");
  // the physical segments of the logical rows, in their order: sink rows in place, ring rows rotated, at most one wrap (the ring
  // rows of the block are at most cache_row0 + M - ring_lo <= ring_size: they never meet themselves)
  int seg[3][2], ns = 0, a = cache_row0, n = M;
  if (ring_size <= 0) {
    seg[ns][0] = a, seg[ns++][1] = n;
  } else {
    if (a < ring_lo) {
      const int m = n < ring_lo - a ? n : ring_lo - a;
      seg[ns][0] = a, seg[ns++][1] = m;
      a += m, n -= m;
    }
    if (n > 0) {
      const int p0 = ring_lo + (a - ring_lo + ring_shift) % ring_size;
      const int first = n < ring_lo + ring_size - p0 ? n : ring_lo + ring_size - p0;
      seg[ns][0] = p0, seg[ns++][1] = first;
      if (n > first) seg[ns][0] = ring_lo, seg[ns++][1] = n - first;
    }
  }
  CommitArgs p;
  p.kv8 = (const uint8_t*)kv8;
  p.k8 = (uint8_t*)k8;
  p.v8t = (uint8_t*)v8t;
  p.S = M / world;
  p.H = H;
  p.g0 = 0;
  for (int i = 0; i < ns; ++i) {
    p.row0 = seg[i][0];
    p.rows = seg[i][1];
    p.tile0 = p.row0 >> 6;
    const int tiles = ((p.row0 + p.rows - 1) >> 6) - p.tile0 + 1;
    ProfScope prof(PROF_MISC, (hipStream_t)stream, 4.0 * p.rows * H * ATT_D);
    hipLaunchKernelGGL(commit_kv8_kernel, dim3(tiles, H), dim3(256), 0, (hipStream_t)stream, p);
    if (int s = check_launch("attn_fp8_commit_kv8")) return s;
    p.g0 += p.rows;
  }
  return 0;
}
