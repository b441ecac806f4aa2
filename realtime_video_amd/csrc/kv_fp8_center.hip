// K smoothing on the e4m3-only KV cache (include/rtv_hip_attn_fp8_only_center.h): the kernels that keep a compact cache under a centre
// without a bf16 K row to go back to.  (The centred row writer is the CENTER instantiation of qk_norm_rope_k8_kernel, kv_fp8.hip.)
//
//   attn_k8_center_*_kernel    attn_kv_center_*_kernel (attn_fp8.hip) reading codes: the same chunks, the same order of additions.
//   attn_k8_recenter_kernel    a read-once / write-once byte kernel: 16-byte pieces, the thread's 16 deltas in registers over the rows
//                              it walks (yardstick: the 4.7 TB/s copy rate noted in elementwise.hip).
#include <cmath>

#include "../../include/rtv_hip_attn_fp8_only_center.h"
#include "attn_common.h"
#include "fp8_quant.h"
#include "rtv_common.h"
#include "rtv_internal.h"

namespace rtv {

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
  block_max_stage(kmax, s_max);
  __syncthreads();
  if (tid == 0) block_max_commit(s_max, p.amax);
}

}  // namespace rtv

using namespace rtv;

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
