// FP8 (OCP e4m3) projection GEMM with PER-ROW scales for gfx950 (include/rtv_hip_fp8_rows.h; torchao's PerRow granularity
// restated): y[m, n] = bf16( (q(x) . q(W)^T)[m, n] * s_x[m] * s_w[n] + bias[n] ), one scale per activation row and one per
// weight row (output channel); the quantisers are in fp8_rows.hip.
//
// The kernel is gemm_fp8.hip's gemm_fp8_kernel - same tiling, staging, schedule and split-K: both are gemm_fp8_body.h - with one
// change, in the de-quantise step behind the K loop: each accumulator is multiplied by s_x[row] and s_w[column] instead of one
// scalar.  The two kernels stay in translation units of their own (gemm_fp8_body.h says why); read the body for the schedule.
#include "gemm_fp8_body.h"

namespace rtv {

namespace gf8r {
struct Fp8Args {
  const uint8_t* A;      // [M][lda] e4m3
  const uint8_t* W;      // [N][ldw] e4m3
  int lda, ldw;          // bytes
  const float* a_scales;  // [M] device: s_x per row of this call (written by the quantisation kernel)
  const float* w_scales;  // [N] device: s_w per weight row = output column (16-byte aligned)
};
}  // namespace gf8r

__global__ __launch_bounds__(gf8::THREADS, 2) void gemm_fp8_rows_kernel(GemmParams p, gf8r::Fp8Args f, SplitArgs sp) {
  // de-quantise: (q(x) . q(W)^T)[m, n] * s_x[m] * s_w[n].  mb / nb = the lane's first output row / column (gemm_fp8_body.h has the
  // layout).  Rows >= M and columns >= N of edge tiles are never stored; their scale reads are clamped into the arrays
  // (N % 8 == 0, so a quad of columns is inside or outside as a whole).
  // Two multiplications per element, not one by a product: the compiler sinks this step into the six epilogue branches below, and
  // what stays live across them is then the 4 + 32 scales of a lane instead of their 128 products (which spilled).
  gf8::gemm_body(p, f, sp, [&](f32x16 (&acc)[4][2], int mb, int nb) {
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
  });
}

int launch_gemm_fp8_rows(GemmParams p, const uint8_t* A, int lda, const uint8_t* W, int ldw, const float* a_scales,
                         const float* w_scales, hipStream_t stream) {
  if (int st = gf8::prepare_launch(p, lda, ldw, "gemm_fp8_rows")) return st;
  if (((uintptr_t)a_scales & 3) || ((uintptr_t)w_scales & 15))
    return set_error(-1, "gemm_fp8_rows: a_row_scales must be 4-byte aligned, w_row_scales 16-byte aligned");
  static LdsAttr lds_attr;   // per device (a second GPU used from this process needs the attribute as well)
  if (int st = ensure_dynamic_lds((const void*)gemm_fp8_rows_kernel, gf8::LDS_BYTES, &lds_attr, "gemm_fp8_rows")) return st;
  SplitArgs sp;
  int grid = 0;
  if (int st = plan_split_k(p.tiles_m * p.tiles_n, p.K / gf8::BK, true, &sp, &grid, stream)) return st;
  gf8r::Fp8Args f{A, W, lda, ldw, a_scales, w_scales};
  ProfScope prof(PROF_GEMM, stream, 2.0 * p.M * (double)p.N * p.K);
  note_kernel(DK_GEMM_FP8_256x256);
  hipLaunchKernelGGL(gemm_fp8_rows_kernel, dim3(grid), dim3(gf8::THREADS), gf8::LDS_BYTES, stream, p, f, sp);
  return check_launch("gemm_fp8_rows");
}

}  // namespace rtv

using namespace rtv;

extern "C" int rtv_gemm_fp8_rows(const void* A, int lda, const void* W, int ldw, const float* a_row_scales,
                                 const float* w_row_scales, void* C, int ldc, int M, int N, int K, const void* bias, int act,
                                 const void* gate, int gate_stride, int rows_per_frame, int row_offset, const void* residual,
                                 int ldr, rtv_stream_t stream) {
  if (!A || !W || !C || !a_row_scales || !w_row_scales) return set_error(-1, "gemm_fp8_rows: null pointer");
  const GemmParams p = gemm_params(nullptr, lda, nullptr, ldw, C, ldc, M, N, K, bias, act, gate, gate_stride, rows_per_frame, row_offset,
                                   residual, ldr);
  return launch_gemm_fp8_rows(p, (const uint8_t*)A, lda, (const uint8_t*)W, ldw, a_row_scales, w_row_scales, (hipStream_t)stream);
}
