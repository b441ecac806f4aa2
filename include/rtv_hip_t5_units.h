/* Unit entry points of the text encoder's kernels (realtime_video_amd/csrc/t5_encoder.hip): one thin launcher per kernel, for
 * tests/test_t5_kernels_gpu.py.  rtv_t5_encode (include/rtv_hip.h) launches the same kernels through the same helpers, with the
 * same grids and block sizes, so what a test runs here is what the product runs.  A header of its own, like rtv_hip_mx_rotate.h:
 * nothing here changes a signature or a layout of rtv_hip.h, and RTV_ABI_VERSION stays.
 *
 * Every pointer is a device address.  Each launcher checks its arguments (the alignments the kernels' vector loads need, the
 * divisibility their loops assume) and reports through rtv_last_error like the rest of the library; the kernels themselves have
 * no per-element bounds, so the extents below are the caller's promise. */
#ifndef RTV_HIP_T5_UNITS_H
#define RTV_HIP_T5_UNITS_H
#include "rtv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* x[r] = float32(table[clamp(r < valid ? ids[r] : 0, 0, vocab - 1)]) for r < rows.  ids: int32 [valid]; table: bf16 [vocab][dim],
 * 16-byte aligned; x: float32 [rows][dim], 16-byte aligned; dim % 8 == 0; 0 <= valid <= rows. */
int rtv_t5_embed(const int* ids, const void* table, void* x, int rows, int valid, int dim, int vocab, rtv_stream_t stream);

/* T5LayerNorm: out[r] = w * (x[r] * rsqrt(mean(x[r]^2) + eps)) in float32.  x: float32 [rows][dim], 16-byte aligned; w: bf16
 * [dim]; out: bf16 [rows][dim], 8-byte aligned (out_f32 == 0) or float32 [rows][dim], 16-byte aligned (out_f32 == 1);
 * dim % 4 == 0. */
int rtv_t5_rmsnorm(const void* x, const void* w, void* out, int rows, int dim, float eps, int out_f32, rtv_stream_t stream);

/* x (float32 [n]) += y (bf16 [n]); n % 8 == 0, both 16-byte aligned. */
int rtv_t5_add(void* x, const void* y, size_t n, rtv_stream_t stream);

/* h[r][c] = bf16(fc1 * gelu_tanh(gate)) from gf = [rows][gate (dff) | fc1 (dff)], bf16; h: bf16 [rows][dff]; dff % 8 == 0, both
 * 16-byte aligned. */
int rtv_t5_geglu(const void* gf, void* h, int rows, int dff, rtv_stream_t stream);

/* o[i][h] = softmax_j(q[i][h] . k[j][h] + bias[h][j - i + max_len - 1]) v[j][h] over the keys j < valid, head_dim 64, no
 * 1 / sqrt(d) scaling, for every query row i < rows.  qk: bf16 [rows][2 * 64 * num_heads], q columns then k columns, 16-byte
 * aligned; vt: bf16 [64 * num_heads][rows], V transposed, 8-byte aligned; o: bf16 [rows][64 * num_heads], 8-byte aligned; bias:
 * float32 [num_heads][2 * max_len - 1].  rows % 32 == 0, 0 < valid <= rows, valid <= max_len.
 * Rows at and behind `valid` are padding: their K is never used (a NaN there is harmless), their V^T columns must be FINITE (the PV
 * product multiplies them by P = 0), and as queries they look the table up at the last valid row's distances - never outside the
 * table - and give finite, otherwise unspecified output. */
int rtv_t5_attention(const void* qk, const void* vt, void* o, const void* bias, int rows, int valid, int num_heads, int max_len,
                     rtv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
