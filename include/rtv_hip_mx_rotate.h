/* Block Hadamard rotation in front of the MXFP4 / MXFP6 quantisers (rtv_dit_config.use_fp8 == 5: MXFP4 rotated, 6: MXFP6 rotated;
 * include/rtv_hip_mxfp4.h, include/rtv_hip_mxfp6.h).  Opt-in, like the modes it goes with.  With the Sylvester Hadamard matrix H of
 * order 32 (entries +-1, H H^T = 32 I), (x H)(W H)^T = 32 x W^T over every block of 32 K elements: the product of a Linear is
 * unchanged, and each operand's energy is spread evenly over the block before the block's shared exponent is chosen, so that one
 * outlier channel no longer pushes the block's other 31 values into the last steps of the element format.  The rotation spans
 * exactly one MX block, which a quad of lanes holds in the quantisers: no extra pass over memory, and neither GEMM changes.  A
 * header of its own, like rtv_hip_mxfp6.h: nothing here changes a signature or a layout of rtv_hip.h or of the two format headers.
 *
 * ARITHMETIC (part of the ABI; tests/mx_rotate_oracle.py is the restatement).  For each block of 32 consecutive K elements, index
 * k = 0..31 inside the block, inputs bf16:
 *   1. the 32 values as fp32
 *   2. for b = 0, 1, 2, 3, 4, in this order: for every pair (k, k | 1 << b) with bit b of k clear, (u, v) -> (u + v, u - v); fp32
 *      adds and subtracts, round to nearest even, nothing fused.  (The order is pinned because fp32 rounds once a block spans more
 *      than 16 binades.)
 *   3. times 2^-shift, exact.  1 / 32 = 2^-3 * 2^-2: a model rotates activations at RTV_MX_ROT_ACT_SHIFT and weights at
 *      RTV_MX_ROT_WEIGHT_SHIFT, so that the product of the two rotated operands is the product of the plain ones.
 *   4. the fp32 results are quantised by the format's floor rule, unchanged: E from the fp32 exponent field of the block maximum,
 *      code = the nearest magnitude of the scaled value, ties to even, saturating.
 * Storage of codes and scales is that of rtv_hip_mxfp4.h / rtv_hip_mxfp6.h; rtv_gemm_mxfp4 / rtv_gemm_mxfp6 multiply them.
 * Inputs are finite; a block whose butterflies would leave fp32's normal range is outside the contract. */
#ifndef RTV_HIP_MX_ROTATE_H
#define RTV_HIP_MX_ROTATE_H
#include "rtv_hip.h"

#define RTV_MX_ROT_BLOCK 32
#define RTV_MX_ROT_ACT_SHIFT 3
#define RTV_MX_ROT_WEIGHT_SHIFT 2
#define RTV_MX_ROT_MAX_SHIFT 5

#ifdef __cplusplus
extern "C" {
#endif

/* rtv_quantize_mxfp4 / rtv_quantize_mxfp6 (same arguments, same checks, same error strings) on the rotated blocks, scaled by
 * 2^-shift; 0 <= shift <= RTV_MX_ROT_MAX_SHIFT. */
int rtv_quantize_mxfp4_rot(const void* x, int64_t ld, int M, int d, void* codes, int64_t ld_codes, void* scales, int64_t ld_scales,
                           int shift, rtv_stream_t stream);
int rtv_quantize_mxfp6_rot(const void* x, int64_t ld, int M, int d, void* codes, int64_t ld_codes, void* scales, int64_t ld_scales,
                           int shift, rtv_stream_t stream);

/* rtv_layernorm_modulate (same arguments, same rounding points) followed by rtv_quantize_mx*_rot at shift = RTV_MX_ROT_ACT_SHIFT on
 * its bf16 result, in one kernel and bit for bit.  Arguments and checks of rtv_layernorm_modulate_mxfp4 / _mxfp6. */
int rtv_layernorm_modulate_mxfp4_rot(const void* x, void* codes, int64_t ld_codes, void* scales, int64_t ld_scales, int M, int d,
                                     float eps, const void* shift, const void* scale, int frame_stride, int rows_per_frame,
                                     int row_offset, const void* weight, const void* bias, rtv_stream_t stream);
int rtv_layernorm_modulate_mxfp6_rot(const void* x, void* codes, int64_t ld_codes, void* scales, int64_t ld_scales, int M, int d,
                                     float eps, const void* shift, const void* scale, int frame_stride, int rows_per_frame,
                                     int row_offset, const void* weight, const void* bias, rtv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
