/* MXFP6 Linears (rtv_dit_config.use_fp8 == 4; include/rtv_hip.h): e2m3 codes with one e8m0 scale per 32 elements, multiplied by
 * v_mfma_scale_f32_32x32x64_f8f6f4 cbsz:2 blgp:2, which applies the block scales inside the MFMA and, on gfx950, issues in the cycles
 * of the FP4 form.  A header of its own, like rtv_hip_mxfp4.h: nothing here changes a signature or a layout of rtv_hip.h.  Opt-in and
 * never a reference mode (the reference has no FP6 path); the pin is the restatement of the OCP Microscaling Formats v1.0 conversion
 * in tests/mxfp6_oracle.py.
 *
 * Arithmetic, for a row of K bf16 values (K % 32 == 0, finite), block by block over 32 consecutive K elements:
 *   amax = max |x| over the block
 *   e    = clamp(floor(log2 amax) - 2, -127, 127)      (the floor rule; 2 = the largest exponent of e2m3)
 *   E    = e + 127, the block's scale byte (e8m0; 255 is never written).  An all-zero block: E = 0, codes 0.
 *   code = e2m3(x * 2^-e), round to nearest even, saturating at +-7.5.  A code is sign, 2 exponent bits, 3 mantissa bits:
 *          magnitudes k / 8 for k = 0..7 (subnormal) and (1 + m / 8) * 2^eps for eps = 0..2; as a number the 5 magnitude bits
 *          count the 32 magnitudes in increasing order.  (-0 and +0 are both produced; they are the same value.)
 *   y[m, n] = bf16(sum over blocks of 2^(ea + ew) * sum_k a_k w_k + bias[n]) with fp32 accumulation, then rtv_gemm's bf16 epilogue.
 * There is no de-quantise multiplication anywhere: the MFMA applies 2^(ea + ew).
 *
 * STORAGE (part of the ABI; tests/mxfp6_oracle.py holds the Python twin of the macros):
 *   codes   [rows][ld_codes bytes]: block b of a row is the 24 bytes [24 b, 24 b + 24), one little-endian 192-bit string with
 *           element j of the block at bits [6 j, 6 j + 6).  That is the register image of the MFMA (scripts/micro/mxfp6_mfma.hip:
 *           lane l holds row l & 31 and block l >> 5 of a 64-deep step in operand registers 0-5), so a block goes from memory to
 *           the matrix core without a shift.  A row of K elements is 3 K / 4 bytes.
 *   scales  [rows][ld_scales bytes], one array per matrix.  The GEMM's K-tile is 128 elements = 4 blocks = two 64-deep MFMA steps;
 *           in step st lanes with g = lane >> 5 own block 2 st + g, and the MFMA applies byte `opsel` of the lane's scale register.
 *           So the 4 scale bytes of a K-tile are stored lane half first: byte 2 g + st holds the scale of block 2 st + g.  A lane
 *           then loads ONE aligned 16-bit word per row and K-tile (bytes 4 kt + 2 g, + 1) and the MFMA of step st selects byte st.
 *           (rtv_hip_mxfp4.h's order is the same rule for its 8-block K-tile; with a 4-block tile that order would put a tile's two
 *           bytes in the low or the high half of a dword by the parity of the tile.)  Block b of a row lives at byte
 *           RTV_MXFP6_SCALE_POS(b); a row owns RTV_MXFP6_SCALE_BYTES(K) bytes (= K / 32 when K % 128 == 0; bytes of blocks a
 *           short last K-tile does not have are never written or read). */
#ifndef RTV_HIP_MXFP6_H
#define RTV_HIP_MXFP6_H
#include "rtv_hip.h"

#define RTV_MXFP6_BLOCK 32
#define RTV_MXFP6_BLOCK_BYTES 24
/* byte of block b inside its row of scales */
#define RTV_MXFP6_SCALE_POS(b) (((b) & ~3) | (((b) & 1) << 1) | (((b) & 3) >> 1))
/* bytes a row of K elements occupies in a scales array: K / 32 rounded up to whole K-tiles of 4 blocks */
#define RTV_MXFP6_SCALE_BYTES(K) ((((K) / RTV_MXFP6_BLOCK) + 3) & ~3)
/* bytes a row of K elements occupies in a codes array */
#define RTV_MXFP6_CODE_BYTES(K) ((K) / 4 * 3)
/* first bit of element k inside its row of codes (bit i of a row = bit i & 7 of byte i >> 3; a code may straddle two bytes) */
#define RTV_MXFP6_CODE_BIT(k) ((k) * 6)

#ifdef __cplusplus
extern "C" {
#endif

/* x [M, d] bf16 (row stride ld elements) -> codes [M][ld_codes bytes] and scales [M][ld_scales bytes] in the storage above.
 * One pass: the row stays in registers between the block maxima and the conversion; no memset, no atomics, no scratch.  The
 * weights of a model are quantised by this same kernel (one arithmetic).
 * d % 32 == 0, d <= 14336, ld % 8 == 0, ld >= d, ld_codes % 4 == 0, ld_codes >= 3 d / 4, ld_scales >= RTV_MXFP6_SCALE_BYTES(d),
 * x 16-byte aligned, codes 4-byte aligned. */
int rtv_quantize_mxfp6(const void* x, int64_t ld, int M, int d, void* codes, int64_t ld_codes, void* scales, int64_t ld_scales,
                       rtv_stream_t stream);

/* rtv_layernorm_modulate (same arguments, same rounding points) followed by rtv_quantize_mxfp6 on its bf16 result, in one kernel
 * and bit for bit.  x [M, d] contiguous rows; codes / scales as above.  d % 32 == 0, d <= 8192. */
int rtv_layernorm_modulate_mxfp6(const void* x, void* codes, int64_t ld_codes, void* scales, int64_t ld_scales, int M, int d,
                                 float eps, const void* shift, const void* scale, int frame_stride, int rows_per_frame,
                                 int row_offset, const void* weight, const void* bias, rtv_stream_t stream);

/* C[M,N] bf16 = epilogue(sum over blocks 2^(ea + ew) * (A_codes . W_codes^T)): lda / ldw in bytes (multiples of 16, >= 3 K / 4),
 * a_scales [M][K / 32] and w_scales [N][K / 32] bytes with DENSE rows (ld_scales == K / 32) and 4-byte aligned bases.
 * K % 128 == 0, N % 8 == 0.  A launch over a row range of a weight passes the matching slice of its codes and of its scales.
 * Epilogue arguments and the split-K workspace are rtv_gemm_fp8's. */
int rtv_gemm_mxfp6(const void* A_codes, int lda, const void* W_codes, int ldw, const void* a_scales, const void* w_scales, void* C,
                   int ldc, int M, int N, int K, const void* bias, int act, const void* gate, int gate_stride, int rows_per_frame,
                   int row_offset, const void* residual, int ldr, rtv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
