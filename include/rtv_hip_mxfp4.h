/* MXFP4 Linears (rtv_dit_config.use_fp8 == 3; include/rtv_hip.h): e2m1 codes with one e8m0 scale per 32 elements, multiplied by
 * v_mfma_scale_f32_32x32x64_f8f6f4 cbsz:4 blgp:4, which applies the block scales inside the MFMA.  A header of its own, like
 * rtv_hip_fp8_rows.h: nothing here changes a signature or a layout of rtv_hip.h.  Opt-in and never a reference mode (the reference
 * has no FP4 path); the pin is the restatement of the OCP Microscaling Formats v1.0 conversion in tests/mxfp4_oracle.py.
 *
 * Arithmetic, for a row of K bf16 values (K % 32 == 0, finite), block by block over 32 consecutive K elements:
 *   amax = max |x| over the block
 *   e    = clamp(floor(log2 amax) - 2, -127, 127)      (the floor rule; 2 = the largest exponent of e2m1)
 *   E    = e + 127, the block's scale byte (e8m0; 255 is never written).  An all-zero block: E = 0, codes 0.
 *   code = e2m1(x * 2^-e), round to nearest even, saturating at +-6.  A nibble is sign, 2 exponent bits, 1 mantissa bit:
 *          magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6.  (-0 and +0 are both produced; they are the same value.)
 *   y[m, n] = bf16(sum over blocks of 2^(ea + ew) * sum_k a_k w_k + bias[n]) with fp32 accumulation, then rtv_gemm's bf16 epilogue.
 * There is no de-quantise multiplication anywhere: the MFMA applies 2^(ea + ew).
 *
 * STORAGE (part of the ABI; tests/mxfp4_oracle.py holds the Python twin of the two macros):
 *   codes   [rows][ld_codes bytes]: two per byte in natural order - element 2j of the row in the low nibble of byte j, element
 *           2j + 1 in the high nibble.  The MFMA takes a lane's 32-element block as 16 consecutive bytes of this order
 *           (scripts/micro/mxfp4_mfma.hip: lane l holds row l & 31 and block l >> 5 of a 64-deep step; with both operands in the
 *           same order the order of the two nibbles of a byte cannot change a dot product, so natural order it is).
 *   scales  [rows][ld_scales bytes], one array per matrix.  In a 64-deep MFMA step st of a 256-element K-tile, lanes with
 *           g = lane >> 5 own block 2 st + g, and the scale the MFMA applies to a lane's block is byte `opsel` of that lane's scale
 *           register.  So the 8 scale bytes of a K-tile are stored lane half first: byte 4 g + st holds the scale of block
 *           2 st + g.  A lane then loads ONE aligned dword per row and K-tile (bytes 8 kt + 4 g .. + 4) and the MFMA of step st
 *           selects byte st.  Block b of a row lives at byte RTV_MXFP4_SCALE_POS(b); a row owns RTV_MXFP4_SCALE_BYTES(K) bytes
 *           (= K / 32 when K % 256 == 0; bytes of blocks a short last K-tile does not have are never written or read). */
#ifndef RTV_HIP_MXFP4_H
#define RTV_HIP_MXFP4_H
#include "rtv_hip.h"

#define RTV_MXFP4_BLOCK 32
/* byte of block b inside its row of scales */
#define RTV_MXFP4_SCALE_POS(b) (((b) & ~7) | (((b) & 1) << 2) | (((b) & 7) >> 1))
/* bytes a row of K elements occupies in a scales array: K / 32 rounded up to whole K-tiles of 8 blocks */
#define RTV_MXFP4_SCALE_BYTES(K) ((((K) / RTV_MXFP4_BLOCK) + 7) & ~7)
/* byte and shift of element k inside its row of codes */
#define RTV_MXFP4_CODE_BYTE(k) ((k) >> 1)
#define RTV_MXFP4_CODE_SHIFT(k) (((k) & 1) << 2)

#ifdef __cplusplus
extern "C" {
#endif

/* x [M, d] bf16 (row stride ld elements) -> codes [M][ld_codes bytes] and scales [M][ld_scales bytes] in the storage above.
 * One pass: the row stays in registers between the block maxima and the conversion; no memset, no atomics, no scratch.  The
 * weights of a model are quantised by this same kernel (one arithmetic).
 * d % 32 == 0, d <= 14336, ld % 8 == 0, ld >= d, ld_codes % 4 == 0, ld_codes >= d / 2, ld_scales >= RTV_MXFP4_SCALE_BYTES(d),
 * x 16-byte aligned, codes 4-byte aligned. */
int rtv_quantize_mxfp4(const void* x, int64_t ld, int M, int d, void* codes, int64_t ld_codes, void* scales, int64_t ld_scales,
                       rtv_stream_t stream);

/* rtv_layernorm_modulate (same arguments, same rounding points) followed by rtv_quantize_mxfp4 on its bf16 result, in one kernel
 * and bit for bit.  x [M, d] contiguous rows; codes / scales as above.  d % 32 == 0, d <= 8192. */
int rtv_layernorm_modulate_mxfp4(const void* x, void* codes, int64_t ld_codes, void* scales, int64_t ld_scales, int M, int d,
                                 float eps, const void* shift, const void* scale, int frame_stride, int rows_per_frame,
                                 int row_offset, const void* weight, const void* bias, rtv_stream_t stream);

/* C[M,N] bf16 = epilogue(sum over blocks 2^(ea + ew) * (A_codes . W_codes^T)): lda / ldw in bytes (multiples of 16, >= K / 2),
 * a_scales [M][K / 32] and w_scales [N][K / 32] bytes with DENSE rows (ld_scales == K / 32) and 4-byte aligned bases.
 * K % 256 == 0, N % 8 == 0.  A launch over a row range of a weight passes the matching slice of its codes and of its scales.
 * Epilogue arguments and the split-K workspace are rtv_gemm_fp8's. */
int rtv_gemm_mxfp4(const void* A_codes, int lda, const void* W_codes, int ldw, const void* a_scales, const void* w_scales, void* C,
                   int ldc, int M, int N, int K, const void* bias, int act, const void* gate, int gate_stride, int rows_per_frame,
                   int row_offset, const void* residual, int ldr, rtv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
