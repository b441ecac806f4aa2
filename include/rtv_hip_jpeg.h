/* Frame delivery side of librtv_hip.so: decoder pixels -> complete JPEG files, on the device.  The reference's frame callback
 * (release_server.py:970-1007) downloads a block's pixels and runs `TF.to_pil_image(...).save(format='JPEG', quality=90)` per
 * frame on a CPU thread pool; rtv_jpeg_encode produces the files in front of the copy.  Same conventions as rtv_hip.h: device
 * pointers unless stated, 0 = success, non-zero = failure with the reason in rtv_last_error(), every launch goes to `stream`.
 *
 * This is a header of its own for the reason rtv_hip_io.h is: the declarations were added without a new ABI revision, nothing
 * here changes a struct layout, RTV_ABI_VERSION stays as it is.
 *
 * The stream format (fixed):
 *   - baseline sequential DCT JFIF (ITU-T T.81, JFIF 1.01), 8 bit, Y Cb Cr with the JFIF full-range BT.601 matrix, 4:2:0
 *     (Y 2x2, Cb and Cr 1x1, chroma = the mean of each 2x2 block): what PIL writes at quality 90;
 *   - quantisation tables: T.81 Annex K.1 / K.2 scaled by libjpeg's rule (scale = 5000 / q below 50, else 200 - 2q;
 *     (base * scale + 50) / 100 clamped to 1..255); Huffman tables: the four "typical" tables of Annex K.3 - K.6;
 *   - restart interval = one MCU row (DRI = ceil(W / 16)), RST0..7 cycling between the rows: every MCU row is an entropy segment
 *     of its own (DC predictors reset, last byte padded with 1 bits, 0xFF stuffed with 0x00), which is the parallelism;
 *   - H and W are multiples of 8, SOF0 has the true size; where one is 8 mod 16 the far half of the edge MCUs replicates the last
 *     pixel column / row for the chroma means, and the luma blocks that lie wholly outside the picture are dummy blocks as libjpeg
 *     codes them (no AC, the DC of the block coded before them): a decoder drops their pixels, so they cost 6 bits, not a column's
 *     worth of coefficients (replicated luma made small frames up to 13 % larger than PIL's);
 *   - forward DCT in fp32 on the level-shifted samples, quantisation rounds half away from zero (not libjpeg's integer DCT).
 * Segments in order: SOI, APP0, DQT (luma), DQT (chroma), SOF0, DHT x 4 (DC luma, AC luma, DC chroma, AC chroma), DRI, SOS. */
#ifndef RTV_HIP_JPEG_H
#define RTV_HIP_JPEG_H
#include <stddef.h>
#include <stdint.h>

#include "rtv_hip_io.h"
#ifdef __cplusplus
extern "C" {
#endif

/* HOST only, no device call: everything of the file in front of the entropy-coded data, SOI .. SOS, into host_buf (cap bytes).
 * Returns the length (629); 0 with rtv_last_error() set for a null buffer, a cap that is too small, quality outside 1..100, or
 * H / W that are not positive multiples of 8 up to 65528. */
size_t rtv_jpeg_header(int quality, int H, int W, void* host_buf, size_t cap);

/* Bytes of scratch ("arena") one rtv_jpeg_encode / rtv_jpeg_coefficients call of T frames needs; 0 for sizes those refuse. */
size_t rtv_jpeg_arena_bytes(int T, int H, int W);

/* The provable upper bound of what T frames can take in `out` (every coefficient at its longest code, every byte stuffed):
 * a buffer of this size cannot overflow.  0 for sizes rtv_jpeg_encode refuses.  Real frames take a few percent of it. */
size_t rtv_jpeg_out_bound(int T, int H, int W);

/* T frames -> T JPEG files back to back in out; offsets = int64 [T + 1], file t is out[offsets[t] .. offsets[t + 1]).
 * pixels: fp32 planar [T][3][H][W] in [-1, 1] (pixels_are_rgb8 == 0; 16-byte aligned; the byte of a sample is made exactly as
 * rtv_pixels_to_rgb8 makes it, so encoding the floats and encoding their rgb8 give identical files) or rgb8 [T][H][W][3]
 * (pixels_are_rgb8 != 0, no alignment asked).  arena: rtv_jpeg_arena_bytes(T, H, W) bytes, 16-byte aligned, contents irrelevant
 * before and undefined after.  Three launches on `stream`, no synchronisation and no allocation inside.
 *
 * Nothing is written at or beyond out + out_cap, and the offsets always hold the TRUE sizes: offsets[T] > out_cap tells the
 * caller that the files are truncated and the call is to be repeated with a larger buffer (rtv_jpeg_out_bound never is).
 * Refused before any launch: a null pointer, non-positive sizes, H or W not multiples of 8 (or above 65528), quality outside
 * 1..100, T above RTV_FRAMES_MAX, an arena that is too small or misaligned, misaligned float pixels.  T == 0 returns 0. */
int rtv_jpeg_encode(const void* pixels, int pixels_are_rgb8, int T, int H, int W, int quality, void* arena, size_t arena_bytes,
                    void* out, size_t out_cap, void* offsets, rtv_stream_t stream);

/* Unit-test hook (like rtv_taehv_conv): the first stage of rtv_jpeg_encode alone - bytes, Y Cb Cr, chroma mean, DCT, quantisation -
 * and a copy of its result to coefficients = int16 [T][mcu_rows][mcus][6][64] (mcu_rows = ceil(H / 16), mcus = ceil(W / 16); the
 * six blocks of an MCU in scan order Y00 Y01 Y10 Y11 Cb Cr, each in zigzag order).  Same refusals as rtv_jpeg_encode. */
int rtv_jpeg_coefficients(const void* pixels, int pixels_are_rgb8, int T, int H, int W, int quality, void* arena,
                          size_t arena_bytes, void* coefficients, rtv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
