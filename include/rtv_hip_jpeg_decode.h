/* Frame input side of librtv_hip.so, second half: a camera's JPEG file -> the rgb8 frame rtv_frames_from_rgb8 reads, on the
 * device.  The reference's push_frame (release_server.py:470-487) takes what a browser sends, a JPEG file, and decodes it with PIL on
 * the CPU; rtv_jpeg_decode takes the file as it arrived.  Same conventions as rtv_hip.h: device pointers unless stated, 0 = success,
 * non-zero = failure with the reason in rtv_last_error(), every launch goes to `stream`, no allocation and no synchronisation inside.
 *
 * A header of its own for the reason rtv_hip_io.h and rtv_hip_jpeg.h are: nothing here changes a struct layout of the ABI,
 * RTV_ABI_VERSION stays as it is.
 *
 * Streams accepted: baseline sequential DCT (SOF0), 8 bit, Huffman, ONE interleaved scan; 1 component (grey, delivered as
 * R = G = B) or 3 components Y Cb Cr with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1; any Huffman tables (ids 0 and 1, as baseline
 * allows); up to four 8-bit quantisation tables; any width and height up to RTV_JPEG_DECODE_MAX_SIDE; with or without a restart
 * interval.  Everything else is refused by rtv_jpeg_parse, with the reason, before anything touches the device.
 *
 * Arithmetic: libjpeg's defaults, all integer - the "islow" inverse DCT of jidctint.c on the dequantised coefficients, "fancy"
 * triangle-filter chroma upsampling (h2v1, h2v2, edges replicated) and the fixed-point Y Cb Cr -> RGB tables of jdcolor.c - so
 * the pixels equal PIL's `Image.open(...).convert("RGB")` byte for byte on an undamaged file.
 *
 * A damaged scan never reads outside the file, never writes outside the arena or the frame and never loops without a bound: the
 * first code that is in no table, zigzag index past 63, marker where none belongs or block too many ends that frame's entropy
 * decode, the blocks not reached keep zero coefficients, and the frame's status word says what happened (RTV_JPEG_STATUS_*). */
#ifndef RTV_HIP_JPEG_DECODE_H
#define RTV_HIP_JPEG_DECODE_H
#include <stddef.h>
#include <stdint.h>

#include "rtv_hip_io.h"
#ifdef __cplusplus
extern "C" {
#endif

#define RTV_JPEG_DECODE_MAX_SIDE 4096          /* width and height rtv_jpeg_parse accepts */
#define RTV_JPEG_DECODE_MAX_FILE 8388608       /* file bytes rtv_jpeg_parse accepts (8 MiB) */
#define RTV_JPEG_HUFF_WORDS 228                /* one Huffman table in the kernel's form, in 32-bit words */

/* status word of a frame: 0 = clean, else the OR of */
#define RTV_JPEG_STATUS_BAD_CODE 1             /* a bit pattern that is no code of the table in force */
#define RTV_JPEG_STATUS_ZIGZAG 2               /* a run that leads past coefficient 63 */
#define RTV_JPEG_STATUS_BLOCKS 4               /* more blocks than the frame, or than a restart interval, has */
#define RTV_JPEG_STATUS_MARKER 8               /* a restart marker inside a block, or not where the restart interval puts it */
#define RTV_JPEG_STATUS_SHORT 16               /* the scan ended before the frame's last block */

/* What rtv_jpeg_parse makes of a file's marker segments: plain data, little-endian, sizeof = 4496 (a multiple of 16).  A frame on
 * the DEVICE is this struct followed by the file's bytes ("descriptor plus file"): the kernels read the tables from that copy.
 *   quant[c]: the quantiser steps of component c, natural (row-major) order.
 *   huff[0], huff[1]: DC tables 0 and 1; huff[2], huff[3]: AC tables 0 and 1; comp_dc[c] / comp_ac[c]: which of them component c
 *   uses.  One table = 256 uint16 (index = the next 8 bits of the stream; (code length << 8) | symbol, 0 = longer than 8 bits),
 *   17 uint32 limit[l] (the first 16-bit-left-aligned code value that is longer than l bits), 17 int32 offset[l] (index of a
 *   length-l code's symbol = offset[l] + code), 256 uint8 symbols in code order, 2 words of padding. */
typedef struct {
  int height, width, components, hsamp, vsamp, restart_interval;   /* hsamp x vsamp: luma blocks per MCU (1x1 for grey) */
  int mcu_cols, mcu_rows, blocks_per_mcu;
  int scan_offset, scan_bytes, file_bytes;     /* the entropy-coded data is file[scan_offset .. scan_offset + scan_bytes) */
  int comp_dc[3], comp_ac[3];
  int quant[3][64];
  int huff[4][228];                            /* [4][RTV_JPEG_HUFF_WORDS] */
  int reserved[2];
} rtv_jpeg_desc;

/* HOST only, no device call: the marker segments of `file` (host memory, file_bytes bytes) -> *desc.  Returns 0, or non-zero with
 * the reason in rtv_last_error(): a null argument; no SOI; progressive, extended, lossless or arithmetic coding (any SOFn but
 * SOF0); 12-bit samples; a 16-bit quantisation table; 2, 4 or more components; sampling factors other than those above; more than
 * one scan, or a scan that is not the full 0..63 interleaved one; an Adobe APP14 marker with transform 0 on a 3-component file
 * (RGB, not Y Cb Cr); a quantisation or Huffman table the scan names but the file does not define; a malformed Huffman table; a
 * header that is cut short or malformed; width or height 0 or above RTV_JPEG_DECODE_MAX_SIDE; a file above
 * RTV_JPEG_DECODE_MAX_FILE. */
int rtv_jpeg_parse(const void* file, size_t file_bytes, rtv_jpeg_desc* desc);

/* Bytes of scratch ("arena") one rtv_jpeg_decode call needs for the T frames descs[0 .. T) (HOST array): their coefficient planes.
 * 0 for T outside 1..RTV_FRAMES_MAX or a descriptor rtv_jpeg_decode refuses. */
size_t rtv_jpeg_decode_arena_bytes(const rtv_jpeg_desc* descs, int T);

/* T frames, which may differ in size and sampling -> rgb8 [height][width][3] each, cropped to the true size.
 * descs: HOST array [T], as rtv_jpeg_parse wrote them.  frames: HOST array [T] of DEVICE pointers, each to a frame's descriptor
 * plus file (sizeof(rtv_jpeg_desc) + file_bytes bytes, 16-byte aligned).  rgb8: HOST array [T] of DEVICE pointers to the outputs
 * (no alignment asked).  status: int32 [T] on the device, RTV_JPEG_STATUS_* per frame.  rounds: int32 [T] on the device or NULL:
 * the synchronisation rounds the frame's entropy decode took (a measurement).  subseq_bits: bits of the scan one thread decodes,
 * 0 = the default (512), otherwise a multiple of 32 no smaller than 32; it is raised per frame so that a scan has at most 1024
 * subsequences.  arena: rtv_jpeg_decode_arena_bytes(descs, T) bytes, 16-byte aligned, contents irrelevant before and undefined
 * after.  Two launches on `stream`: entropy decode (one workgroup of 1024 threads per frame) and the fused dequantisation,
 * inverse DCT, upsampling and colour conversion.
 * Refused before any launch: a null pointer, T above RTV_FRAMES_MAX, a descriptor whose fields contradict each other or exceed
 * the caps, a misaligned frame or arena, an arena that is too small, a bad subseq_bits.  T == 0 returns 0. */
int rtv_jpeg_decode(const rtv_jpeg_desc* descs, const void* const* frames, void* const* rgb8, int T, int subseq_bits, void* arena,
                    size_t arena_bytes, void* status, void* rounds, rtv_stream_t stream);

/* Unit-test hook (as rtv_jpeg_coefficients is for the encoder): the entropy decode of ONE frame alone.  coefficients: the quantised
 * coefficients as int16, component after component, each [block_rows][block_cols][64] in natural order over the padded block grid
 * (component 0: mcu_rows * vsamp x mcu_cols * hsamp blocks, the others mcu_rows x mcu_cols), DC terms rebuilt;
 * rtv_jpeg_decode_arena_bytes(desc, 1) bytes.  status, rounds: int32 [1].  Same refusals as rtv_jpeg_decode. */
int rtv_jpeg_decode_coefficients(const rtv_jpeg_desc* desc, const void* frame, int subseq_bits, void* arena, size_t arena_bytes,
                                 void* coefficients, void* status, void* rounds, rtv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
