/* Pixel input side of librtv_hip.so: camera / decoder bytes -> the VAE encoder's input, the mirror image of rtv_pixels_to_rgb8
 * (include/rtv_hip.h).  Same conventions as rtv_hip.h: device pointers unless stated, 0 = success, non-zero = failure with the
 * reason in rtv_last_error(), every launch goes to `stream`.
 *
 * This is a header of its own only because the declarations were added without a new ABI revision: nothing here changes a
 * struct layout, RTV_ABI_VERSION stays as it is.  Folding it into rtv_hip.h is a later clean-up. */
#ifndef RTV_HIP_IO_H
#define RTV_HIP_IO_H
#include <stdint.h>

#include "rtv_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Frames one rtv_frames_from_rgb8 call can take (its slot table travels by value with the launch). */
#define RTV_FRAMES_MAX 16

/* rgb8 frames [Hin][Win][3] (bytes as a camera or a JPEG decoder delivers them) -> frames out_t0 .. out_t0 + T - 1 of the planar
 * fp16 tensor out [3][out_T][H][W] in [-1, 1], in ONE launch: the reference's push_frame arithmetic (release_server.py:479-481,
 * to_tensor -> half -> sub_(0.5).mul_(2.0)) and, when (Hin, Win) != (H, W), encode_video_latent's bicubic resize (v2v.py:153,
 * F.interpolate(mode='bicubic'): align_corners=False, A = -0.75, border-clamped taps, fp32 accumulation, one rounding to fp16, no
 * clamp of the overshoot).  At equal size the output is the decoded byte, bit for bit.
 *
 * Frame t is read at rgb8 + slots[t] * slot_stride bytes: `slots` is a HOST array of T non-negative indices into a ring of
 * frame slots (NULL = 0 .. T-1, i.e. T frames back to back when slot_stride = Hin * Win * 3).  No alignment is asked of rgb8 or
 * slot_stride.  Refused: null rgb8 / out, non-positive sizes, H or W not multiples of 8, out not 16-byte aligned, T above
 * RTV_FRAMES_MAX, frames outside [0, out_T), a negative slot or stride, and a downscale so strong (beyond ~20x) that the source
 * footprint of the smallest tile does not fit the LDS.  T == 0 returns 0. */
int rtv_frames_from_rgb8(const void* rgb8, const int* slots, int64_t slot_stride, int T, int Hin, int Win, void* out, int out_T,
                         int out_t0, int H, int W, rtv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
