/*
 * asciichat_yuv.h -- libasciichat_yuv.so: camera and decoder frames as they arrive -- I420, NV12, YUYV, UYVY -- in front of the
 * renderers, on the device.  A library of its own: it links neither libasciichat_hip.so nor libasciichat_raster.so and shares
 * only achip_types.h and the error-code values with them.
 *
 * THE RULE (8-bit BT.601, video range, integer; stated here once):
 *
 *     y = Y - 16, u = U - 128, v = V - 128            (int)
 *     R = clamp255((298*y + 409*v + 128) >> 8)
 *     G = clamp255((298*y - 100*u - 208*v + 128) >> 8)
 *     B = clamp255((298*y + 516*u + 128) >> 8)        (>> is arithmetic, clamp to 0..255)
 *
 * Where the samples of pixel (sx, sy) of a w x h source sit, with cw = (w+1)/2, ch = (h+1)/2, Pk = plane[k], sk = stride[k]:
 *
 *     format  planes                  strides and sizes                              Y                                      U                             V
 *     I420    P0 Y, P1 U, P2 V        s0 >= w, s1, s2 >= cw; odd w and h allowed     P0[sy*s0 + sx]                         P1[(sy/2)*s1 + sx/2]          P2[(sy/2)*s2 + sx/2]
 *     NV12    P0 Y, P1 UV, P2 NULL    s0 >= w, s1 >= 2*cw; odd w and h allowed       as I420                                P1[(sy/2)*s1 + 2*(sx/2)]      that + 1
 *     UYVY    P0 only                 s0 >= 2*w, w even                              P0[sy*s0 + 4*(sx/2) + 1 + 2*(sx&1)]    P0[sy*s0 + 4*(sx/2)]          that + 2
 *     YUYV    P0 only                 s0 >= 2*w, w even                              P0[sy*s0 + 4*(sx/2) + 2*(sx&1)]        P0[sy*s0 + 4*(sx/2) + 1]      P0[sy*s0 + 4*(sx/2) + 3]
 *
 * A stride of 0 means tight (the minimum above); strides are below 2^24; width and height are 1..8192; a plane the format does
 * not use must be NULL.  A plane of r rows is read within its (r - 1) * stride + row bytes and nowhere else.  Chroma is the
 * sample of the pixel's 2x2 (4:2:0) or 2x1 (4:2:2) block as it stands: nothing is interpolated.
 *
 * The arithmetic and the I420 and UYVY layouts restate the reference's convert_pixel_buffer_to_rgb24
 * (lib/video/webcam/macos/webcam_avfoundation.m:406-472; I420 addressing :457-459, UYVY :413-416).  Its loop writes one pixel
 * past an odd-width packed row, so odd widths are refused for the packed formats.  NV12 and YUYV are the same arithmetic over
 * the other two layouts the reference's Linux capture negotiates (lib/video/webcam/linux/webcam_v4l2.c:198-306); there the
 * reference converts with libswscale, which is NOT restated and for which nothing is claimed.
 *
 * Conversion is a per-pixel map, so it commutes with the renderers' nearest-neighbour sampling: a render over the sampled
 * images run() leaves gives byte for byte the text a render over the wholly converted frame gives.
 *
 * Every call returns 0 or an ASCIICHAT_YUV_ERR_* code and records a message for asciichat_yuv_last_error() (per thread).
 * All pointers named *_dev, and the planes of a source, are device-visible.  A handle's calls belong to one stream.
 */
#ifndef ASCIICHAT_YUV_H
#define ASCIICHAT_YUV_H

#include <stddef.h>
#include <stdint.h>

#include "achip_types.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { /* the values of asciichat_hip.h and asciichat_raster.h */
  ASCIICHAT_YUV_OK = 0,
  ASCIICHAT_YUV_ERR_MEMORY = 3,
  ASCIICHAT_YUV_ERR_NOT_SUPPORTED = 30,
  ASCIICHAT_YUV_ERR_INVALID_PARAM = 86,
  ASCIICHAT_YUV_ERR_NO_DEVICE = 200 /* no HIP device, or a HIP runtime failure */
};

enum { ASCIICHAT_YUV_I420 = 0, ASCIICHAT_YUV_NV12 = 1, ASCIICHAT_YUV_YUYV = 2, ASCIICHAT_YUV_UYVY = 3 };

typedef struct {
  const uint8_t *plane[3];
  int32_t stride[3]; /* bytes per plane row; 0 = tight */
  int32_t format, width, height;
} asciichat_yuv_source_t;

typedef struct asciichat_yuv asciichat_yuv_t;

int asciichat_yuv_device_count(void);
const char *asciichat_yuv_last_error(void);

/* One source, whole: RGB24 row y at rgb_dev + y * rgb_stride (rgb_stride >= 3 * width, below 2^24; 0 = tight), any base
 * alignment.  The source travels in the kernel arguments: nothing is uploaded, nothing allocated.  Asynchronous on `stream`. */
int asciichat_yuv_convert(const asciichat_yuv_source_t *src, uint8_t *rgb_dev, int rgb_stride, void *stream);

/* A handle for up to max_frames (1..65535) sources per set.  Everything a handle ever needs is allocated here. */
int asciichat_yuv_create(asciichat_yuv_t **h, int max_frames);

/* The tick's sources and, with them, the descriptors achip_frame_setup() made for them (n of each, 1 <= n <= max_frames).
 * Of frames[i], src and src_stride are not read; src_w x src_h must equal source i's size; achip_frame_ratios_ok's rule must
 * hold; a descriptor with comp is refused with ERR_NOT_SUPPORTED (the YUV tiles of a composite: asciichat_yuvgrid.h).
 * frames may be NULL: the handle then serves run_whole only, and run / render_frames refuse.
 * Checked on the host before anything changes: a refused call leaves the handle as it was.  Sources and descriptors travel in
 * one pinned block the handle owns, by one asynchronous copy on `stream`; should the block still be in flight from the set
 * before, the call waits for that stream first. */
int asciichat_yuv_set(asciichat_yuv_t *h, const asciichat_yuv_source_t *sources, const achip_frame_t *frames, int n, void *stream);

/* the largest 3 * out_w * out_h of the set's descriptors, rounded up to 128; 0 without descriptors */
size_t asciichat_yuv_image_pitch(const asciichat_yuv_t *h);

/* Frame i's sampled image to images_dev + i * pitch: out_w x out_h RGB24, rows tight; pixel (x, y) is the conversion of source
 * pixel sx = min((x * x_ratio) >> 16, w - 1), sy = min((y * y_ratio) >> 16, h - 1), then the flips of ops.  Exactly
 * 3 * out_w * out_h bytes of a slot are stored.  images_dev and pitch: multiples of 16, the pitch at least the largest image.
 * Asynchronous; never synchronises. */
int asciichat_yuv_run(asciichat_yuv_t *h, uint8_t *images_dev, size_t pitch, void *stream);

/* The set's descriptors rewritten onto those images, as asciichat_hip_box_render_frames does it: src_w x src_h = out_w x out_h,
 * ratios 65537, tight stride, the flip bits cleared, comp NULL; paddings and every other bit of ops (tint, override, dither
 * style) kept.  The use: set, render_frames, asciichat_hip_plan_create(mode, palette, frames_out); then per tick set, run,
 * plan_render on one stream.  Every mode works, since the pass only makes images. */
int asciichat_yuv_render_frames(const asciichat_yuv_t *h, const uint8_t *images_dev, size_t pitch, achip_frame_t *frames_out);

/* the largest 3 * width * height of the set's sources, rounded up to 128 */
size_t asciichat_yuv_whole_pitch(const asciichat_yuv_t *h);

/* Source i whole to rgb_dev + i * pitch: 3 * width * height bytes, rows tight, any alignment; pitch at least the largest
 * image.  For consumers of whole RGB frames: grid-composite sources, the frame table, the box pass.  Asynchronous. */
int asciichat_yuv_run_whole(asciichat_yuv_t *h, uint8_t *rgb_dev, size_t pitch, void *stream);

void asciichat_yuv_destroy(asciichat_yuv_t *h);

#ifdef __cplusplus
}
#endif
#endif
