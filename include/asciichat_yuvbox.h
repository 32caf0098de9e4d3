/*
 * asciichat_yuvbox.h -- libasciichat_yuvbox.so: camera and decoder frames -- I420, NV12, YUYV, UYVY -- averaged to the size a
 * render target samples, straight from their planes, on the device.  The two opt-in passes in front of the renderers in one:
 * the YUV sources of asciichat_yuv.h and the area-average (box filter) downscale of asciichat_hip.h, without the whole RGB24
 * frames between them -- every YUV sample is read once, only the small images are written.
 *
 * THE RULE (stated here once; nothing in it is new, it is the composition of two rules the project states already):
 *
 *     image i = box average of (the whole conversion of source i)
 *
 *   - the whole conversion is asciichat_yuv.h's "THE RULE" over the four layouts stated there: 8-bit BT.601, video range,
 *     integer, each channel clamped to 0..255, the chroma of the pixel's 2x2 (4:2:0) or 2x1 (4:2:2) block as it stands;
 *   - the box average is asciichat_hip.h's (achip_box_bounds): the column box of x is x0 = floor(x * width / out_w),
 *     x1 = max(x0 + 1, floor((x + 1) * width / out_w)), rows alike; per channel A[y][x] = (S + n / 2) / n with S the sum of the
 *     CONVERTED, CLAMPED channel over the box and n its pixels; the ACHIP_OP_FLIP_X / _Y bits of `ops` mirror the averaged
 *     image: stored pixel (x, y) = A[flip_y ? out_h - 1 - y : y][flip_x ? out_w - 1 - x : x].
 *
 * Every pixel is converted and clamped first, then summed: the clamp does not commute with the sum, so nothing is averaged in
 * YUV.  The result is by definition byte for byte what asciichat_yuv_run_whole followed by asciichat_hip_box_run leaves.
 *
 * Opt-in and NOT a parity mode, exactly as the box pass is not: the reference point-samples its sources.  The renderers run
 * over the averaged images give byte for byte what the reference's renderers give over those images; nothing is claimed about
 * the source frames.  The YUV tiles of a composite have the same rule in a library of their own (asciichat_yuvboxgrid.h).  Out
 * of scope, as for the two passes it composes: BT.709 and full-range matrices, interpolated chroma.
 *
 * A library of its own: it links none of libasciichat_hip.so, libasciichat_raster.so, libasciichat_yuv.so and
 * libasciichat_yuvgrid.so and shares only achip_types.h and asciichat_yuv.h (the source structure, the formats, the error-code
 * values) with them.
 *
 * Every call returns 0 or an ASCIICHAT_YUV_ERR_* code and records a message for asciichat_yuvbox_last_error() (per thread).
 * All pointers named *_dev, and the planes of a source, are device-visible.  A handle's calls belong to one stream.
 */
#ifndef ASCIICHAT_YUVBOX_H
#define ASCIICHAT_YUVBOX_H

#include <stddef.h>
#include <stdint.h>

#include "achip_types.h"
#include "asciichat_yuv.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct asciichat_yuvbox asciichat_yuvbox_t;

int asciichat_yuvbox_device_count(void);
const char *asciichat_yuvbox_last_error(void);

/* A handle for up to max_frames (1..65535) sources per set.  Everything a handle ever needs is allocated here -- one device
 * block, one pinned block --; nothing allocates afterwards. */
int asciichat_yuvbox_create(asciichat_yuvbox_t **h, int max_frames);

/* The tick's sources and the descriptors achip_frame_setup() made for them (n of each, 1 <= n <= max_frames; both required).
 * A source is checked as asciichat_yuv_set checks it, and may be 3840 x 2160 at the most (the box pass's limit).  Of frames[i]:
 * src, src_stride, x_ratio and y_ratio are not read; src_w x src_h must equal source i's size; out_w and out_h must lie in
 * 1..16384; a descriptor with comp is refused with ERR_NOT_SUPPORTED; everything else with ERR_INVALID_PARAM.
 * Checked on the host before anything changes: a refused call leaves the handle as it was.  The set travels in the pinned
 * block by one asynchronous copy on `stream`; should the block still be in flight from the set before, the call waits for that
 * stream first. */
int asciichat_yuvbox_set(asciichat_yuvbox_t *h, const asciichat_yuv_source_t *sources, const achip_frame_t *frames, int n, void *stream);

/* the largest 3 * out_w * out_h of the set's descriptors, rounded up to 128; 0 before any set */
size_t asciichat_yuvbox_image_pitch(const asciichat_yuvbox_t *h);

/* Image i (THE RULE, out_w x out_h RGB24, rows tight) to images_dev + i * pitch.  Exactly 3 * out_w * out_h bytes of a slot
 * are stored, and nothing else.  images_dev and pitch: multiples of 16, the pitch at least the largest image.  One launch;
 * asynchronous; never synchronises. */
int asciichat_yuvbox_run(asciichat_yuvbox_t *h, uint8_t *images_dev, size_t pitch, void *stream);

/* The set's descriptors rewritten onto those images, as asciichat_hip_box_render_frames and asciichat_yuv_render_frames do it:
 * src = the image, src_w x src_h = out_w x out_h, ratios 65537, tight stride, the flip bits cleared (the pass applied them),
 * comp NULL; paddings and every other bit of ops (tint, override, dither style) kept.  The use: set, render_frames,
 * asciichat_hip_plan_create(mode, palette, frames_out); then per tick set, run, plan_render on one stream. */
int asciichat_yuvbox_render_frames(const asciichat_yuvbox_t *h, const uint8_t *images_dev, size_t pitch, achip_frame_t *frames_out);

/* One source averaged to dst_w x dst_h (1..16384 each; 3 * dst_w * dst_h bytes at dst_dev, rows tight, any alignment), beside
 * asciichat_yuv_convert and asciichat_hip_box_downscale.  The source travels in the kernel arguments: nothing is uploaded,
 * nothing allocated.  Asynchronous on `stream`. */
int asciichat_yuvbox_downscale(const asciichat_yuv_source_t *src, uint8_t *dst_dev, int dst_w, int dst_h, int flip_x, int flip_y,
                               void *stream);

void asciichat_yuvbox_destroy(asciichat_yuvbox_t *h);

#ifdef __cplusplus
}
#endif
#endif
