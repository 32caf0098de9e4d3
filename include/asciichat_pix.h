/*
 * asciichat_pix.h -- libasciichat_pix.so: packed RGB camera frames as they arrive -- RGB24, RGBA, BGR24, BGRA -- in front of the
 * renderers, on the device: only the pixels a render target samples (run), whole frames (run_whole, convert), or the box
 * average straight from the source (run_box, downscale).  A library of its own: it links none of the other seven and shares only
 * achip_types.h and the error-code values with them.
 *
 * THE RULE (stated here once).  A source is one plane of width x height pixels, both 1..8192.
 *
 *   - bpp is 3 bytes per pixel for RGB and BGR, 4 for RGBA and BGRA;
 *   - the stride is at least bpp * width and below 2^24; a stride of 0 means tight (bpp * width);
 *   - any base alignment is allowed;
 *   - a negative stride is refused (a bottom-up image is a top-down one with ACHIP_OP_FLIP_Y in its descriptor).
 *
 * Pixel (sx, sy) is the bpp bytes b0 b1 b2 [b3] at pixels + sy * stride + bpp * sx.  Its RGB24 value is
 *
 *     RGB   (b0, b1, b2)        RGBA  (b0, b1, b2)
 *     BGR   (b2, b1, b0)        BGRA  (b2, b1, b0)
 *
 * The fourth byte is never looked at: alpha has no meaning here, nothing is blended or premultiplied.  A source is read within
 * its (height - 1) * stride + bpp * width bytes and nowhere else.
 *
 * The conversion is a per-pixel map, so it commutes with the renderers' nearest-neighbour sampling: a render over the sampled
 * images run() leaves gives byte for byte the text a render over the wholly converted frame gives.  run_box() is the
 * composition of the whole conversion and asciichat_hip.h's area average, and like that pass opt-in and NOT a parity mode.
 *
 * The format values are those of the reference's wire constants PIXEL_FORMAT_RGB / RGBA / BGR / BGRA
 * (include/ascii-chat/common/protocol_constants.h:75-84).  The reference's own receive path disagrees with those constants:
 * lib/network/acip/handlers.c:813 accepts 1..4 and src/client/capture.c:299 sends 1 for RGB24.  The mapping from a packet's
 * field to a format below is therefore the caller's, and nothing about the wire is claimed.  What the layouts restate is the
 * reference's per-pixel CPU conversions of its capture backends: BGRA with a padded bytesPerRow
 * (lib/video/webcam/macos/webcam_avfoundation.m:390-404), tight BGRA (lib/video/webcam/windows/webcam_mediafoundation.c:563-),
 * tight RGBA (lib/video/webcam/wasm/webcam_wasm.c:166-176).  RGB is there so that a server tick with clients of every platform
 * is one set and one launch; for RGB sources the three passes are a gather, a strided copy and the box pass's own arithmetic.
 *
 * The packed tiles of a grid composite are libasciichat_pixgrid.so's (include/asciichat_pixgrid.h), sampled or averaged straight
 * from these sources.  Out of scope: 16-bit and planar RGB, alpha of any meaning, bottom-up images other than through the
 * descriptor's flip_y.
 *
 * Every call returns 0 or an ASCIICHAT_PIX_ERR_* code and records a message for asciichat_pix_last_error() (per thread).
 * All pointers named *_dev, and the pixels of a source, are device-visible.  A handle's calls belong to one stream.
 */
#ifndef ASCIICHAT_PIX_H
#define ASCIICHAT_PIX_H

#include <stddef.h>
#include <stdint.h>

#include "achip_types.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { /* the values of asciichat_hip.h, asciichat_raster.h and asciichat_yuv.h */
  ASCIICHAT_PIX_OK = 0,
  ASCIICHAT_PIX_ERR_MEMORY = 3,
  ASCIICHAT_PIX_ERR_NOT_SUPPORTED = 30,
  ASCIICHAT_PIX_ERR_INVALID_PARAM = 86,
  ASCIICHAT_PIX_ERR_NO_DEVICE = 200 /* no HIP device, or a HIP runtime failure */
};

enum { ASCIICHAT_PIX_RGB = 0, ASCIICHAT_PIX_RGBA = 1, ASCIICHAT_PIX_BGR = 2, ASCIICHAT_PIX_BGRA = 3 };

typedef struct {
  const uint8_t *pixels;
  int32_t stride; /* bytes per row; 0 = tight */
  int32_t format, width, height;
} asciichat_pix_source_t;

typedef struct asciichat_pix asciichat_pix_t;

int asciichat_pix_device_count(void);
const char *asciichat_pix_last_error(void);

/* One source, whole: RGB24 row y at rgb_dev + y * rgb_stride (rgb_stride >= 3 * width, below 2^24; 0 = tight), any base
 * alignment.  The source travels in the kernel arguments: nothing is uploaded, nothing allocated.  Asynchronous on `stream`. */
int asciichat_pix_convert(const asciichat_pix_source_t *src, uint8_t *rgb_dev, int rgb_stride, void *stream);

/* One source (3840 x 2160 at the most) averaged to dst_w x dst_h (1..16384 each; 3 * dst_w * dst_h bytes at dst_dev, rows tight,
 * any alignment), beside asciichat_pix_convert and asciichat_hip_box_downscale.  The source travels in the kernel arguments:
 * nothing is uploaded, nothing allocated.  Asynchronous on `stream`. */
int asciichat_pix_downscale(const asciichat_pix_source_t *src, uint8_t *dst_dev, int dst_w, int dst_h, int flip_x, int flip_y,
                            void *stream);

/* A handle for up to max_frames (1..65535) sources per set.  Everything a handle ever needs is allocated here -- one device
 * block, one pinned block --; nothing allocates afterwards. */
int asciichat_pix_create(asciichat_pix_t **h, int max_frames);

/* The tick's sources and, with them, the descriptors achip_frame_setup() made for them (n of each, 1 <= n <= max_frames).
 * Each source is checked against THE RULE, in the order of its sentences.  Of frames[i], src and src_stride are not read; a
 * descriptor with comp is refused with ERR_NOT_SUPPORTED (the packed tiles of a composite go through asciichat_pixgrid.h); src_w x
 * src_h must equal source i's size; out_w and out_h are at least 1 and the image below 2^31 bytes; achip_frame_ratios_ok's rule
 * must hold.  frames may be NULL: the handle then serves run_whole only, and run / run_box / render_frames refuse.
 * Checked on the host before anything changes: a refused call leaves the handle as it was.  Sources and descriptors travel in
 * one pinned block the handle owns, by one asynchronous copy on `stream`; should the block still be in flight from the set
 * before, the call waits for that stream first. */
int asciichat_pix_set(asciichat_pix_t *h, const asciichat_pix_source_t *sources, const achip_frame_t *frames, int n, void *stream);

/* the largest 3 * out_w * out_h of the set's descriptors, rounded up to 128; 0 without descriptors */
size_t asciichat_pix_image_pitch(const asciichat_pix_t *h);

/* Frame i's sampled image to images_dev + i * pitch: out_w x out_h RGB24, rows tight; pixel (x, y) is the RGB24 value of source
 * pixel sx = min((x * x_ratio) >> 16, w - 1), sy = min((y * y_ratio) >> 16, h - 1), then the flips of ops.  Exactly
 * 3 * out_w * out_h bytes of a slot are stored.  images_dev and pitch: multiples of 16, the pitch at least the largest image.
 * One launch; asynchronous; never synchronises. */
int asciichat_pix_run(asciichat_pix_t *h, uint8_t *images_dev, size_t pitch, void *stream);

/* The same slots: image i is the box average of the whole conversion of source i to out_w x out_h -- asciichat_hip.h's rule
 * (achip_box_bounds): the column box of x is x0 = floor(x * width / out_w), x1 = max(x0 + 1, floor((x + 1) * width / out_w)),
 * rows alike; per channel A[y][x] = (S + n / 2) / n with S the channel's sum over the box and n its pixels; the
 * ACHIP_OP_FLIP_X / _Y bits of ops mirror the averaged image: stored pixel (x, y) =
 * A[flip_y ? out_h - 1 - y : y][flip_x ? out_w - 1 - x : x].  x_ratio and y_ratio play no part.  By definition byte for byte
 * what asciichat_pix_run_whole followed by asciichat_hip_box_run leaves.  Opt-in and not a parity mode, as the box pass is
 * not.  ERR_NOT_SUPPORTED if a source of the set exceeds the box pass's 3840 x 2160 or an image side its 16384: decided at
 * set, reported here.  One launch; asynchronous; never synchronises. */
int asciichat_pix_run_box(asciichat_pix_t *h, uint8_t *images_dev, size_t pitch, void *stream);

/* The set's descriptors rewritten onto those images, as asciichat_hip_box_render_frames and asciichat_yuv_render_frames do it:
 * src = the image, src_w x src_h = out_w x out_h, ratios 65537, tight stride, the flip bits cleared (the pass applied them),
 * comp NULL; paddings and every other bit of ops (tint, override, dither style) kept.  One form serves run and run_box.  The
 * use: set, render_frames, asciichat_hip_plan_create(mode, palette, frames_out); then per tick set, run, plan_render on one
 * stream.  Every mode works, since the pass only makes images. */
int asciichat_pix_render_frames(const asciichat_pix_t *h, const uint8_t *images_dev, size_t pitch, achip_frame_t *frames_out);

/* the largest 3 * width * height of the set's sources, rounded up to 128 */
size_t asciichat_pix_whole_pitch(const asciichat_pix_t *h);

/* Source i whole to rgb_dev + i * pitch: 3 * width * height bytes, rows tight, any alignment; pitch at least the largest
 * image.  For consumers of whole RGB frames: grid-composite sources, the frame table, the box pass.  Asynchronous. */
int asciichat_pix_run_whole(asciichat_pix_t *h, uint8_t *rgb_dev, size_t pitch, void *stream);

void asciichat_pix_destroy(asciichat_pix_t *h);

#ifdef __cplusplus
}
#endif
#endif
