/*
 * asciichat_yuvboxgrid.h -- libasciichat_yuvboxgrid.so: camera and decoder frames -- I420, NV12, YUYV, UYVY -- as the AVERAGED
 * tiles of a grid composite, straight from their planes, on the device.  The fourth corner of the table
 *
 *                        point-sampled            box-averaged
 *     plain source       asciichat_yuv_*          asciichat_yuvbox_*
 *     composite tile     asciichat_yuvgrid_*      asciichat_yuvboxgrid_*   (this header)
 *
 * One launch for all tiles of all composites of a tick; every YUV sample is read once, only the tiles -- about 1 KB each for an
 * 80 x 24 terminal -- are written, and no whole RGB24 frame exists anywhere.
 *
 * THE RULE (stated here once; nothing in it is new, it is a composition of rules the project states already):
 *
 *     the tile of YUV slot k of composite c = box average of (the whole conversion of its source) to tile_w x tile_h
 *
 *   - the whole conversion is asciichat_yuv.h's "THE RULE" over the four layouts stated there: 8-bit BT.601, video range,
 *     integer, each channel clamped to 0..255, the chroma of the pixel's 2x2 (4:2:0) or 2x1 (4:2:2) block as it stands;
 *   - the box average is asciichat_hip.h's (achip_box_bounds): the column box of x is x0 = floor(x * width / tile_w),
 *     x1 = max(x0 + 1, floor((x + 1) * width / tile_w)), rows alike; per channel (S + n / 2) / n with S the sum of the
 *     CONVERTED, CLAMPED channel over the box and n its pixels;
 *   - no flips: the composite samplers apply none;
 *   - the slot's x_ratio / y_ratio are not read.
 *
 * Every pixel is converted and clamped first, then summed: nothing is averaged in YUV.  By definition the tile is step (1) of
 * asciichat_hip_box_composites over the wholly converted frame, byte for byte.
 *
 * Opt-in and NOT a parity mode, exactly as the box pass is not: the reference point-samples its sources.
 *
 * The interface is asciichat_yuvgrid.h's under another prefix: a caller switches between point-sampled and averaged tiles by
 * switching the prefix and nothing else.  A library of its own: it links none of libasciichat_hip.so, libasciichat_raster.so,
 * libasciichat_yuv.so, libasciichat_yuvgrid.so and libasciichat_yuvbox.so and shares only achip_types.h and asciichat_yuv.h (the
 * source structure, the formats, the error-code values) with them.
 *
 * Every call returns 0 or an ASCIICHAT_YUV_ERR_* code and records a message for asciichat_yuvboxgrid_last_error() (per thread).
 * All pointers named *_dev, and the planes of a source, are device-visible.  A handle's calls belong to one stream.
 *
 * Out of scope: BT.709 and full-range matrices, interpolated chroma, flipped or tinted slots, RGB24 slots through the pass, and
 * fusing the canvas average (step (3) of asciichat_hip_box_composites) into it.
 */
#ifndef ASCIICHAT_YUVBOXGRID_H
#define ASCIICHAT_YUVBOXGRID_H

#include <stddef.h>
#include <stdint.h>

#include "achip_types.h"
#include "asciichat_yuv.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct asciichat_yuvboxgrid asciichat_yuvboxgrid_t;

int asciichat_yuvboxgrid_device_count(void);
const char *asciichat_yuvboxgrid_last_error(void);

/* A handle for up to max_tiles (1..4096) YUV slots, and as many composites, per set.  Everything a handle ever needs is allocated
 * here -- one device block, one pinned block --; nothing allocates afterwards. */
int asciichat_yuvboxgrid_create(asciichat_yuvboxgrid_t **g, int max_tiles);

/* The tick's composites: comps_host[c] a host descriptor as achip_composite_setup makes it, sources[c] nine sources beside its
 * nine slots (n_comps of each, 1 <= n_comps <= max_tiles).  Slot k of composite c is a YUV slot when sources[c][k].plane[0] is
 * not NULL; otherwise the slot is left as it stands (RGB24, or empty) and nothing else of sources[c][k] is read.  Of a YUV slot,
 * s[k].src only has to be non-NULL -- placed; the pointer is not read --, k must lie below n_src (0..9), the source must be one
 * asciichat_yuv.h takes and no larger than 3840 x 2160, src_w x src_h must equal the source's size, and tile_w and tile_h must
 * lie in 1..8192; x_ratio and y_ratio are not read.  At most max_tiles YUV slots (and at most 2^31 - 1 workgroups: rows times
 * column segments over all tiles, far beyond any slab that fits a device).  Checked on the host before anything changes: a
 * refused call (ERR_INVALID_PARAM, the message names composite and slot) leaves the handle as it was.  The set travels in the
 * pinned block by one asynchronous copy on `stream`; should the block still be in flight from the set before, the call waits
 * for that stream first. */
int asciichat_yuvboxgrid_set(asciichat_yuvboxgrid_t *g, const achip_composite_t *const *comps_host, const asciichat_yuv_source_t *const *sources,
                             int n_comps, void *stream);

/* The bytes of the tile slab the set needs: exactly asciichat_yuvgrid_tiles_bytes' layout.  Tile t is counted over composites
 * in order, then slots in order, over YUV slots only, and starts at the sum of the earlier tiles' 3 * tile_w * tile_h, each
 * rounded up to 16; the total is rounded up to 128, and is 0 when the set has no YUV slot. */
size_t asciichat_yuvboxgrid_tiles_bytes(const asciichat_yuvboxgrid_t *g);

/* One launch averages every tile of every composite of the set into tiles_dev (16-aligned) by THE RULE above; rows are tight;
 * exactly 3 * tile_w * tile_h bytes of a slot are stored and nothing else.  Asynchronous; never synchronises.  A set without
 * YUV slots launches nothing and returns 0. */
int asciichat_yuvboxgrid_run(asciichat_yuvboxgrid_t *g, uint8_t *tiles_dev, void *stream);

/* The set's n_comps descriptors with every YUV slot rewritten onto its tile: src = the tile, src_w x src_h = tile_w x tile_h,
 * src_stride = 3 * tile_w, ratios 65537; tile_* and org_* kept, every other slot and field unchanged.  Two uses:
 *   (a) upload them with asciichat_hip_composite_upload (once per geometry) and render: the composite samplers read an identity
 *       tile pixel for pixel, so the canvas shows the averaged tiles, rounded once;
 *   (b) hand them to asciichat_hip_box_composites: its step (1) over an identity tile is the identity (x0 = x, x1 = x + 1), so
 *       the images are byte for byte those of asciichat_yuv_run_whole + asciichat_hip_box_composites over the converted frames,
 *       and no whole frame is written.
 * Per tick the sequence is set, run, then (a) or (b), on one stream. */
int asciichat_yuvboxgrid_composites(const asciichat_yuvboxgrid_t *g, const uint8_t *tiles_dev, achip_composite_t *comps_out);

void asciichat_yuvboxgrid_destroy(asciichat_yuvboxgrid_t *g);

#ifdef __cplusplus
}
#endif
#endif
