/*
 * asciichat_pixgrid.h -- libasciichat_pixgrid.so: packed RGB camera frames as they arrive -- RGB24, RGBA, BGR24, BGRA -- as the
 * tiles of a grid composite, point-sampled or box-averaged, straight from the source, on the device.  The packed row of the
 * table
 *
 *                        point-sampled                box-averaged
 *     plain source       asciichat_pix_run            asciichat_pix_run_box
 *     composite tile     asciichat_pixgrid_run        asciichat_pixgrid_run_box   (this header)
 *
 * beside asciichat_yuvgrid.h's and asciichat_yuvboxgrid.h's for YUV sources.  One launch per form for all tiles of all
 * composites of a tick; only the tiles -- about 1 KB each for an 80 x 24 terminal -- are written, and no whole RGB24 frame
 * exists anywhere.  As asciichat_pix_t does, one handle offers both tile forms.
 *
 * THE RULE (stated here once; nothing in it is new, it is a composition of rules the project states already).
 *
 * Packed slots.  Slot k of composite c is a packed slot when sources[c][k].pixels is not NULL.  Every other slot is left as it
 * stands -- RGB24 in place, already rewritten by another pass, or empty --, and nothing else of its source entry is read.  The
 * source of a packed slot obeys THE RULE of asciichat_pix.h: sides 1..8192; bpp 3 (RGB, BGR) or 4 (RGBA, BGRA); a stride of at
 * least bpp * width and below 2^24, 0 meaning tight; any base alignment; a negative stride refused; the fourth byte never looked
 * at; nothing read outside its (height - 1) * stride + bpp * width bytes.  Format RGB goes through the pass like the others, so
 * that a tick with clients of every platform is one set and one launch per form.
 *
 *   run       pixel (lx, ly) of the tile = the RGB24 value of source pixel
 *                 (min((lx * x_ratio) >> 16, width - 1), min((ly * y_ratio) >> 16, height - 1)):
 *             the composite samplers' own lookup; no flips, no tint.  The conversion is a per-pixel permutation and commutes
 *             with nearest-neighbour sampling: a render over the rewritten descriptors prints, in every mode, the bytes a render
 *             over asciichat_pix_run_whole's frames prints.
 *
 *   run_box   the tile = the box average of (the whole conversion of the source) to tile_w x tile_h, asciichat_hip.h's rule
 *             (achip_box_bounds): the column box of x is x0 = floor(x * width / tile_w), x1 = max(x0 + 1, floor((x + 1) * width
 *             / tile_w)), rows alike; per channel (S + n / 2) / n with S the channel's sum over the box and n its pixels; no
 *             flips; the ratios play no part in the tile.  By definition byte for byte step (1) of asciichat_hip_box_composites
 *             over asciichat_pix_run_whole's frame.  Opt-in and NOT a parity mode, exactly as the box pass is not: the reference
 *             point-samples its sources.  Sources above 3840 x 2160 are beyond the box pass: decided at set, reported by run_box
 *             with ERR_NOT_SUPPORTED, as asciichat_pix_run_box does; run still serves such a set.
 *
 * One check set serves both forms: a slot whose ratios fail run's 2^32 check is refused at set even where only run_box would be
 * called (achip_composite_setup never makes such ratios).
 *
 * Mixed ticks.  Passes chain through the descriptors, in either direction: what asciichat_yuvgrid_composites (or
 * asciichat_yuvboxgrid_composites) hands back is a valid comps_host for asciichat_pixgrid_set, and what
 * asciichat_pixgrid_composites hands back is a valid comps_host for asciichat_yuvgrid_set (or asciichat_yuvboxgrid_set): each
 * pass leaves the slots that are not its own exactly as they stand, and a slot another pass has rewritten is to this one an
 * RGB24 slot in place.  The caller gives each pass source entries for its own slots only.
 *
 * A library of its own: it links none of the other seven and shares only achip_types.h and asciichat_pix.h (the source
 * structure, the formats, the error-code values) with them.  The interface is asciichat_yuvgrid.h's with asciichat_pix_source_t
 * in the YUV source's place, and run_box beside run.
 *
 * Every call returns 0 or an ASCIICHAT_PIX_ERR_* code and records a message for asciichat_pixgrid_last_error() (per thread).
 * All pointers named *_dev, and the pixels of a source, are device-visible.  A handle's calls belong to one stream.
 *
 * Out of scope: flipped or tinted slots (the composite samplers do neither); fusing the canvas average (step (3) of
 * asciichat_hip_box_composites) into the pass; sampling packed pixels inside the render kernels; 16-bit, planar and ARGB / ABGR
 * layouts; alpha of any meaning; MJPEG.
 */
#ifndef ASCIICHAT_PIXGRID_H
#define ASCIICHAT_PIXGRID_H

#include <stddef.h>
#include <stdint.h>

#include "achip_types.h"
#include "asciichat_pix.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct asciichat_pixgrid asciichat_pixgrid_t;

int asciichat_pixgrid_device_count(void);
const char *asciichat_pixgrid_last_error(void);

/* A handle for up to max_tiles (1..4096) packed slots, and as many composites, per set.  Everything a handle ever needs is
 * allocated here -- one device block, one pinned block --; nothing allocates afterwards. */
int asciichat_pixgrid_create(asciichat_pixgrid_t **g, int max_tiles);

/* The tick's composites: comps_host[c] a host descriptor as achip_composite_setup makes it, sources[c] nine sources beside its
 * nine slots (n_comps of each, 1 <= n_comps <= max_tiles).  Of a packed slot, s[k].src only has to be non-NULL -- placed; the
 * pointer is not read --, k must lie below n_src (0..9), the source must be one asciichat_pix.h takes, src_w x src_h must equal
 * the source's size, tile_w and tile_h must lie in 1..8192, and (tile_w - 1) * x_ratio and (tile_h - 1) * y_ratio must stay
 * below 2^32.  At most max_tiles packed slots (and at most 2^31 - 1 workgroups of the averaged pass: rows times column segments
 * over all tiles, far beyond any slab a tick uses).  All checks happen on the host before anything changes: a refused call
 * (ERR_INVALID_PARAM, the message names composite and slot) leaves the handle as it was.  The set travels in the pinned block by
 * one asynchronous copy on `stream`; should the block still be in flight from the set before, the call waits for that stream
 * first. */
int asciichat_pixgrid_set(asciichat_pixgrid_t *g, const achip_composite_t *const *comps_host, const asciichat_pix_source_t *const *sources,
                          int n_comps, void *stream);

/* The bytes of the tile slab the set needs: exactly asciichat_yuvgrid_tiles_bytes' layout.  Tile t is counted over composites
 * in order, then slots in order, over packed slots only, and starts at the sum of the earlier tiles' 3 * tile_w * tile_h, each
 * rounded up to 16; the total is rounded up to 128, and is 0 when the set has no packed slot. */
size_t asciichat_pixgrid_tiles_bytes(const asciichat_pixgrid_t *g);

/* One launch samples every tile of every composite of the set into tiles_dev (16-aligned) by run's rule above; rows are tight;
 * exactly 3 * tile_w * tile_h bytes of a slot are stored and nothing else.  Asynchronous; never synchronises.  A set without
 * packed slots launches nothing and returns 0. */
int asciichat_pixgrid_run(asciichat_pixgrid_t *g, uint8_t *tiles_dev, void *stream);

/* The same slab, the same bytes stored: one launch averages every tile by run_box's rule above.  ERR_NOT_SUPPORTED if a source of
 * the set exceeds 3840 x 2160: decided at set, reported here, nothing launched.  Asynchronous; never synchronises.  A set
 * without packed slots launches nothing and returns 0. */
int asciichat_pixgrid_run_box(asciichat_pixgrid_t *g, uint8_t *tiles_dev, void *stream);

/* The set's n_comps descriptors with every packed slot rewritten onto its tile: src = the tile, src_w x src_h = tile_w x tile_h,
 * src_stride = 3 * tile_w, ratios 65537; tile_* and org_* kept, every other slot and field unchanged.  One rewritten form serves
 * run and run_box.  Sampled tiles: upload the descriptors with asciichat_hip_composite_upload (once per geometry) and render --
 * every mode works, since the pass only makes images.  Averaged tiles have two uses:
 *   (a) upload them and render: the composite samplers read an identity tile pixel for pixel, so the canvas shows the averaged
 *       tiles, rounded once;
 *   (b) hand them to asciichat_hip_box_composites: its step (1) over an identity tile is the identity (x0 = x, x1 = x + 1), so
 *       the images are byte for byte those of asciichat_pix_run_whole + asciichat_hip_box_composites over the converted frames,
 *       and no whole frame is written.
 * Per tick the sequence is set, run or run_box, then render, (a) or (b), on one stream. */
int asciichat_pixgrid_composites(const asciichat_pixgrid_t *g, const uint8_t *tiles_dev, achip_composite_t *comps_out);

void asciichat_pixgrid_destroy(asciichat_pixgrid_t *g);

#ifdef __cplusplus
}
#endif
#endif
