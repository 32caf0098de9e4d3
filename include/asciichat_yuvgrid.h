/*
 * asciichat_yuvgrid.h -- libasciichat_yuvgrid.so: camera and decoder frames -- I420, NV12, YUYV, UYVY -- as the tiles of a grid
 * composite, on the device.  The grid composite is the view a server renders for every client of a call; its samplers
 * (achip_composite_t, achip_types.h) point-sample each source into its tile.  This pass converts exactly those pixels of every
 * YUV source, one launch for all tiles of all composites of a tick, and hands back the descriptors with each YUV slot rewritten
 * onto its tile: a tile_w x tile_h RGB24 source with the identity ratios, which is what the multi-GPU grid path feeds the
 * renderers already.  Nothing in the renderers changes, and nothing converts a whole frame.
 *
 * The rule, the four layouts, the source structure and the error-code values are asciichat_yuv.h's, stated there once.  A
 * library of its own: it links none of libasciichat_hip.so, libasciichat_raster.so and libasciichat_yuv.so.
 *
 * Byte-exact: conversion is a per-pixel map, and the composite lookup samples source pixel
 *     sx = min((lx * x_ratio) >> 16, src_w - 1), sy = min((ly * y_ratio) >> 16, src_h - 1)          (no flips, no tint)
 * for pixel (lx, ly) of a tile.  A tile converted at those pixels and sampled with the identity ratio 65537 -- (l * 65537) >> 16
 * = l for l < 65536 -- renders the bytes the composite over the wholly converted frames renders, in every mode.
 *
 * Every call returns 0 or an ASCIICHAT_YUV_ERR_* code and records a message for asciichat_yuvgrid_last_error() (per thread).
 * All pointers named *_dev, and the planes of a source, are device-visible.  A handle's calls belong to one stream.
 */
#ifndef ASCIICHAT_YUVGRID_H
#define ASCIICHAT_YUVGRID_H

#include <stddef.h>
#include <stdint.h>

#include "achip_types.h"
#include "asciichat_yuv.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct asciichat_yuvgrid asciichat_yuvgrid_t;

int asciichat_yuvgrid_device_count(void);
const char *asciichat_yuvgrid_last_error(void);

/* A handle for up to max_tiles (1..4096) YUV slots, and as many composites, per set.  Everything a handle ever needs is allocated
 * here -- one device block, one pinned block --; nothing allocates afterwards. */
int asciichat_yuvgrid_create(asciichat_yuvgrid_t **g, int max_tiles);

/* The tick's composites: comps_host[c] a host descriptor as achip_composite_setup makes it, sources[c] nine sources beside its
 * nine slots (n_comps of each, 1 <= n_comps <= max_tiles).  Slot k of composite c is a YUV slot when sources[c][k].plane[0] is
 * not NULL; otherwise the slot is left as it stands (RGB24, or empty) and nothing else of sources[c][k] is read.  Of a YUV slot,
 * s[k].src only has to be non-NULL -- placed; the pointer is not read --, k must lie below n_src (0..9), src_w x src_h must equal
 * the source's size, tile_w and tile_h must lie in 1..8192, and (tile_w - 1) * x_ratio and (tile_h - 1) * y_ratio must stay
 * below 2^32.  At most max_tiles YUV slots.  Checked on the host before anything changes: a refused call (ERR_INVALID_PARAM, the
 * message names composite and slot) leaves the handle as it was.  The set travels in the pinned block by one asynchronous copy
 * on `stream`; should the block still be in flight from the set before, the call waits for that stream first. */
int asciichat_yuvgrid_set(asciichat_yuvgrid_t *g, const achip_composite_t *const *comps_host, const asciichat_yuv_source_t *const *sources,
                          int n_comps, void *stream);

/* The bytes of the tile slab the set needs.  Tile t is counted over composites in order, then slots in order, over YUV slots
 * only, and starts at the sum of the earlier tiles' 3 * tile_w * tile_h, each rounded up to 16; the total is rounded up to 128,
 * and is 0 when the set has no YUV slot.  Offsets depend only on which slots are YUV and on their tile sizes: a set per tick
 * with new plane pointers keeps every tile where it was. */
size_t asciichat_yuvgrid_tiles_bytes(const asciichat_yuvgrid_t *g);

/* One launch converts every tile of every composite of the set into tiles_dev (16-aligned): pixel (lx, ly) of a tile is the
 * conversion of source pixel (min((lx * x_ratio) >> 16, width - 1), min((ly * y_ratio) >> 16, height - 1)); rows are tight;
 * exactly 3 * tile_w * tile_h bytes of a slot are stored and nothing else.  Asynchronous; never synchronises.  A set without YUV
 * slots launches nothing and returns 0. */
int asciichat_yuvgrid_run(asciichat_yuvgrid_t *g, uint8_t *tiles_dev, void *stream);

/* The set's n_comps descriptors with every YUV slot rewritten onto its tile: src = the tile, src_w x src_h = tile_w x tile_h,
 * src_stride = 3 * tile_w, ratios 65537; tile_* and org_* kept, every other slot and field unchanged.  The caller uploads them
 * with asciichat_hip_composite_upload once per geometry; per tick the sequence is set, run, plan_render on one stream.  A
 * rewritten slot is never flipped or tinted: the composite samplers do neither.  asciichat_hip_box_composites over rewritten
 * descriptors averages each source to its tile, so an identity tile stays the point-sampled tile -- not the average over the
 * whole frame; for that, switch the prefix: asciichat_yuvboxgrid_* (asciichat_yuvboxgrid.h) is this interface over averaged tiles. */
int asciichat_yuvgrid_composites(const asciichat_yuvgrid_t *g, const uint8_t *tiles_dev, achip_composite_t *comps_out);

void asciichat_yuvgrid_destroy(asciichat_yuvgrid_t *g);

#ifdef __cplusplus
}
#endif
#endif
