/* yuvgrid_math.h -- YUV sources as the tiles of a grid composite (include/asciichat_yuvgrid.h): the pure-C checks of a set, the
 * item a workgroup of the tile kernel reads, the offsets of the tiles in their slab, the sampling of a tile and the rewriting of
 * a descriptor onto its tiles.  One text for the host (yuvgrid.c), the kernel (yuvgrid_kernels.hpp), the emulator driver and the
 * sanitizer program of the tests.  The arithmetic, the layouts and the check of a source are yuv_math.h's.  Plain C;
 * __host__ __device__ under hipcc.  Not installed. */
#ifndef ASCIICHAT_YUVGRID_MATH_H
#define ASCIICHAT_YUVGRID_MATH_H

#include "yuv_math.h"

#define YUVGRID_MAX_TILES 4096
#define YUVGRID_MAX_SIDE 8192 /* of a tile */
#define YUVGRID_SLOTS 9       /* of a composite: achip_composite_t.s */

/* one tile as its workgroups take it: uniform per workgroup, so the loads are scalar */
typedef struct {
  asciichat_yuv_source_t src; /* resolved (no stride 0) */
  uint32_t x_ratio, y_ratio;  /* the slot's: source -> tile */
  int32_t tile_w, tile_h;
  uint64_t at;                /* where the tile starts in the slab: a multiple of 16 */
} yuvgrid_item_t;

/* the bytes a tile takes in the slab: 3 * tile_w * tile_h rounded up to 16 (so every tile starts 16-aligned) */
YUV_FN uint64_t yuvgrid_tile_bytes(int32_t tile_w, int32_t tile_h) {
  return (3ull * (uint64_t)(uint32_t)tile_w * (uint64_t)(uint32_t)tile_h + 15ull) & ~15ull;
}
/* the slab of tiles that end at `end`: rounded up to 128 */
YUV_FN uint64_t yuvgrid_slab_bytes(uint64_t end) { return (end + 127ull) & ~127ull; }

/* the composite samplers' rule (sample_composite, render_kernels.hpp): the source pixel of pixel (lx, ly) of a tile.  ly may be
 * tile_h for a pixel behind the tile that is computed and never stored: its product may wrap, the clamp holds all the same. */
YUV_FN void yuvgrid_sample_at(const yuvgrid_item_t *it, uint32_t lx, uint32_t ly, int32_t *sx, int32_t *sy) {
  uint32_t cx = (lx * it->x_ratio) >> 16, cy = (ly * it->y_ratio) >> 16;
  if (cx > (uint32_t)it->src.width - 1u)
    cx = (uint32_t)it->src.width - 1u;
  if (cy > (uint32_t)it->src.height - 1u)
    cy = (uint32_t)it->src.height - 1u;
  *sx = (int32_t)cx, *sy = (int32_t)cy;
}

/* ---- the checks (host) ---- */
/* slot k of a composite is a YUV slot when its entry of the nine sources has a first plane */
static inline int yuvgrid_is_yuv(const asciichat_yuv_source_t *nine, int k) { return nine[k].plane[0] != NULL; }

/* NULL when YUV slot k of `comp` is taken with source `y`, else what is wrong */
static inline const char *yuvgrid_slot_check(const achip_composite_t *comp, int k, const asciichat_yuv_source_t *y) {
  const achip_comp_src_t *s = &comp->s[k];
  if (k >= comp->n_src)
    return "a YUV source for a slot at or behind n_src";
  if (!s->src)
    return "a YUV source for a slot that is not placed (src == NULL)";
  const char *why = yuv_source_check(y);
  if (why)
    return why;
  if (s->src_w != y->width || s->src_h != y->height)
    return "src_w x src_h of the slot is not the source's size";
  if (s->tile_w < 1 || s->tile_w > YUVGRID_MAX_SIDE || s->tile_h < 1 || s->tile_h > YUVGRID_MAX_SIDE)
    return "tile_w or tile_h outside 1..8192";
  achip_frame_t f; /* achip_desc_ratios_ok's rule over the tile */
  memset(&f, 0, sizeof(f));
  f.out_w = s->tile_w, f.out_h = s->tile_h, f.x_ratio = s->x_ratio, f.y_ratio = s->y_ratio;
  if (!achip_desc_ratios_ok(&f))
    return "(tile_w - 1) * x_ratio or (tile_h - 1) * y_ratio reaches 2^32";
  return NULL;
}

/* NULL when set() takes (comps[0..n_comps-1], sources[0..n_comps-1]) for a handle of max_tiles, else what is wrong.
 * *bad_comp, *bad_slot (optional): the offending composite and slot, -1 where it is none of them; *n_tiles (optional): the YUV
 * slots of a taken set.  A handle keeps a set's descriptors, so a set has at most max_tiles composites as well. */
static inline const char *yuvgrid_set_check(const achip_composite_t *const *comps, const asciichat_yuv_source_t *const *sources, int n_comps,
                                            int max_tiles, int *bad_comp, int *bad_slot, int *n_tiles) {
  int tiles = 0;
  if (bad_comp)
    *bad_comp = -1;
  if (bad_slot)
    *bad_slot = -1;
  if (n_tiles)
    *n_tiles = 0;
  if (!comps || !sources || n_comps < 1 || n_comps > max_tiles)
    return "no composites, no sources, or their number outside 1..max_tiles";
  for (int c = 0; c < n_comps; c++) {
    if (bad_comp)
      *bad_comp = c;
    if (bad_slot)
      *bad_slot = -1;
    if (!comps[c] || !sources[c])
      return "a NULL composite or a NULL source array";
    if (comps[c]->n_src < 0 || comps[c]->n_src > YUVGRID_SLOTS)
      return "n_src outside 0..9";
    for (int k = 0; k < YUVGRID_SLOTS; k++) {
      if (!yuvgrid_is_yuv(sources[c], k))
        continue; /* RGB24 or empty: left as it stands, nothing else of the entry is read */
      if (bad_slot)
        *bad_slot = k;
      const char *why = yuvgrid_slot_check(comps[c], k, &sources[c][k]);
      if (why)
        return why;
      if (++tiles > max_tiles)
        return "more YUV slots than max_tiles";
    }
  }
  if (bad_comp)
    *bad_comp = -1;
  if (bad_slot)
    *bad_slot = -1;
  if (n_tiles)
    *n_tiles = tiles;
  return NULL;
}

/* ---- a checked set as the handle keeps it ---- */
/* The items of a checked set, tile t counted over composites in order, then slots in order, over YUV slots only; masks[c]
 * (optional) receives bit k for YUV slot k of composite c; *max_pixels the largest tile_w * tile_h.  -> the bytes of the slab:
 * 0 without YUV slots.  Offsets depend on which slots are YUV and on their tile sizes, on nothing else. */
static inline uint64_t yuvgrid_fill(const achip_composite_t *const *comps, const asciichat_yuv_source_t *const *sources, int n_comps,
                                    yuvgrid_item_t *items, uint16_t *masks, uint32_t *max_pixels) {
  uint64_t at = 0;
  uint32_t most = 0u;
  int t = 0;
  for (int c = 0; c < n_comps; c++) {
    unsigned mask = 0u;
    for (int k = 0; k < YUVGRID_SLOTS; k++) {
      if (!yuvgrid_is_yuv(sources[c], k))
        continue;
      const achip_comp_src_t *s = &comps[c]->s[k];
      yuvgrid_item_t *it = &items[t++];
      memset(it, 0, sizeof(*it)); /* (the padding of the source too: the block is copied as bytes) */
      it->src = yuv_source_resolved(&sources[c][k]);
      it->x_ratio = s->x_ratio, it->y_ratio = s->y_ratio;
      it->tile_w = s->tile_w, it->tile_h = s->tile_h;
      it->at = at;
      at += yuvgrid_tile_bytes(s->tile_w, s->tile_h);
      const uint32_t pixels = (uint32_t)s->tile_w * (uint32_t)s->tile_h;
      most = pixels > most ? pixels : most;
      mask |= 1u << k;
    }
    if (masks)
      masks[c] = (uint16_t)mask;
  }
  if (max_pixels)
    *max_pixels = most;
  return yuvgrid_slab_bytes(at);
}

/* A descriptor rewritten onto its tiles: every YUV slot (mask) becomes a tile_w x tile_h source at tiles + *at with the identity
 * ratios, tile_* and org_* kept; every other slot and field as it stands.  *at moves on past the composite's tiles. */
static inline void yuvgrid_rewrite(const achip_composite_t *comp, unsigned mask, const uint8_t *tiles, uint64_t *at, achip_composite_t *out) {
  *out = *comp;
  for (int k = 0; k < YUVGRID_SLOTS; k++) {
    if (!(mask >> k & 1u))
      continue;
    achip_comp_src_t *s = &out->s[k];
    s->src = tiles + *at;
    s->src_w = s->tile_w, s->src_h = s->tile_h;
    s->src_stride = 3 * s->tile_w;
    s->x_ratio = s->y_ratio = 65537u; /* ((s << 16) / s) + 1: the identity */
    *at += yuvgrid_tile_bytes(s->tile_w, s->tile_h);
  }
}

/* a tile on the host: what the kernel stores, 3 * tile_w * tile_h bytes at out (the planes host memory) */
static inline void yuvgrid_host_tile(const yuvgrid_item_t *it, uint8_t *out) {
  const yuv_layout_t l = yuv_layout(&it->src);
  for (int32_t ly = 0; ly < it->tile_h; ly++)
    for (int32_t lx = 0; lx < it->tile_w; lx++) {
      int32_t sx, sy;
      yuvgrid_sample_at(it, (uint32_t)lx, (uint32_t)ly, &sx, &sy);
      const uint32_t p = yuv_pixel(&l, sx, sy);
      uint8_t *o = out + 3u * ((size_t)ly * (size_t)it->tile_w + (size_t)lx);
      o[0] = (uint8_t)p, o[1] = (uint8_t)(p >> 8), o[2] = (uint8_t)(p >> 16);
    }
}

#endif
