/* pixgrid.h -- what the host side of libasciichat_pixgrid.so (pixgrid.c) and its launchers (pixgrid.hip, the kernels in
 * pixgrid_kernels.hpp) share: the item a workgroup of either kernel reads -- the sampling ratios and the workgroup table of the
 * averaged pass both in it --, the pure-C checks of a set, the fill, the rule of include/asciichat_pixgrid.h walked on the host
 * for both tile forms (the emulator driver and the sanitizer program of the tests call all of them), and the launchers.  The
 * source's check, addressing and permutation are pix_math.h's, the host walks of one image pix.h's, the slab's layout and the
 * rewriting of the descriptors yuvgrid_math.h's (they read no YUV source), the cut of a row into segments and the row slices
 * yuvboxgrid.h's: none of them is restated.  Not installed. */
#ifndef ASCIICHAT_PIXGRID_PRIV_H
#define ASCIICHAT_PIXGRID_PRIV_H

#include "pix.h"
#include "yuvboxgrid.h"

#ifdef __cplusplus
extern "C" {
#endif

/* THE SEGMENT WIDTH of the averaged pass: the bound on the source columns a workgroup sums, and so on its LDS stage (12 bytes a
 * column); 0: no split, a workgroup per stored row.  The cut is yuvboxgrid_cut's and the row slices yuvboxgrid_slices', as they
 * stand.  Chosen by measurement among 0, 1024, 512 and 256 (profiles/pixgrid_timing.txt); make EXTRA=-DPIXGRID_SEG_COLS=N
 * BUILD=build_pixgridN PIXGRIDOUT=build_pixgridN/libasciichat_pixgrid.so build_pixgridN/libasciichat_pixgrid.so builds the
 * library at another width (the Makefile hands that -D to the C compiler too: the width is the host's choice). */
#ifndef PIXGRID_SEG_COLS
#define PIXGRID_SEG_COLS 512
#endif

#define PIXGRID_MAX_TILES YUVGRID_MAX_TILES
#define PIXGRID_MAX_SIDE YUVGRID_MAX_SIDE /* of a tile */
#define PIXGRID_SLOTS YUVGRID_SLOTS
#define PIXGRID_MAX_WORKGROUPS YUVBOXGRID_MAX_WORKGROUPS /* of the averaged launch: its grid is one-dimensional */

#if PIX_BLOCK != YUV_BLOCK
#error "yuvboxgrid_slices cuts a workgroup of YUV_BLOCK lanes: the kernels here run PIX_BLOCK"
#endif

/* one tile as the workgroups of either kernel take it: uniform per workgroup, so the loads are scalar.  The sampled kernel reads
 * src, the ratios, the size and `at`; the averaged kernel src, the size, `at` and the cut.  first_wg is the workgroup table of
 * the averaged launch: the workgroups of tile t are [items[t].first_wg, items[t + 1].first_wg), tile_h * segs of them, rows
 * outermost */
typedef struct {
  asciichat_pix_source_t src; /* resolved (no stride 0) */
  uint32_t x_ratio, y_ratio;  /* the slot's: source -> tile */
  int32_t tile_w, tile_h;
  uint64_t at;         /* where the tile starts in the slab: a multiple of 16 */
  uint32_t first_wg;   /* the prefix sum of the earlier tiles' workgroups */
  uint32_t segs;       /* segments of a row: 1..tile_w */
  uint32_t seg_out;    /* output columns of a segment (the last may have fewer): segs = ceil(tile_w / seg_out) */
  uint32_t stage_cols; /* the columns a segment's stage may hold: a multiple of four (yuvboxgrid_cut) */
  uint32_t slices;     /* the row slices of a box, PIX_BLOCK / slices lanes each: 1, 2 or 4 */
  uint32_t _pad;
} pixgrid_item_t;

/* the composite samplers' rule (sample_composite, render_kernels.hpp): the source pixel of pixel (lx, ly) of a tile.  ly may be
 * tile_h for a pixel behind the tile that is computed and never stored: its product may wrap, the clamp holds all the same. */
PIX_FN void pixgrid_sample_at(const pixgrid_item_t *it, uint32_t lx, uint32_t ly, int32_t *sx, int32_t *sy) {
  uint32_t cx = (lx * it->x_ratio) >> 16, cy = (ly * it->y_ratio) >> 16;
  if (cx > (uint32_t)it->src.width - 1u)
    cx = (uint32_t)it->src.width - 1u;
  if (cy > (uint32_t)it->src.height - 1u)
    cy = (uint32_t)it->src.height - 1u;
  *sx = (int32_t)cx, *sy = (int32_t)cy;
}

/* the tile of workgroup b of the averaged launch among n items: the last whose first_wg is not above b */
PIX_FN uint32_t pixgrid_tile_of(const pixgrid_item_t *items, uint32_t n, uint32_t b) {
  uint32_t lo = 0u, hi = n;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (items[mid].first_wg <= b)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

/* ---- the checks (host) ---- */
/* slot k of a composite is a packed slot when its entry of the nine sources has pixels */
static inline int pixgrid_is_packed(const asciichat_pix_source_t *nine, int k) { return nine[k].pixels != NULL; }

/* NULL when packed slot k of `comp` is taken with source `p`, else what is wrong: yuvgrid_slot_check's conditions over
 * pix_source_check.  One check serves both tile forms: the ratios must hold for run even where only run_box will be called. */
static inline const char *pixgrid_slot_check(const achip_composite_t *comp, int k, const asciichat_pix_source_t *p) {
  const achip_comp_src_t *s = &comp->s[k];
  if (k >= comp->n_src)
    return "a packed source for a slot at or behind n_src";
  if (!s->src)
    return "a packed source for a slot that is not placed (src == NULL)";
  const char *why = pix_source_check(p);
  if (why)
    return why;
  if (s->src_w != p->width || s->src_h != p->height)
    return "src_w x src_h of the slot is not the source's size";
  if (s->tile_w < 1 || s->tile_w > PIXGRID_MAX_SIDE || s->tile_h < 1 || s->tile_h > PIXGRID_MAX_SIDE)
    return "tile_w or tile_h outside 1..8192";
  achip_frame_t f; /* achip_desc_ratios_ok's rule over the tile */
  memset(&f, 0, sizeof(f));
  f.out_w = s->tile_w, f.out_h = s->tile_h, f.x_ratio = s->x_ratio, f.y_ratio = s->y_ratio;
  if (!achip_desc_ratios_ok(&f))
    return "(tile_w - 1) * x_ratio or (tile_h - 1) * y_ratio reaches 2^32";
  return NULL;
}

/* NULL when set() takes (comps[0..n_comps-1], sources[0..n_comps-1]) for a handle of max_tiles at segment width seg_cols, else
 * what is wrong.  *bad_comp, *bad_slot (optional): the offending composite and slot, -1 where it is none of them; *n_tiles
 * (optional): the packed slots of a taken set.  A handle keeps a set's descriptors, so a set has at most max_tiles composites. */
static inline const char *pixgrid_set_check(const achip_composite_t *const *comps, const asciichat_pix_source_t *const *sources, int n_comps,
                                            int max_tiles, uint32_t seg_cols, int *bad_comp, int *bad_slot, int *n_tiles) {
  int tiles = 0;
  uint64_t workgroups = 0;
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
    if (comps[c]->n_src < 0 || comps[c]->n_src > PIXGRID_SLOTS)
      return "n_src outside 0..9";
    for (int k = 0; k < PIXGRID_SLOTS; k++) {
      if (!pixgrid_is_packed(sources[c], k))
        continue; /* RGB24 in place, another pass's tile, or empty: left as it stands, nothing else of the entry is read */
      if (bad_slot)
        *bad_slot = k;
      const char *why = pixgrid_slot_check(comps[c], k, &sources[c][k]);
      if (why)
        return why;
      if (++tiles > max_tiles)
        return "more packed slots than max_tiles";
      uint32_t seg_out, segs;
      (void)yuvboxgrid_cut((uint32_t)sources[c][k].width, (uint32_t)comps[c]->s[k].tile_w, seg_cols, &seg_out, &segs);
      workgroups += (uint64_t)segs * (uint64_t)(uint32_t)comps[c]->s[k].tile_h;
      if (workgroups > PIXGRID_MAX_WORKGROUPS)
        return "more than 2^31 - 1 workgroups of the averaged pass (rows times segments over all tiles)";
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

/* what a filled set needs of its launches */
typedef struct {
  uint32_t max_pixels; /* the largest tile_w * tile_h: the sampled launch's grid */
  uint32_t workgroups; /* of the averaged launch */
  uint32_t stage_cols; /* the widest stage among the tiles, all slices of it */
  int boxable;         /* every source within the box pass's 3840 x 2160 */
} pixgrid_launches_t;

/* ---- a checked set as the handle keeps it ---- */
/* The items of a checked set, tile t counted over composites in order, then slots in order, over packed slots only -- yuvgrid_fill's
 * order at yuvgrid_fill's offsets --, each with its cut and its place in the workgroup table; masks[c] (optional) receives bit k
 * for packed slot k of composite c; *launches (optional) what run and run_box launch with.  -> the bytes of the slab: 0 without
 * packed slots.  Offsets depend on which slots are packed and on their tile sizes, on nothing else. */
static inline uint64_t pixgrid_fill(const achip_composite_t *const *comps, const asciichat_pix_source_t *const *sources, int n_comps,
                                    uint32_t seg_cols, pixgrid_item_t *items, uint16_t *masks, pixgrid_launches_t *launches) {
  uint64_t at = 0;
  pixgrid_launches_t l = {0u, 0u, 0u, 1};
  int t = 0;
  for (int c = 0; c < n_comps; c++) {
    unsigned mask = 0u;
    for (int k = 0; k < PIXGRID_SLOTS; k++) {
      if (!pixgrid_is_packed(sources[c], k))
        continue;
      const achip_comp_src_t *s = &comps[c]->s[k];
      pixgrid_item_t *it = &items[t++];
      memset(it, 0, sizeof(*it)); /* (the padding too: the block is copied as bytes) */
      it->src = pix_source_resolved(&sources[c][k]);
      it->x_ratio = s->x_ratio, it->y_ratio = s->y_ratio;
      it->tile_w = s->tile_w, it->tile_h = s->tile_h;
      it->at = at;
      at += yuvgrid_tile_bytes(s->tile_w, s->tile_h);
      it->first_wg = l.workgroups;
      it->stage_cols = yuvboxgrid_cut((uint32_t)it->src.width, (uint32_t)it->tile_w, seg_cols, &it->seg_out, &it->segs);
      it->slices = yuvboxgrid_slices(it->stage_cols);
      const uint32_t pixels = (uint32_t)s->tile_w * (uint32_t)s->tile_h, cols = it->slices * it->stage_cols;
      l.max_pixels = pixels > l.max_pixels ? pixels : l.max_pixels;
      l.stage_cols = cols > l.stage_cols ? cols : l.stage_cols;
      l.workgroups += it->segs * (uint32_t)it->tile_h;
      l.boxable &= pix_source_boxable(&it->src);
      mask |= 1u << k;
    }
    if (masks)
      masks[c] = (uint16_t)mask;
  }
  if (launches)
    *launches = l;
  return yuvgrid_slab_bytes(at);
}

/* ---- THE RULE on the host: the tile of an item, 3 * tile_w * tile_h bytes at `out` (host-readable pixels).  What the kernels
 * must leave; walked by the tests and by the sanitizer program, never by the library ---- */
static inline void pixgrid_host_tile(const pixgrid_item_t *it, uint8_t *out) {
  for (int32_t ly = 0; ly < it->tile_h; ly++)
    for (int32_t lx = 0; lx < it->tile_w; lx++) {
      int32_t sx, sy;
      pixgrid_sample_at(it, (uint32_t)lx, (uint32_t)ly, &sx, &sy);
      const uint32_t p = pix_pixel(&it->src, sx, sy);
      uint8_t *o = out + 3u * ((size_t)ly * (size_t)it->tile_w + (size_t)lx);
      o[0] = (uint8_t)p, o[1] = (uint8_t)(p >> 8), o[2] = (uint8_t)(p >> 16);
    }
}
/* pix.h's walk of the box average of the whole conversion, without flips */
static inline void pixgrid_host_box_tile(const pixgrid_item_t *it, uint8_t *out) { pix_host_box(&it->src, it->tile_w, it->tile_h, 0u, out); }

/* the bytes of dynamic LDS an averaged launch needs: 3 * stage_cols column sums of 32 bits (stage_cols: every slice's columns) */
static inline size_t pixgrid_lds_bytes(uint32_t stage_cols) { return pix_box_lds_bytes((int)stage_cols); }

/* The launchers (pixgrid.hip); each returns a hipError_t.  Arguments are the host's to check: nothing is checked again there but
 * what keeps a grid legal.  items: device, n of them.
 * sampled tiles: max_pixels the largest tile_w * tile_h among them */
int pixgrid_launch_tiles(const pixgrid_item_t *items, int n, uint32_t max_pixels, uint8_t *tiles, void *stream);
/* averaged tiles: `workgroups` in all; stage_cols: the widest stage among the items, all its slices */
int pixgrid_launch_box(const pixgrid_item_t *items, int n, uint32_t workgroups, uint32_t stage_cols, uint8_t *tiles, void *stream);

#ifdef __cplusplus
}
#endif
#endif
