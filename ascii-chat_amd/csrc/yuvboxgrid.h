/* yuvboxgrid.h -- what the host side of libasciichat_yuvboxgrid.so (yuvboxgrid.c) and its launcher (yuvboxgrid.hip, the kernel in
 * yuvboxgrid_kernels.hpp) share: the item a workgroup reads with the workgroup table in it, the pure-C checks of a set, the
 * cutting of a tile's rows into column segments, the rule of include/asciichat_yuvboxgrid.h walked on the host (the emulator
 * driver and the sanitizer program of the tests call all of them), and the launcher.  The slab's layout and the rewriting of the
 * descriptors are yuvgrid_math.h's, the box bounds, the source limit and the host walk of one image yuvbox.h's: none of them is
 * restated.  Not installed. */
#ifndef ASCIICHAT_YUVBOXGRID_PRIV_H
#define ASCIICHAT_YUVBOXGRID_PRIV_H

#include "yuvbox.h"
#include "yuvgrid_math.h"

#ifdef __cplusplus
extern "C" {
#endif

/* THE SEGMENT WIDTH: the bound on the source columns a workgroup sums, and so on its LDS stage (12 bytes a column); 0: no
 * split, a workgroup per stored row.  A workgroup is (tile, stored row, segment of output columns): an output row is cut into
 * segments of equal numbers of boxes whose source columns, the first rounded down to a multiple of four, stay within the bound
 * -- but never into less than one box, which no bound can cut without a sum across workgroups.  Where a segment's groups of four
 * columns leave lanes of the workgroup idle (a lane owns a group), the rows of the box are cut into 2 or 4 slices, a part of the
 * workgroup each, staged side by side and added up behind the barrier (yuvboxgrid_slices).  Chosen by measurement among 0, 1024,
 * 512 and 256 (profiles/yuvboxgrid_timing.txt). */
#ifndef YUVBOXGRID_SEG_COLS
#define YUVBOXGRID_SEG_COLS 512
#endif

#define YUVBOXGRID_MAX_WORKGROUPS 0x7FFFFFFFull /* of one launch: the grid is one-dimensional */

/* one tile as its workgroups take it: uniform per workgroup, so the loads are scalar.  first_wg is the workgroup table: the
 * workgroups of tile t are [items[t].first_wg, items[t + 1].first_wg), tile_h * segs of them, rows outermost */
typedef struct {
  asciichat_yuv_source_t src; /* resolved (no stride 0) */
  int32_t tile_w, tile_h;
  uint64_t at;       /* where the tile starts in the slab: a multiple of 16 (yuvgrid_fill's offsets) */
  uint32_t first_wg; /* the prefix sum of the earlier tiles' workgroups */
  uint32_t segs;     /* segments of a row: 1..tile_w */
  uint32_t seg_out;  /* output columns of a segment (the last may have fewer): segs = ceil(tile_w / seg_out) */
  uint32_t stage_cols; /* the columns a segment's stage may hold: a multiple of four (yuvboxgrid_cut) */
  uint32_t slices;     /* the row slices of a box, YUV_BLOCK / slices lanes each: 1, 2 or 4 */
  uint32_t _pad;
} yuvboxgrid_item_t;

/* the row slices for a stage of stage_cols columns: as many as keep every lane of a slice a group of its own */
static inline uint32_t yuvboxgrid_slices(uint32_t stage_cols) {
  const uint32_t groups = stage_cols / 4u;
  return groups <= YUV_BLOCK / 4u ? 4u : groups <= YUV_BLOCK / 2u ? 2u : 1u;
}

/* A row of `out` boxes over `src` columns cut for the bound `seg_cols` (0: no split): *seg_out the boxes of a segment,
 * *segs their number; -> the columns the stage of any segment may hold (a multiple of four, at most src rounded up to four).
 * k boxes from box a cover [lo(a), hi(a + k - 1)) with hi - lo <= ceil(k * src / out) + 1 (yuvbox_bounds: floors of
 * multiples of src / out, a box at least one column), three more for rounding lo down to a multiple of four, and the groups
 * that touch the range end at most three columns behind it. */
static inline uint32_t yuvboxgrid_cut(uint32_t src, uint32_t out, uint32_t seg_cols, uint32_t *seg_out, uint32_t *segs) {
  uint32_t k = out;
  if (seg_cols && (uint64_t)out * src > 0u) {
    const uint64_t fit = seg_cols > 8u ? (uint64_t)(seg_cols - 8u) * out / src : 0u; /* ceil(k * src / out) + 8 <= seg_cols */
    k = fit < 1u ? 1u : fit > out ? out : (uint32_t)fit;
  }
  *segs = (out + k - 1u) / k;
  k = (out + *segs - 1u) / *segs; /* the same number of segments, evenly filled */
  *seg_out = k;
  *segs = (out + k - 1u) / k;
  const uint64_t cols = (((uint64_t)k * src + out - 1u) / out + 8u + 3u) & ~(uint64_t)3u;
  const uint32_t whole = (src + 3u) & ~3u;
  return cols < whole ? (uint32_t)cols : whole;
}

/* NULL when YUV slot k of `comp` is taken with source `y`, else what is wrong: yuvgrid_slot_check's conditions without its
 * ratio check (the ratios are not read), and yuvbox's limit on the source */
static inline const char *yuvboxgrid_slot_check(const achip_composite_t *comp, int k, const asciichat_yuv_source_t *y) {
  const achip_comp_src_t *s = &comp->s[k];
  if (k >= comp->n_src)
    return "a YUV source for a slot at or behind n_src";
  if (!s->src)
    return "a YUV source for a slot that is not placed (src == NULL)";
  const char *why = yuvbox_source_check(y);
  if (why)
    return why;
  if (s->src_w != y->width || s->src_h != y->height)
    return "src_w x src_h of the slot is not the source's size";
  if (s->tile_w < 1 || s->tile_w > YUVGRID_MAX_SIDE || s->tile_h < 1 || s->tile_h > YUVGRID_MAX_SIDE)
    return "tile_w or tile_h outside 1..8192";
  return NULL;
}

/* NULL when set() takes (comps[0..n_comps-1], sources[0..n_comps-1]) for a handle of max_tiles at segment width seg_cols, else
 * what is wrong.  *bad_comp, *bad_slot (optional): the offending composite and slot, -1 where it is none of them; *n_tiles
 * (optional): the YUV slots of a taken set.  A handle keeps a set's descriptors, so a set has at most max_tiles composites. */
static inline const char *yuvboxgrid_set_check(const achip_composite_t *const *comps, const asciichat_yuv_source_t *const *sources, int n_comps,
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
    if (comps[c]->n_src < 0 || comps[c]->n_src > YUVGRID_SLOTS)
      return "n_src outside 0..9";
    for (int k = 0; k < YUVGRID_SLOTS; k++) {
      if (!yuvgrid_is_yuv(sources[c], k))
        continue; /* RGB24 or empty: left as it stands, nothing else of the entry is read */
      if (bad_slot)
        *bad_slot = k;
      const char *why = yuvboxgrid_slot_check(comps[c], k, &sources[c][k]);
      if (why)
        return why;
      if (++tiles > max_tiles)
        return "more YUV slots than max_tiles";
      uint32_t seg_out, segs;
      (void)yuvboxgrid_cut((uint32_t)sources[c][k].width, (uint32_t)comps[c]->s[k].tile_w, seg_cols, &seg_out, &segs);
      workgroups += (uint64_t)segs * (uint64_t)(uint32_t)comps[c]->s[k].tile_h;
      if (workgroups > YUVBOXGRID_MAX_WORKGROUPS)
        return "more than 2^31 - 1 workgroups (rows times segments over all tiles)";
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

/* The items of a checked set: yuvgrid_fill's tiles in yuvgrid_fill's order at yuvgrid_fill's offsets (grid: room for as many
 * yuvgrid_item_t, filled on the way), each with its cut and its place in the workgroup table; masks[c] (optional) as
 * yuvgrid_fill leaves them.  *workgroups: the launch's; *stage_cols: the widest stage among the tiles, all slices of it.  -> the
 * bytes of the slab */
static inline uint64_t yuvboxgrid_fill(const achip_composite_t *const *comps, const asciichat_yuv_source_t *const *sources, int n_comps,
                                       uint32_t seg_cols, yuvgrid_item_t *grid, yuvboxgrid_item_t *items, uint16_t *masks, uint32_t *workgroups,
                                       uint32_t *stage_cols) {
  const uint64_t bytes = yuvgrid_fill(comps, sources, n_comps, grid, masks, NULL);
  int n = 0;
  for (int c = 0; c < n_comps; c++)
    for (int k = 0; k < YUVGRID_SLOTS; k++)
      n += yuvgrid_is_yuv(sources[c], k);
  uint32_t first = 0u, widest = 0u;
  for (int t = 0; t < n; t++) {
    yuvboxgrid_item_t *it = &items[t];
    memset(it, 0, sizeof(*it)); /* (the padding too: the block is copied as bytes) */
    it->src = grid[t].src;
    it->tile_w = grid[t].tile_w, it->tile_h = grid[t].tile_h;
    it->at = grid[t].at;
    it->first_wg = first;
    it->stage_cols = yuvboxgrid_cut((uint32_t)it->src.width, (uint32_t)it->tile_w, seg_cols, &it->seg_out, &it->segs);
    it->slices = yuvboxgrid_slices(it->stage_cols);
    const uint32_t cols = it->slices * it->stage_cols;
    widest = cols > widest ? cols : widest;
    first += it->segs * (uint32_t)it->tile_h;
  }
  if (workgroups)
    *workgroups = first;
  if (stage_cols)
    *stage_cols = widest;
  return bytes;
}

/* the tile of workgroup b among n items: the last whose first_wg is not above b */
YUV_FN uint32_t yuvboxgrid_tile_of(const yuvboxgrid_item_t *items, uint32_t n, uint32_t b) {
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

/* THE RULE on the host: the tile of an item, 3 * tile_w * tile_h bytes at `out` (host-readable planes) -- yuvbox.h's walk of
 * the box average of the whole conversion, without flips.  What the kernel must leave; walked by the tests and by the sanitizer
 * program, never by the library. */
static inline void yuvboxgrid_host_tile(const yuvboxgrid_item_t *it, uint8_t *out) {
  const yuvbox_item_t image = yuvbox_item(&it->src, it->tile_w, it->tile_h, 0u);
  yuvbox_host_image(&image, out);
}

/* the bytes of dynamic LDS a launch needs: 3 * stage_cols column sums of 32 bits (stage_cols: every slice's columns) */
static inline size_t yuvboxgrid_lds_bytes(uint32_t stage_cols) { return yuvbox_lds_bytes((int)stage_cols); }

/* The launcher (yuvboxgrid.hip); returns a hipError_t.  Arguments are the host's to check: nothing is checked again there but
 * what keeps a grid legal.  items: device, n of them, `workgroups` in all; stage_cols: the widest stage among them, all its slices */
int yuvboxgrid_launch(const yuvboxgrid_item_t *items, int n, uint32_t workgroups, uint32_t stage_cols, uint8_t *tiles, void *stream);

#ifdef __cplusplus
}
#endif
#endif
