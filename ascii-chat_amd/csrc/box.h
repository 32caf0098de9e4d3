/* box.h -- the area-average downscale pass: the per-frame descriptor shared by the host C (box.c) and the kernels
 * (box_kernels.hpp), the launchers between them (box.hip), and the plan step that turns a tick's plain and grid-composite
 * frames into the work of a run (pure C: the emulator driver of the tests calls it too).  Not installed. */
#ifndef ACHIP_BOX_H
#define ACHIP_BOX_H

#include <stdint.h>
#include <string.h>

#include "achip_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one frame of a box batch: what the pass reads of a render descriptor (achip_frame_t), the stride resolved */
typedef struct {
  const uint8_t *src;     /* RGB24 rows, any alignment */
  int64_t src_stride;     /* bytes per source row, >= 3 * src_w */
  int32_t src_w, src_h;   /* 1..3840 x 1..2160 */
  int32_t out_w, out_h;   /* the averaged image: 1..ACHIP_BOX_MAX_OUT each */
  uint32_t flips;         /* ACHIP_OP_FLIP_X | ACHIP_OP_FLIP_Y, applied to the averaged image */
  uint32_t _pad;
} achip_box_desc_t;

/* A launch whose descriptors differ only in their source, and there by a constant pitch: the common descriptor travels in
 * the kernel arguments (frame i reads d.src + i * src_pitch), as achip_uniform_t does for the renderers. */
typedef struct {
  achip_box_desc_t d;
  int64_t src_pitch;
  uint32_t enabled;
  uint32_t _pad;
} achip_box_uniform_t;

/* One grid cell of an averaged composite frame: where its tile lies on the canvas and in the tile scratch slab. */
typedef struct {
  int32_t org_x, org_y;   /* canvas position of tile pixel (0, 0); the plan keeps |org| below the canvas limits */
  int32_t tile_w, tile_h; /* 1..canvas size */
  int32_t slot;           /* the tile is tight RGB24 at tiles + slot * tile_pitch; -1: nothing of this cell is ever shown */
  int32_t _pad[3];
} achip_box_cell_t;

/* One composite frame of a box batch as box_canvas_kernel reads it: the grid lookup of sample_composite
 * (render_kernels.hpp) with an averaged tile per placed source, the canvas averaged to out_w x out_h. */
typedef struct {
  int32_t canvas_w, canvas_h; /* 1..3840 x 1..2160 */
  int32_t out_w, out_h;       /* 1..ACHIP_BOX_MAX_OUT each */
  uint32_t flips;             /* applied to the averaged image */
  int32_t cols, rows;         /* >= 0 */
  int32_t cell_w, cell_h;     /* <= 0: no grid, the canvas is black */
  int32_t n_src;              /* 0..9 */
  int32_t frame;              /* the image goes to images + frame * pitch */
  int32_t _pad;
  achip_box_cell_t cell[9];
} achip_box_canvas_t;

/* why a render descriptor is refused (achip_box_desc_from_frame, achip_box_plan) */
enum {
  ACHIP_BOX_OK = 0,
  ACHIP_BOX_COMPOSITE,
  ACHIP_BOX_NO_SOURCE,
  ACHIP_BOX_SOURCE_SIZE,
  ACHIP_BOX_OUT_SIZE,
  ACHIP_BOX_STRIDE,
  /* composite frames only */
  ACHIP_BOX_CANVAS_SIZE,  /* canvas outside 1..3840 x 1..2160 */
  ACHIP_BOX_CANVAS_FRAME, /* the frame's src_w x src_h is not the canvas */
  ACHIP_BOX_GRID,         /* n_src outside 0..9, negative cols or rows */
  ACHIP_BOX_TILE_SIZE     /* a placed source's tile outside 1..canvas size */
};

#define ACHIP_BOX_BLOCK 256      /* threads per workgroup: one workgroup per (frame, output row) */
#define ACHIP_BOX_MAX_SRC_W 3840 /* image_validate_dimensions: the LDS stage holds 3 * src_w column sums (45 KB) */
#define ACHIP_BOX_MAX_SRC_H 2160
#define ACHIP_BOX_MAX_OUT 16384  /* (out * src) stays far below 2^32 in the box bounds */

/* frames i < n: desc_dev[i] (device memory; unused when uniform->enabled), averaged image i at images + i * pitch
 * (3 * out_w * out_h bytes, tight rows).  max_out_h / max_src_w: the largest of the launch.  Returns a hipError_t. */
int achip_launch_box(const achip_box_desc_t *desc_dev, const achip_box_uniform_t *uniform, int n, int max_out_h, int max_src_w,
                     uint8_t *images, uint64_t pitch, void *stream);

/* composite frames k < n: table_dev[k] (device memory) assembled from the tiles of its cells (tiles + slot * tile_pitch, may be
 * NULL when no cell has one) into images + table[k].frame * pitch.  max_out_h / max_canvas_w: the largest of the launch.
 * Returns a hipError_t.  (Named outside exports.map's patterns: the library keeps it to itself.) */
int box_canvas_launch(const achip_box_canvas_t *table_dev, int n, int max_out_h, int max_canvas_w, const uint8_t *tiles,
                      uint64_t tile_pitch, uint8_t *images, uint64_t pitch, void *stream);

/* one render descriptor as the pass reads it: ACHIP_BOX_OK and *d, or the refusal */
static inline int achip_box_desc_from_frame(const achip_frame_t *f, achip_box_desc_t *d) {
  if (f->comp)
    return ACHIP_BOX_COMPOSITE;
  if (!f->src)
    return ACHIP_BOX_NO_SOURCE;
  if (f->src_w <= 0 || f->src_h <= 0 || f->src_w > ACHIP_BOX_MAX_SRC_W || f->src_h > ACHIP_BOX_MAX_SRC_H)
    return ACHIP_BOX_SOURCE_SIZE;
  if (f->out_w <= 0 || f->out_h <= 0 || f->out_w > ACHIP_BOX_MAX_OUT || f->out_h > ACHIP_BOX_MAX_OUT)
    return ACHIP_BOX_OUT_SIZE;
  if (f->src_stride != 0 && f->src_stride < 3 * f->src_w)
    return ACHIP_BOX_STRIDE;
  memset(d, 0, sizeof(*d));
  d->src = f->src;
  d->src_stride = f->src_stride ? f->src_stride : 3 * f->src_w;
  d->src_w = f->src_w;
  d->src_h = f->src_h;
  d->out_w = f->out_w;
  d->out_h = f->out_h;
  d->flips = f->ops & (ACHIP_OP_FLIP_X | ACHIP_OP_FLIP_Y);
  return ACHIP_BOX_OK;
}

/* fills u for d[0..n): enabled iff every field but src is equal and src[i] == src[0] + i * pitch for one pitch (n == 1:
 * always), as achip_frames_uniform decides for the renderers.  Returns u->enabled. */
static inline int achip_box_uniform(const achip_box_desc_t *d, int n, achip_box_uniform_t *u) {
  memset(u, 0, sizeof(*u));
  if (n <= 0)
    return 0;
  const int64_t pitch = n > 1 ? (int64_t)((intptr_t)d[1].src - (intptr_t)d[0].src) : 0;
  for (int i = 1; i < n; i++) {
    achip_box_desc_t a = d[i];
    if ((int64_t)((intptr_t)a.src - (intptr_t)d[0].src) != pitch * i)
      return 0;
    a.src = d[0].src;
    if (memcmp(&a, &d[0], sizeof(a)) != 0) /* descriptors are memset by achip_box_desc_from_frame: padding is zero */
      return 0;
  }
  u->d = d[0];
  u->src_pitch = pitch;
  u->enabled = 1;
  return 1;
}

/* What a run of a batch launches (achip_box_plan): box_kernel over the plain frames (their descriptors in plain[0..n), a
 * composite frame's entry all zero: out_h 0 makes its workgroups return), box_kernel over the unique tiles into the scratch
 * slab (tile t at t * tile_pitch), box_canvas_kernel over the composite frames.  A launch with a count of 0 is not issued. */
typedef struct {
  int32_t n_plain, n_tiles, n_canvas;
  int32_t plain_max_out_h, plain_max_src_w;
  int32_t tile_max_out_h, tile_max_src_w;
  int32_t canvas_max_out_h, canvas_max_w;
  int32_t bad_frame, bad_src; /* a refusal: the frame, and the composite source (-1: the frame itself) */
  uint64_t tile_pitch;        /* the largest tile's bytes rounded up to 128 */
  uint64_t image_bytes;       /* the largest 3 * out_w * out_h of the batch */
} achip_box_plan_t;

/* The plan step of a batch of n frames; comps == NULL or comps[i] == NULL: frame i is plain (achip_box_desc_from_frame's
 * rules), else it is averaged from the HOST composite descriptor comps[i] (frames[i].src and .comp are not read).
 * Validates every frame first -- ACHIP_BOX_OK, or the first refusal with p->bad_frame / p->bad_src -- and, when plain, tiles
 * and canvas are given (n, 9 * n and n entries; all three or none: none = validation only), fills them and *p.
 * Tiles are unique over the whole batch by (src, src_stride, src_w, src_h, tile_w, tile_h): targets of one terminal size
 * share the tiles of their sources.  A tile is made for a placed source (k < n_src, src != NULL) whose cell the lookup can
 * reach (a grid with cell_w, cell_h > 0, k < cols * rows) and whose rectangle meets the canvas; x_ratio / y_ratio are not
 * read. */
static inline int achip_box_plan(const achip_frame_t *frames, const achip_composite_t *const *comps, int n, achip_box_desc_t *plain,
                                 achip_box_desc_t *tiles, achip_box_canvas_t *canvas, achip_box_plan_t *p) {
  const int emit = plain && tiles && canvas;
  memset(p, 0, sizeof(*p));
  p->bad_src = -1;
  for (int i = 0; i < n; i++) { /* refusals first: nothing is written for a batch that holds one */
    const achip_frame_t *f = &frames[i];
    const achip_composite_t *c = comps ? comps[i] : NULL;
    p->bad_frame = i;
    p->bad_src = -1;
    if (!c) {
      achip_box_desc_t d;
      const int rc = achip_box_desc_from_frame(f, &d);
      if (rc != ACHIP_BOX_OK)
        return rc;
      continue;
    }
    if (c->canvas_w <= 0 || c->canvas_h <= 0 || c->canvas_w > ACHIP_BOX_MAX_SRC_W || c->canvas_h > ACHIP_BOX_MAX_SRC_H)
      return ACHIP_BOX_CANVAS_SIZE;
    if (f->src_w != c->canvas_w || f->src_h != c->canvas_h)
      return ACHIP_BOX_CANVAS_FRAME;
    if (f->out_w <= 0 || f->out_h <= 0 || f->out_w > ACHIP_BOX_MAX_OUT || f->out_h > ACHIP_BOX_MAX_OUT)
      return ACHIP_BOX_OUT_SIZE;
    if (c->n_src < 0 || c->n_src > 9 || c->cols < 0 || c->rows < 0)
      return ACHIP_BOX_GRID;
    for (int k = 0; k < c->n_src; k++) {
      const achip_comp_src_t *s = &c->s[k];
      if (!s->src)
        continue;
      p->bad_src = k;
      if (s->src_w <= 0 || s->src_h <= 0 || s->src_w > ACHIP_BOX_MAX_SRC_W || s->src_h > ACHIP_BOX_MAX_SRC_H)
        return ACHIP_BOX_SOURCE_SIZE;
      if (s->src_stride < 3 * s->src_w)
        return ACHIP_BOX_STRIDE;
      if (s->tile_w <= 0 || s->tile_h <= 0 || s->tile_w > c->canvas_w || s->tile_h > c->canvas_h)
        return ACHIP_BOX_TILE_SIZE;
    }
  }
  p->bad_frame = p->bad_src = -1;
  if (!emit)
    return ACHIP_BOX_OK;
  for (int i = 0; i < n; i++) {
    const achip_frame_t *f = &frames[i];
    const achip_composite_t *c = comps ? comps[i] : NULL;
    const uint64_t bytes = 3u * (uint64_t)f->out_w * (uint64_t)f->out_h;
    if (bytes > p->image_bytes)
      p->image_bytes = bytes;
    if (!c) {
      (void)achip_box_desc_from_frame(f, &plain[i]);
      p->n_plain++;
      if (plain[i].out_h > p->plain_max_out_h)
        p->plain_max_out_h = plain[i].out_h;
      if (plain[i].src_w > p->plain_max_src_w)
        p->plain_max_src_w = plain[i].src_w;
      continue;
    }
    memset(&plain[i], 0, sizeof(plain[i]));
    achip_box_canvas_t *t = &canvas[p->n_canvas++];
    memset(t, 0, sizeof(*t));
    t->canvas_w = c->canvas_w;
    t->canvas_h = c->canvas_h;
    t->out_w = f->out_w;
    t->out_h = f->out_h;
    t->flips = f->ops & (ACHIP_OP_FLIP_X | ACHIP_OP_FLIP_Y);
    t->cols = c->cols;
    t->rows = c->rows;
    t->cell_w = c->cell_w;
    t->cell_h = c->cell_h;
    t->n_src = c->n_src;
    t->frame = i;
    if (f->out_h > p->canvas_max_out_h)
      p->canvas_max_out_h = f->out_h;
    if (c->canvas_w > p->canvas_max_w)
      p->canvas_max_w = c->canvas_w;
    const int grid = c->cell_w > 0 && c->cell_h > 0;
    for (int k = 0; k < 9; k++) {
      const achip_comp_src_t *s = &c->s[k];
      achip_box_cell_t *cell = &t->cell[k];
      cell->slot = -1;
      if (!grid || k >= c->n_src || !s->src || (int64_t)k >= (int64_t)c->cols * (int64_t)c->rows)
        continue;
      if (s->org_x >= c->canvas_w || s->org_y >= c->canvas_h || (int64_t)s->org_x + s->tile_w <= 0 ||
          (int64_t)s->org_y + s->tile_h <= 0)
        continue; /* wholly off the canvas */
      cell->org_x = s->org_x;
      cell->org_y = s->org_y;
      cell->tile_w = s->tile_w;
      cell->tile_h = s->tile_h;
      int u = 0;
      for (; u < p->n_tiles; u++)
        if (tiles[u].src == s->src && tiles[u].src_stride == (int64_t)s->src_stride && tiles[u].src_w == s->src_w &&
            tiles[u].src_h == s->src_h && tiles[u].out_w == s->tile_w && tiles[u].out_h == s->tile_h)
          break;
      if (u == p->n_tiles) {
        achip_box_desc_t *d = &tiles[p->n_tiles++];
        memset(d, 0, sizeof(*d));
        d->src = s->src;
        d->src_stride = s->src_stride;
        d->src_w = s->src_w;
        d->src_h = s->src_h;
        d->out_w = s->tile_w;
        d->out_h = s->tile_h;
        const uint64_t tb = (3u * (uint64_t)s->tile_w * (uint64_t)s->tile_h + 127u) & ~(uint64_t)127u;
        if (tb > p->tile_pitch)
          p->tile_pitch = tb;
        if (s->tile_h > p->tile_max_out_h)
          p->tile_max_out_h = s->tile_h;
        if (s->src_w > p->tile_max_src_w)
          p->tile_max_src_w = s->src_w;
      }
      cell->slot = u;
    }
  }
  return ACHIP_BOX_OK;
}

#ifdef __cplusplus
}
#endif
#endif
