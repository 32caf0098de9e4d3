/* raster.h -- the rasteriser of libasciichat_raster.so (include/asciichat_raster.h): the records shared by the host C
 * (raster.c) and the kernels (raster_kernels.hpp), the launchers between them (raster.hip), and the pure-C step that checks a
 * font and turns it into the tables the kernels read (the emulator driver of the tests calls it too).  Not installed. */
#ifndef ASCIICHAT_RASTER_PRIV_H
#define ASCIICHAT_RASTER_PRIV_H

#include <stdint.h>
#include <string.h>

#include "asciichat_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RASTER_BLOCK 256        /* threads per workgroup of every kernel */
#define RASTER_CHUNK 256        /* bytes of a text row a wave stages in LDS at a time */
#define RASTER_ROWS_PER_BLOCK 4 /* parse: one wave per text row */
#define RASTER_FIX_ROWS 32      /* resolve: cell rows per workgroup */
#define RASTER_TILE_GROUPS 64   /* raster: 16-byte groups (4 pixels) of an image row per tile = one wave's store */
#define RASTER_ATLAS_LDS 32768  /* raster: a coverage atlas up to this size is staged in LDS, a larger one read through L2 */
#define RASTER_NO_GLYPH 0xFFFFu
#define RASTER_INHERIT_FG 0x80000000u /* a cell written before its row's first fg-setting parameter: the entry pen's */
#define RASTER_INHERIT_BG 0x40000000u
#define RASTER_PEN_UNTOUCHED 0xFFFFFFFFu

/* a cell: atlas slot (RASTER_NO_GLYPH: none) | inherit marks until the fix-up, resolved colours 0x00RRGGBB */
typedef struct {
  uint32_t slot, fg, bg;
} raster_cell_t;

/* what a text row leaves behind: its exit pen per channel (RASTER_PEN_UNTOUCHED, or the colour -- the default's included),
 * its flags.  Record `rows` of a frame is the text behind the last row of the grid (flags only). */
typedef struct {
  uint32_t fg, bg, flags, _pad;
} raster_rowrec_t;

/* a glyph as the raster kernel reads it: the bitmap rectangle relative to the cell origin, biased to bytes */
typedef struct {
  uint32_t box;   /* (x0 + 32) | (y0 + 64) << 8 | (x1 + 32) << 16 | (y1 + 64) << 24; x0 == x1: draws nothing */
  uint32_t pitch;
  uint32_t offset;
  uint32_t _pad;
} raster_glyph_t;

/* everything constant over a handle's life, by value in the kernel arguments */
typedef struct {
  int32_t cols, rows, cell_w, cell_h;
  int32_t n_glyphs, matrix_map;
  uint32_t default_fg, default_bg;
  const uint32_t *codepoints;   /* n_glyphs, ascending */
  const raster_glyph_t *glyphs; /* n_glyphs */
  const uint32_t *lut;          /* 512: indexed colour n as fg, then as bg */
  const uint8_t *coverage;
  uint32_t coverage_bytes;
  uint32_t atlas_in_lds; /* 1: the raster kernel stages the atlas */
} raster_params_t;

static inline uint32_t raster_xterm_rgb(int n) {
  static const uint8_t ansi16[16][3] = {{0, 0, 0},       {128, 0, 0},   {0, 128, 0},   {128, 128, 0}, {0, 0, 128},   {128, 0, 128},
                                        {0, 128, 128},   {192, 192, 192}, {128, 128, 128}, {255, 0, 0},   {0, 255, 0},   {255, 255, 0},
                                        {0, 0, 255},     {255, 0, 255}, {0, 255, 255}, {255, 255, 255}}; /* get_16color_rgb */
  static const uint8_t cube[6] = {0, 95, 135, 175, 215, 255};
  uint32_t r, g, b;
  if (n < 16) {
    r = ansi16[n][0], g = ansi16[n][1], b = ansi16[n][2];
  } else if (n < 232) {
    n -= 16;
    r = cube[n / 36], g = cube[n / 6 % 6], b = cube[n % 6];
  } else {
    r = g = b = (uint32_t)(8 + 10 * (n - 232));
  }
  return r << 16 | g << 8 | b;
}

/* NULL when the font and the grid are within asciichat_raster.h's limits, else what is wrong */
static inline const char *raster_check(const asciichat_raster_font_t *f, int cols, int rows, int max_frames) {
  if (!f)
    return "no font";
  if (cols < 1 || cols > ASCIICHAT_RASTER_MAX_COLS || rows < 1 || rows > ASCIICHAT_RASTER_MAX_ROWS)
    return "grid outside 1..1024 x 1..512";
  if (max_frames < 1 || max_frames > ASCIICHAT_RASTER_MAX_FRAMES)
    return "max_frames outside 1..4096";
  if (f->cell_w < 1 || f->cell_w > ASCIICHAT_RASTER_MAX_CELL_W || f->cell_h < 1 || f->cell_h > ASCIICHAT_RASTER_MAX_CELL_H)
    return "cell outside 1..32 x 1..64";
  if (f->baseline < 0 || f->baseline > f->cell_h)
    return "baseline outside the cell";
  if (f->n_glyphs < 0 || f->n_glyphs > ASCIICHAT_RASTER_MAX_GLYPHS || (f->n_glyphs && !f->glyphs))
    return "glyph count outside 0..1024, or no glyphs";
  if (f->coverage_bytes > ASCIICHAT_RASTER_MAX_COVERAGE || (f->coverage_bytes && !f->coverage))
    return "coverage above 1 MB, or none";
  if (f->indexed != ASCIICHAT_RASTER_INDEXED_FLAT && f->indexed != ASCIICHAT_RASTER_INDEXED_XTERM)
    return "indexed is neither FLAT nor XTERM";
  for (int i = 0; i < f->n_glyphs; i++) {
    const asciichat_raster_glyph_t *g = &f->glyphs[i];
    if (i && g->codepoint <= f->glyphs[i - 1].codepoint)
      return "codepoints not strictly ascending";
    const int x0 = g->left, y0 = f->baseline - g->top, x1 = x0 + g->width, y1 = y0 + g->rows;
    if (x0 < -f->cell_w || x1 > 2 * f->cell_w || y0 < -f->cell_h || y1 > 2 * f->cell_h)
      return "a glyph reaches beyond its cell's neighbours";
    if (g->pitch < g->width)
      return "a glyph's pitch below its width";
    if ((uint64_t)g->offset + (uint64_t)g->pitch * g->rows > (uint64_t)f->coverage_bytes)
      return "a glyph's bitmap beyond the coverage";
  }
  return NULL;
}

/* the tables of a checked font: codepoints[n_glyphs], glyphs[n_glyphs], lut[512] */
static inline void raster_tables(const asciichat_raster_font_t *f, uint32_t *codepoints, raster_glyph_t *glyphs, uint32_t *lut) {
  for (int i = 0; i < f->n_glyphs; i++) {
    const asciichat_raster_glyph_t *g = &f->glyphs[i];
    const int x0 = g->left, y0 = f->baseline - g->top;
    const int w = g->rows ? g->width : 0; /* (an empty bitmap draws nothing: terminal.c:513) */
    codepoints[i] = g->codepoint;
    memset(&glyphs[i], 0, sizeof(glyphs[i]));
    glyphs[i].box = (uint32_t)(x0 + 32) | (uint32_t)(y0 + 64) << 8 | (uint32_t)(x0 + w + 32) << 16 | (uint32_t)(y0 + g->rows + 64) << 24;
    glyphs[i].pitch = g->pitch;
    glyphs[i].offset = g->offset;
  }
  for (int n = 0; n < 256; n++) {
    const int flat = f->indexed == ASCIICHAT_RASTER_INDEXED_FLAT;
    lut[n] = flat ? f->flat_fg & 0xFFFFFFu : raster_xterm_rgb(n);
    lut[256 + n] = flat ? f->flat_bg & 0xFFFFFFu : raster_xterm_rgb(n);
  }
}

static inline size_t raster_parse_lds(void) { return 4u * ASCIICHAT_RASTER_MAX_GLYPHS + RASTER_ROWS_PER_BLOCK * RASTER_CHUNK; }
static inline size_t raster_draw_lds(const raster_params_t *p) {
  const size_t cells = 2u * (RASTER_TILE_GROUPS * 4u + 8u) * 20u; /* two cell rows of the widest tile, 20 bytes each */
  return cells + (p->atlas_in_lds ? ((size_t)p->coverage_bytes + 15u) & ~(size_t)15u : 0u);
}
/* how many tiles wide an image is (a row may begin up to 3 pixels into its first 16-byte group) */
static inline int raster_tiles(const raster_params_t *p) {
  const int groups = (p->cols * p->cell_w + 3 + 3) / 4;
  return (groups + RASTER_TILE_GROUPS - 1) / RASTER_TILE_GROUPS;
}

/* draw: workgroups an image's tiles are spread over -- small batches spread them, large ones walk them in one workgroup (the
 * staged atlas is loaded once per workgroup) */
static inline unsigned raster_draw_split(const raster_params_t *p, int n) {
  const unsigned tiles = (unsigned)raster_tiles(p), strips = (unsigned)n * (unsigned)p->rows;
  const unsigned split = strips >= 2048u ? 1u : 2048u / strips;
  return split > tiles ? tiles : split;
}

/* ---- the YUV 4:2:0 draw (raster_yuv_kernels.hpp) ---- */
#define RASTER_YUV_LANE_PX 4      /* pixel columns of two image rows a lane owns at a time: two 2x2 blocks, one slot */
#define RASTER_YUV_TILE_CELLS 256 /* cell columns whose records sit in LDS at a time, with a neighbour on either side */

/* cell rows a workgroup owns: its image rows pair up, so two when the cell height is odd (rows is then even, as H is) */
static inline unsigned raster_yuv_span(const raster_params_t *p) { return (p->cell_h & 1) ? 2u : 1u; }
static inline size_t raster_yuv_lds(const raster_params_t *p) {
  const size_t cells = (raster_yuv_span(p) + 1u) * (RASTER_TILE_GROUPS * 4u + 8u) * 20u; /* the span's cell rows and the one below */
  return cells + (p->atlas_in_lds ? ((size_t)p->coverage_bytes + 15u) & ~(size_t)15u : 0u);
}
/* workgroups a strip's slots are spread over: as raster_draw_split, small batches spread them, large ones walk them in one
 * workgroup (the staged atlas is loaded once per workgroup) -- at most as many as the first tile's slots fill */
static inline unsigned raster_yuv_split(const raster_params_t *p, int n) {
  const unsigned span = raster_yuv_span(p), strips = (unsigned)n * ((unsigned)p->rows / span);
  const unsigned ncol = p->cols < RASTER_YUV_TILE_CELLS ? (unsigned)p->cols : RASTER_YUV_TILE_CELLS;
  const unsigned slots = (ncol * (unsigned)p->cell_w + RASTER_YUV_LANE_PX - 1u) / RASTER_YUV_LANE_PX * (span * (unsigned)p->cell_h / 2u);
  const unsigned full = (slots + RASTER_BLOCK - 1u) / RASTER_BLOCK, split = strips >= 2048u ? 1u : 2048u / strips;
  return split > full ? full : split;
}

/* the launchers (raster.hip); each returns a hipError_t.  starts: n * (rows + 2) words, recs: n * (rows + 1), cells:
 * n * rows * cols, all device memory of the handle.  draw_yuv: width and height even, layout one of ASCIICHAT_RASTER_YUV_*. */
int raster_launch_parse(const raster_params_t *p, const uint8_t *frames, uint64_t frame_stride, const uint32_t *len, int n,
                        uint32_t *starts, raster_rowrec_t *recs, raster_cell_t *cells, uint32_t *status, void *stream);
int raster_launch_draw(const raster_params_t *p, const raster_cell_t *cells, int n, uint8_t *pixels, uint64_t image_pitch, void *stream);
int raster_launch_draw_yuv(const raster_params_t *p, const raster_cell_t *cells, int n, uint8_t *yuv, uint64_t image_pitch, int layout,
                           void *stream);

#ifdef __cplusplus
}
#endif
#endif
