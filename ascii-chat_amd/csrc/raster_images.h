/* raster_images.h -- the rasteriser's cells straight from frame descriptors (asciichat_raster_images_set and the entries behind
 * it, include/asciichat_raster.h): the records shared by the host C (raster.c) and the kernel (raster_images_kernels.hpp), and
 * the pure-C steps that check a mode, a palette and a batch of descriptors and turn the palette into the table the kernel
 * reads (the emulator driver and the sanitizer program of the tests call them too).  Not installed. */
#ifndef ASCIICHAT_RASTER_IMAGES_PRIV_H
#define ASCIICHAT_RASTER_IMAGES_PRIV_H

#include "achip_desc.h"
#include "raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RASTER_IMG_CELLS RASTER_BLOCK /* cells of the grid per workgroup: one lane each */
#define RASTER_IMG_ASCII 0x10000u     /* a table entry whose glyph is one byte below 0x80 (the truecolor pen rule) */

/* the dithered mode (images_set_dithered, raster_dither_kernels.hpp): one workgroup per frame */
#define RASTER_DITHER_MAX_W ASCIICHAT_RASTER_MAX_COLS /* out_w a frame may have: the kernel's error line holds 3 x int per column */
#define RASTER_DITHER_CAP 16384                       /* samples of a band of text rows in LDS */
/* the launch's dynamic LDS: the staged composite descriptor (480 bytes), the error line, the band */
#define RASTER_DITHER_LDS_BYTES (480 + 12 * RASTER_DITHER_MAX_W + 4 * RASTER_DITHER_CAP)

/* what a mode's cells look up: the glyph of a luminance as an atlas slot, and the slots of the half-block modes' glyphs */
typedef struct {
  uint32_t slot[256]; /* Y -> slot (RASTER_NO_GLYPH: the atlas lacks it, or it is a space) | RASTER_IMG_ASCII; the dithered mode:
                         the slot of cache[Y] | the slot of cache[ramp[Y >> 2]] << 16, one table for its three styles */
  uint32_t fixed[8];  /* [0] U+2580, [1..3] U+2591 U+2592 U+2593, [4] U+2588; the rest 0 */
} raster_img_tables_t;

/* the last images_set of a handle, by value in the kernel arguments */
typedef struct {
  int32_t mode;                      /* ACHIP_MODE_* 0..8, or ACHIP_MODE_16_DITHER_BG for a set made by images_set_dithered */
  uint32_t mixed;                    /* TRUE_FG: the palette holds one-byte and multi-byte glyphs, so a pen can outlive its cell */
  const raster_img_tables_t *tables; /* device */
  const achip_frame_t *frames;       /* device, as many as were set */
} raster_img_args_t;

/* The parser's reading of a palette (asciichat_raster.h's grammar): NULL when every character is one cell and nothing else --
 * well-formed UTF-8 (no overlong form, no surrogate, nothing above U+10FFFF) without a C0 byte or DEL, which the grammar
 * treats as controls --, else what is wrong. */
static inline const char *raster_images_palette_check(const char *s) {
  if (!s || !s[0])
    return "no palette";
  const unsigned char *p = (const unsigned char *)s;
  while (*p) {
    const unsigned b = *p;
    if (b < 0x20u || b == 0x7Fu)
      return "a control byte in the palette";
    if (b < 0x80u) {
      p++;
      continue;
    }
    const int need = (b >= 0xC2u && b <= 0xDFu) ? 1 : (b >= 0xE0u && b <= 0xEFu) ? 2 : (b >= 0xF0u && b <= 0xF4u) ? 3 : 0;
    if (!need)
      return "the palette is not well-formed UTF-8";
    uint32_t cp = b & (need == 1 ? 0x1Fu : need == 2 ? 0x0Fu : 0x07u);
    for (int k = 1; k <= need; k++) { /* (a NUL is no continuation byte: the walk never passes the terminator) */
      if ((p[k] & 0xC0u) != 0x80u)
        return "the palette is not well-formed UTF-8";
      cp = cp << 6 | (p[k] & 0x3Fu);
    }
    if (cp < (need == 1 ? 0x80u : need == 2 ? 0x800u : 0x10000u) || (cp >= 0xD800u && cp <= 0xDFFFu) || cp > 0x10FFFFu)
      return "the palette is not well-formed UTF-8";
    p += need + 1;
  }
  return NULL;
}

/* NULL when images_set takes (mode, palette, frames[0..n-1]) for a handle of max_frames, else what is wrong; *bad (optional) is
 * the offending frame, -1 when it is none of them */
static inline const char *raster_images_check(int mode, const char *palette, const achip_frame_t *frames, int n, int max_frames,
                                              int *bad) {
  if (bad)
    *bad = -1;
  if (mode < ACHIP_MODE_MONO || mode > ACHIP_MODE_HB_MONO)
    return "mode outside 0..8 (the dithered mode goes through images_set_dithered)";
  const char *why = raster_images_palette_check(palette);
  if (why)
    return why;
  if (!frames || n < 1 || n > max_frames)
    return "no frames, or their number outside 1..max_frames";
  for (int i = 0; i < n; i++) {
    const achip_frame_t *f = &frames[i];
    if (bad)
      *bad = i;
    if (f->comp)
      return "a composite descriptor (composites stay on the text path)";
    if (!f->src)
      return "a descriptor without a source";
    if (f->src_w < 1 || f->src_h < 1 || f->out_w < 1 || f->out_h < 1 || f->pad_left < 0 || f->pad_top < 0)
      return "a size below 1, or a negative padding";
    if (!achip_desc_ratios_ok(f))
      return "(out_w - 1) * x_ratio or (out_h - 1) * y_ratio reaches 2^32";
    if (!achip_desc_extent_ok(f))
      return "a source that spans 4 GiB or more";
    if (f->ops & ACHIP_OP_DITHER_MASK)
      return "a dither bit in ops";
    if ((f->ops & ACHIP_OP_TINT) && (f->ops & ACHIP_OP_FG_OVERRIDE))
      return "TINT and FG_OVERRIDE together";
  }
  if (bad)
    *bad = -1;
  return NULL;
}

/* The same for images_set_composites: a frame may carry comp (a device-visible achip_composite_t the host cannot read, as a plan
 * takes it), and then its src is not read, src_w x src_h is the canvas the ratios were made for and the source-extent check has
 * nothing to measure; every other rule is the plain frame's.  *composites (optional): how many frames carry one. */
static inline const char *raster_images_composites_check(int mode, const char *palette, const achip_frame_t *frames, int n,
                                                         int max_frames, int *bad, int *composites) {
  if (bad)
    *bad = -1;
  if (composites)
    *composites = 0;
  if (mode < ACHIP_MODE_MONO || mode > ACHIP_MODE_HB_MONO)
    return "mode outside 0..8 (the dithered mode goes through images_set_dithered)";
  const char *why = raster_images_palette_check(palette);
  if (why)
    return why;
  if (!frames || n < 1 || n > max_frames)
    return "no frames, or their number outside 1..max_frames";
  int with_comp = 0;
  for (int i = 0; i < n; i++) {
    const achip_frame_t *f = &frames[i];
    if (bad)
      *bad = i;
    if (!f->src && !f->comp)
      return "a descriptor with neither a source nor a composite";
    if (f->src_w < 1 || f->src_h < 1 || f->out_w < 1 || f->out_h < 1 || f->pad_left < 0 || f->pad_top < 0)
      return "a size below 1, or a negative padding";
    if (!achip_desc_ratios_ok(f))
      return "(out_w - 1) * x_ratio or (out_h - 1) * y_ratio reaches 2^32";
    if (!f->comp && !achip_desc_extent_ok(f))
      return "a source that spans 4 GiB or more";
    if (f->ops & ACHIP_OP_DITHER_MASK)
      return "a dither bit in ops";
    if ((f->ops & ACHIP_OP_TINT) && (f->ops & ACHIP_OP_FG_OVERRIDE))
      return "TINT and FG_OVERRIDE together";
    with_comp += f->comp != NULL;
  }
  if (bad)
    *bad = -1;
  if (composites)
    *composites = with_comp;
  return NULL;
}

/* The same for images_set_dithered, whose mode is implied (ACHIP_MODE_16_DITHER_BG): images_set_composites' rules, except that
 * ops may carry the dither style bits -- none, DITHER_FG, or DITHER_FG | DITHER_RAMP; DITHER_RAMP alone names no form of the
 * renderer --, and out_w is bounded by RASTER_DITHER_MAX_W, which sizes the kernel's error line. */
static inline const char *raster_images_dithered_check(const char *palette, const achip_frame_t *frames, int n, int max_frames, int *bad,
                                                       int *composites) {
  if (bad)
    *bad = -1;
  if (composites)
    *composites = 0;
  const char *why = raster_images_palette_check(palette);
  if (why)
    return why;
  if (!frames || n < 1 || n > max_frames)
    return "no frames, or their number outside 1..max_frames";
  int with_comp = 0;
  for (int i = 0; i < n; i++) {
    const achip_frame_t *f = &frames[i];
    if (bad)
      *bad = i;
    if (!f->src && !f->comp)
      return "a descriptor with neither a source nor a composite";
    if (f->src_w < 1 || f->src_h < 1 || f->out_w < 1 || f->out_h < 1 || f->pad_left < 0 || f->pad_top < 0)
      return "a size below 1, or a negative padding";
    if (f->out_w > RASTER_DITHER_MAX_W)
      return "out_w above 1024 (no grid shows such a row)";
    if (!achip_desc_ratios_ok(f))
      return "(out_w - 1) * x_ratio or (out_h - 1) * y_ratio reaches 2^32";
    if (!f->comp && !achip_desc_extent_ok(f))
      return "a source that spans 4 GiB or more";
    if ((f->ops & ACHIP_OP_DITHER_MASK) == ACHIP_OP_DITHER_RAMP)
      return "DITHER_RAMP without DITHER_FG";
    if ((f->ops & ACHIP_OP_TINT) && (f->ops & ACHIP_OP_FG_OVERRIDE))
      return "TINT and FG_OVERRIDE together";
    with_comp += f->comp != NULL;
  }
  if (bad)
    *bad = -1;
  if (composites)
    *composites = with_comp;
  return NULL;
}

/* the parse kernel's lookup: the slot of a codepoint in the atlas' ascending codepoints */
static inline uint32_t raster_images_slot(const uint32_t *codepoints, int n_glyphs, int matrix_map, uint32_t cp) {
  if (cp == 0u || cp == 0x20u)
    return RASTER_NO_GLYPH;
  if (matrix_map && cp >= 32u && cp <= 126u)
    cp = 0xE900u + (cp - 32u) % 27u;
  int lo = 0, hi = n_glyphs;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (codepoints[mid] == cp)
      return (uint32_t)mid;
    if (codepoints[mid] < cp)
      lo = mid + 1;
    else
      hi = mid;
  }
  return RASTER_NO_GLYPH;
}

/* the codepoint of a glyph packed as achip_lut_t packs it (a checked palette: well-formed) */
static inline uint32_t raster_images_codepoint(uint32_t g) {
  const uint32_t b0 = g & 0xFFu, b1 = (g >> 8) & 0x3Fu, b2 = (g >> 16) & 0x3Fu, b3 = (g >> 24) & 0x3Fu;
  if (b0 < 0x80u)
    return b0;
  if (b0 < 0xE0u)
    return (b0 & 0x1Fu) << 6 | b1;
  if (b0 < 0xF0u)
    return (b0 & 0x0Fu) << 12 | b1 << 6 | b2;
  return (b0 & 0x07u) << 18 | b1 << 12 | b2 << 6 | b3;
}

/* The table of a checked (mode, palette) over an atlas' codepoints.  The glyph of a luminance is the renderers':
 * MONO cache64[ramp[Y >> 2]] (index clamped to 63), 16_FG cache[ramp[Y >> 2]], every other mode cache[Y].  Returns `mixed`. */
static inline uint32_t raster_images_tables(int mode, const char *palette, const uint32_t *codepoints, int n_glyphs, int matrix_map,
                                            raster_img_tables_t *t) {
  static const uint32_t fixed[5] = {0x2580u, 0x2591u, 0x2592u, 0x2593u, 0x2588u};
  achip_lut_t lut;
  memset(t, 0, sizeof(*t));
  if (achip_desc_lut_build(palette, &lut) != 0)
    return 0u;
  int ascii = 0, wide = 0;
  for (int y = 0; y < 256; y++) {
    const unsigned ramp = lut.ramp[y >> 2];
    const uint32_t g = mode == ACHIP_MODE_MONO ? lut.glyph64[ramp < 63u ? ramp : 63u] : mode == ACHIP_MODE_16_FG ? lut.glyph[ramp] : lut.glyph[y];
    const int one = (g & 0xFFu) < 0x80u;
    ascii |= one;
    wide |= !one;
    t->slot[y] = raster_images_slot(codepoints, n_glyphs, matrix_map, raster_images_codepoint(g)) | (one ? RASTER_IMG_ASCII : 0u);
  }
  for (int k = 0; k < 5; k++)
    t->fixed[k] = raster_images_slot(codepoints, n_glyphs, matrix_map, fixed[k]);
  return mode == ACHIP_MODE_TRUE_FG && ascii && wide ? 1u : 0u;
}

/* The table of a checked palette for the dithered mode, over an atlas' codepoints: entry Y holds the slot of cache[Y] (the
 * background form and DITHER_FG) in bits 15..0 and the slot of cache[ramp[Y >> 2]] (DITHER_FG | DITHER_RAMP) in bits 31..16;
 * a style is a frame's, so one table serves a set that mixes them. */
static inline void raster_images_dither_tables(const char *palette, const uint32_t *codepoints, int n_glyphs, int matrix_map,
                                               raster_img_tables_t *t) {
  achip_lut_t lut;
  memset(t, 0, sizeof(*t));
  if (achip_desc_lut_build(palette, &lut) != 0)
    return;
  for (int y = 0; y < 256; y++) {
    const uint32_t plain = raster_images_slot(codepoints, n_glyphs, matrix_map, raster_images_codepoint(lut.glyph[y]));
    const uint32_t ramp = raster_images_slot(codepoints, n_glyphs, matrix_map, raster_images_codepoint(lut.glyph[lut.ramp[y >> 2]]));
    t->slot[y] = plain | ramp << 16;
  }
}

/* where the handle keeps a set: the table, then max_frames descriptors, in one block on the device and one pinned on the host */
static inline size_t raster_images_at_frames(void) { return (sizeof(raster_img_tables_t) + 15u) & ~(size_t)15u; }
static inline size_t raster_images_bytes(int frames) { return raster_images_at_frames() + (size_t)frames * sizeof(achip_frame_t); }

/* the launcher (raster.hip); returns a hipError_t.  cells: n * rows * cols of the handle; 1 <= n <= the frames behind a->frames;
 * composites: some frame of the set carries comp (the kernel form with the staged composite sampler), 0: none does (a composite
 * frame in such a launch would be read as a plain one -- the host never lets that happen) */
int raster_launch_cells_images(const raster_params_t *p, const raster_img_args_t *a, int composites, int n, raster_cell_t *cells,
                               uint32_t *status, void *stream);

/* the dithered mode's launcher (raster.hip), one workgroup per frame; a->mode is ACHIP_MODE_16_DITHER_BG, the rest as above */
int raster_launch_cells_dither(const raster_params_t *p, const raster_img_args_t *a, int composites, int n, raster_cell_t *cells,
                               uint32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
