/* pix_math.h -- the addressing and the permutation of the packed RGB sources (include/asciichat_pix.h states the rule and the
 * four layouts), with the sampling rule, the box bounds and the pure-C checks of a source and of a set beside them: one text for
 * the kernels (pix_kernels.hpp), the host (pix.c), the host walks (pix.h), the emulator driver and the sanitizer program of the
 * tests.  Plain C; __host__ __device__ under hipcc.  Not installed. */
#ifndef ASCIICHAT_PIX_MATH_H
#define ASCIICHAT_PIX_MATH_H

#include "achip_desc.h"
#include "asciichat_pix.h"

#if defined(__HIPCC__)
#define PIX_FN __host__ __device__ static inline
#else
#define PIX_FN static inline
#endif

#define PIX_MAX_SIDE 8192
#define PIX_MAX_STRIDE (1 << 24) /* exclusive */
#define PIX_MAX_FRAMES 65535
#define PIX_BLOCK 256 /* threads of every workgroup */
#define PIX_BOX_MAX_SRC_W 3840 /* the box pass's limits: the LDS stage holds 3 * width column sums (45 KB) */
#define PIX_BOX_MAX_SRC_H 2160
#define PIX_BOX_MAX_OUT 16384 /* (out * src) stays far below 2^32 in the box bounds */

/* ---- the layouts: bit 0 of a format says "a fourth byte", bit 1 "blue first" ---- */
PIX_FN int32_t pix_bpp(int32_t format) { return 3 + (format & 1); }
PIX_FN int32_t pix_swapped(int32_t format) { return (format >> 1) & 1; }
/* byte offset of pixel (sx, sy); rows are 64-bit (8191 rows of 2^24 - 1 bytes) */
PIX_FN int64_t pix_at(int64_t stride, int32_t bpp, int32_t sx, int32_t sy) { return (int64_t)sy * stride + (int64_t)bpp * sx; }

/* ---- the permutation: R | G << 8 | B << 16 ---- */
/* of a pixel's first three bytes read as a little-endian word (whatever bits 31..24 hold is dropped) */
PIX_FN uint32_t pix_word_rgb(uint32_t word, int32_t swapped) {
  return swapped ? ((word >> 16) & 0xFFu) | (word & 0xFF00u) | (word & 0xFFu) << 16 : word & 0xFFFFFFu;
}
PIX_FN uint32_t pix_bytes_rgb(uint32_t b0, uint32_t b1, uint32_t b2, int32_t swapped) {
  return swapped ? b2 | b1 << 8 | b0 << 16 : b0 | b1 << 8 | b2 << 16;
}
/* pixel (sx, sy) of a checked, resolved source: three byte loads */
PIX_FN uint32_t pix_pixel(const asciichat_pix_source_t *s, int32_t sx, int32_t sy) {
  const uint8_t *p = s->pixels + pix_at(s->stride, pix_bpp(s->format), sx, sy);
  return pix_bytes_rgb(p[0], p[1], p[2], pix_swapped(s->format));
}

/* the renderers' sampling rule (achip_types.h): the source pixel of image pixel (x, y) of a checked descriptor */
PIX_FN void pix_sample_at(const achip_frame_t *f, int32_t x, int32_t y, int32_t *sx, int32_t *sy) {
  uint32_t cx = ((uint32_t)x * f->x_ratio) >> 16, cy = ((uint32_t)y * f->y_ratio) >> 16;
  if (cx > (uint32_t)f->src_w - 1u)
    cx = (uint32_t)f->src_w - 1u;
  if (cy > (uint32_t)f->src_h - 1u)
    cy = (uint32_t)f->src_h - 1u;
  *sx = (f->ops & ACHIP_OP_FLIP_X) ? f->src_w - 1 - (int32_t)cx : (int32_t)cx;
  *sy = (f->ops & ACHIP_OP_FLIP_Y) ? f->src_h - 1 - (int32_t)cy : (int32_t)cy;
}

/* the box of output index i on one axis of `src` pixels averaged to `out` (achip_box_bounds' rule, restated: that one lives in
 * libasciichat_hip.so, of which this library links nothing; tests/test_pix_emulated.py pins the two against box_ref) */
PIX_FN void pix_bounds(uint32_t src, uint32_t out, uint32_t i, uint32_t *lo, uint32_t *hi) {
  *lo = i * src / out;
  const uint32_t h = (i + 1u) * src / out;
  *hi = h > *lo + 1u ? h : *lo + 1u;
}

/* ---- the checks (host), in the order of the header's sentences ---- */
/* NULL when a source is taken, else what is wrong */
static inline const char *pix_source_check(const asciichat_pix_source_t *s) {
  if (!s)
    return "no source";
  if (s->format < ASCIICHAT_PIX_RGB || s->format > ASCIICHAT_PIX_BGRA)
    return "format outside 0..3";
  if (s->width < 1 || s->width > PIX_MAX_SIDE || s->height < 1 || s->height > PIX_MAX_SIDE)
    return "width or height outside 1..8192";
  if (s->stride < 0 || s->stride >= PIX_MAX_STRIDE)
    return "a stride outside 0..2^24 - 1";
  if (s->stride != 0 && s->stride < pix_bpp(s->format) * s->width)
    return "a stride below bpp * width";
  if (!s->pixels)
    return "no pixels";
  return NULL;
}

/* whether the box pass takes a checked source */
static inline int pix_source_boxable(const asciichat_pix_source_t *s) {
  return s->width <= PIX_BOX_MAX_SRC_W && s->height <= PIX_BOX_MAX_SRC_H;
}

/* a checked source as the kernels take it: the stride stated */
static inline asciichat_pix_source_t pix_source_resolved(const asciichat_pix_source_t *s) {
  asciichat_pix_source_t r = *s;
  if (!r.stride)
    r.stride = pix_bpp(s->format) * s->width;
  return r;
}

/* NULL when set() takes (sources[0..n-1], frames[0..n-1] or no frames) for a handle of max_frames, else what is wrong.
 * *bad (optional): the offending entry, -1 when it is none of them; *unsupported (optional): 1 when the refusal is a
 * composite descriptor (ERR_NOT_SUPPORTED rather than ERR_INVALID_PARAM). */
static inline const char *pix_set_check(const asciichat_pix_source_t *sources, const achip_frame_t *frames, int n, int max_frames, int *bad,
                                        int *unsupported) {
  if (bad)
    *bad = -1;
  if (unsupported)
    *unsupported = 0;
  if (!sources || n < 1 || n > max_frames)
    return "no sources, or their number outside 1..max_frames";
  for (int i = 0; i < n; i++) {
    if (bad)
      *bad = i;
    const char *why = pix_source_check(&sources[i]);
    if (why)
      return why;
    if (!frames)
      continue;
    const achip_frame_t *f = &frames[i];
    if (f->comp) {
      if (unsupported)
        *unsupported = 1;
      return "a composite descriptor (its packed tiles go through asciichat_pixgrid_*, a library of its own)";
    }
    if (f->src_w != sources[i].width || f->src_h != sources[i].height)
      return "src_w x src_h of the descriptor is not the source's size";
    if (f->out_w < 1 || f->out_h < 1 || (uint64_t)f->out_w * (uint64_t)f->out_h > 0x7FFFFFFFull / 3u)
      return "an image size below 1, or an image of 2^31 bytes or more";
    if (!achip_desc_ratios_ok(f))
      return "(out_w - 1) * x_ratio or (out_h - 1) * y_ratio reaches 2^32";
  }
  if (bad)
    *bad = -1;
  return NULL;
}

/* whether run_box serves a checked set with descriptors: every source and every image side within the box pass's limits */
static inline int pix_set_boxable(const asciichat_pix_source_t *sources, const achip_frame_t *frames, int n) {
  for (int i = 0; i < n; i++)
    if (!pix_source_boxable(&sources[i]) || frames[i].out_w > PIX_BOX_MAX_OUT || frames[i].out_h > PIX_BOX_MAX_OUT)
      return 0;
  return 1;
}

/* where the handle keeps a set of n: n resolved sources, then n descriptors (16-aligned), in one block */
static inline size_t pix_set_at_frames(int n) { return ((size_t)n * sizeof(asciichat_pix_source_t) + 15u) & ~(size_t)15u; }
static inline size_t pix_set_bytes(int n) { return pix_set_at_frames(n) + (size_t)n * sizeof(achip_frame_t); }

#endif
