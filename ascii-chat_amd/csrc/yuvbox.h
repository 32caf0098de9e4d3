/* yuvbox.h -- what the host side of libasciichat_yuvbox.so (yuvbox.c) and its launcher (yuvbox.hip, the kernel in
 * yuvbox_kernels.hpp) share: the item a workgroup reads, the pure-C checks of a set, the rule of include/asciichat_yuvbox.h
 * walked on the host (the emulator driver and the sanitizer program of the tests call both), and the launcher.  Not installed. */
#ifndef ASCIICHAT_YUVBOX_PRIV_H
#define ASCIICHAT_YUVBOX_PRIV_H

#include <string.h>

#include "asciichat_yuvbox.h"
#include "yuv_math.h"

#ifdef __cplusplus
extern "C" {
#endif

#define YUVBOX_MAX_SRC_W 3840 /* the box pass's limits: the LDS stage holds 3 * width column sums (45 KB) */
#define YUVBOX_MAX_SRC_H 2160
#define YUVBOX_MAX_OUT 16384 /* (out * src) stays far below 2^32 in the box bounds */

/* one image of a set, as a workgroup reads it */
typedef struct {
  asciichat_yuv_source_t src; /* resolved (no stride 0) */
  int32_t out_w, out_h;       /* 1..YUVBOX_MAX_OUT each */
  uint32_t flips;             /* ACHIP_OP_FLIP_X | ACHIP_OP_FLIP_Y, applied to the averaged image */
  uint32_t _pad;
} yuvbox_item_t;

/* the box of output index i on one axis of `src` pixels averaged to `out` (achip_box_bounds' rule) */
YUV_FN void yuvbox_bounds(uint32_t src, uint32_t out, uint32_t i, uint32_t *lo, uint32_t *hi) {
  *lo = i * src / out;
  const uint32_t h = (i + 1u) * src / out;
  *hi = h > *lo + 1u ? h : *lo + 1u;
}

/* NULL when a source is one the pass takes, else what is wrong: yuv_source_check and the box pass's size limit */
static inline const char *yuvbox_source_check(const asciichat_yuv_source_t *s) {
  const char *why = yuv_source_check(s);
  if (why)
    return why;
  if (s->width > YUVBOX_MAX_SRC_W || s->height > YUVBOX_MAX_SRC_H)
    return "a source larger than 3840 x 2160";
  return NULL;
}

/* NULL when set() takes (sources[0..n-1], frames[0..n-1]) for a handle of max_frames, else what is wrong.  *bad (optional):
 * the offending entry, -1 when it is none of them; *unsupported (optional): 1 when the refusal is a composite descriptor
 * (ERR_NOT_SUPPORTED rather than ERR_INVALID_PARAM).  x_ratio / y_ratio, src and src_stride are not read. */
static inline const char *yuvbox_set_check(const asciichat_yuv_source_t *sources, const achip_frame_t *frames, int n, int max_frames, int *bad,
                                           int *unsupported) {
  if (bad)
    *bad = -1;
  if (unsupported)
    *unsupported = 0;
  if (!sources || !frames)
    return "sources and descriptors are both required";
  if (n < 1 || n > max_frames)
    return "the number of sources outside 1..max_frames";
  for (int i = 0; i < n; i++) {
    if (bad)
      *bad = i;
    const char *why = yuvbox_source_check(&sources[i]);
    if (why)
      return why;
    const achip_frame_t *f = &frames[i];
    if (f->comp) {
      if (unsupported)
        *unsupported = 1;
      return "a composite descriptor";
    }
    if (f->src_w != sources[i].width || f->src_h != sources[i].height)
      return "src_w x src_h of the descriptor is not the source's size";
    if (f->out_w < 1 || f->out_h < 1 || f->out_w > YUVBOX_MAX_OUT || f->out_h > YUVBOX_MAX_OUT)
      return "out_w or out_h outside 1..16384";
  }
  if (bad)
    *bad = -1;
  return NULL;
}

/* the item of a checked source and image size */
static inline yuvbox_item_t yuvbox_item(const asciichat_yuv_source_t *s, int32_t out_w, int32_t out_h, uint32_t flips) {
  yuvbox_item_t it;
  memset(&it, 0, sizeof(it));
  it.src = yuv_source_resolved(s);
  it.out_w = out_w;
  it.out_h = out_h;
  it.flips = flips & (ACHIP_OP_FLIP_X | ACHIP_OP_FLIP_Y);
  return it;
}

/* THE RULE on the host, pixel by pixel: the image of an item, 3 * out_w * out_h bytes at `out` (host-readable planes).  What
 * the kernel must leave; walked by the tests and by the sanitizer program, never by the library. */
static inline void yuvbox_host_image(const yuvbox_item_t *it, uint8_t *out) {
  const yuv_layout_t l = yuv_layout(&it->src);
  const uint32_t w = (uint32_t)it->src.width, h = (uint32_t)it->src.height, ow = (uint32_t)it->out_w, oh = (uint32_t)it->out_h;
  for (uint32_t y = 0; y < oh; y++) {
    uint32_t y0, y1;
    yuvbox_bounds(h, oh, (it->flips & ACHIP_OP_FLIP_Y) ? oh - 1u - y : y, &y0, &y1);
    for (uint32_t x = 0; x < ow; x++) {
      uint32_t x0, x1;
      yuvbox_bounds(w, ow, (it->flips & ACHIP_OP_FLIP_X) ? ow - 1u - x : x, &x0, &x1);
      uint32_t s[3] = {0u, 0u, 0u};
      for (uint32_t sy = y0; sy < y1; sy++)
        for (uint32_t sx = x0; sx < x1; sx++) {
          const uint32_t p = yuv_pixel(&l, (int32_t)sx, (int32_t)sy);
          s[0] += p & 0xFFu, s[1] += (p >> 8) & 0xFFu, s[2] += p >> 16;
        }
      const uint32_t n = (x1 - x0) * (y1 - y0);
      for (int c = 0; c < 3; c++)
        out[3u * ((size_t)y * ow + x) + (unsigned)c] = (uint8_t)((s[c] + n / 2u) / n);
    }
  }
}

/* the bytes of dynamic LDS a launch needs: 3 * max_src_w column sums of 32 bits */
static inline size_t yuvbox_lds_bytes(int max_src_w) { return ((size_t)12 * (size_t)max_src_w + 15u) & ~(size_t)15u; }

/* The launcher (yuvbox.hip); returns a hipError_t.  Arguments are the host's to check: nothing is checked again there but what
 * keeps a grid legal.  Image i of n from items_dev[i] (device), or with items_dev NULL the one image of *one (by value in the
 * kernel arguments), to images + i * pitch; max_out_h / max_src_w: the largest of the launch. */
int yuvbox_launch(const yuvbox_item_t *items_dev, const yuvbox_item_t *one, int n, int max_out_h, int max_src_w, uint8_t *images, uint64_t pitch,
                  void *stream);

#ifdef __cplusplus
}
#endif
#endif
