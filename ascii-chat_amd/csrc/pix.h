/* pix.h -- what the host side of libasciichat_pix.so (pix.c) and its launchers (pix.hip, kernels in pix_kernels.hpp) share: the
 * arguments that travel by value, the rule of include/asciichat_pix.h walked on the host for each of the three passes (the
 * emulator driver and the sanitizer program of the tests call them, never the library), and the launchers.  Not installed. */
#ifndef ASCIICHAT_PIX_PRIV_H
#define ASCIICHAT_PIX_PRIV_H

#include <string.h>

#include "pix_math.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PIX_WHOLE_LANES_X 64 /* a workgroup of the whole conversion: 64 x 4 lanes, one run of pixels of one row each */
#define PIX_WHOLE_LANES_Y (PIX_BLOCK / PIX_WHOLE_LANES_X)
/* the pixels of a lane's run in whole_kernel: 4 (16 or 12 bytes in, 12 out) or 16 (64 or 48 in, 48 out as three 16-byte
 * stores).  Both were measured (scripts/pix_timing.py, profiles/pix_timing.txt: 256 BGRA / BGR24 1080p sources in 645.9 /
 * 550.5 us at 4, 855.0 / 685.9 us at 16); the library ships 4, and make EXTRA=-DPIX_WHOLE_PIXELS=16 BUILD=build_pix16
 * PIXOUT=libasciichat_pix16.so libasciichat_pix16.so builds the other for that script.  The tests run both under the emulator. */
#ifndef PIX_WHOLE_PIXELS
#define PIX_WHOLE_PIXELS 4
#endif

/* a whole conversion, by value in the kernel arguments */
typedef struct {
  const asciichat_pix_source_t *sources; /* device, resolved, one per image; NULL: `one` is the only source */
  asciichat_pix_source_t one;            /* resolved */
  uint8_t *rgb;                          /* image i at rgb + i * pitch */
  uint64_t pitch;
  int32_t rgb_stride; /* bytes per image row; 0: tight, 3 * width of each source */
  int32_t _pad;
} pix_whole_args_t;

/* a box pass, by value in the kernel arguments */
typedef struct {
  const asciichat_pix_source_t *sources; /* device, resolved; NULL: `one` averaged to one_w x one_h under one_flips */
  const achip_frame_t *frames;           /* device: out_w, out_h and the flip bits of ops are read */
  asciichat_pix_source_t one;            /* resolved */
  int32_t one_w, one_h;
  uint32_t one_flips;
  uint32_t rows_per_image; /* the largest out_h of the launch */
  uint8_t *images;         /* image i at images + i * pitch */
  uint64_t pitch;
} pix_box_args_t;

/* ---- THE RULE on the host, pixel by pixel, of a checked and resolved source (host-readable pixels): what the kernels must
 * leave; walked by the tests and by the sanitizer program, never by the library ---- */
/* the whole conversion: row y at out + y * row_bytes (row_bytes >= 3 * width) */
static inline void pix_host_whole(const asciichat_pix_source_t *s, uint8_t *out, size_t row_bytes) {
  for (int32_t y = 0; y < s->height; y++)
    for (int32_t x = 0; x < s->width; x++) {
      const uint32_t p = pix_pixel(s, x, y);
      uint8_t *o = out + (size_t)y * row_bytes + 3u * (size_t)x;
      o[0] = (uint8_t)p, o[1] = (uint8_t)(p >> 8), o[2] = (uint8_t)(p >> 16);
    }
}
/* the sampled image of a checked descriptor: 3 * out_w * out_h bytes */
static inline void pix_host_sample(const asciichat_pix_source_t *s, const achip_frame_t *f, uint8_t *out) {
  for (int32_t y = 0; y < f->out_h; y++)
    for (int32_t x = 0; x < f->out_w; x++) {
      int32_t sx, sy;
      pix_sample_at(f, x, y, &sx, &sy);
      const uint32_t p = pix_pixel(s, sx, sy);
      uint8_t *o = out + 3u * ((size_t)y * (size_t)f->out_w + (size_t)x);
      o[0] = (uint8_t)p, o[1] = (uint8_t)(p >> 8), o[2] = (uint8_t)(p >> 16);
    }
}
/* the box average to out_w x out_h (1..PIX_BOX_MAX_OUT each) under the flip bits of `flips`: 3 * out_w * out_h bytes */
static inline void pix_host_box(const asciichat_pix_source_t *s, int32_t out_w, int32_t out_h, uint32_t flips, uint8_t *out) {
  const uint32_t w = (uint32_t)s->width, h = (uint32_t)s->height, ow = (uint32_t)out_w, oh = (uint32_t)out_h;
  for (uint32_t y = 0; y < oh; y++) {
    uint32_t y0, y1;
    pix_bounds(h, oh, (flips & ACHIP_OP_FLIP_Y) ? oh - 1u - y : y, &y0, &y1);
    for (uint32_t x = 0; x < ow; x++) {
      uint32_t x0, x1;
      pix_bounds(w, ow, (flips & ACHIP_OP_FLIP_X) ? ow - 1u - x : x, &x0, &x1);
      uint32_t sum[3] = {0u, 0u, 0u};
      for (uint32_t sy = y0; sy < y1; sy++)
        for (uint32_t sx = x0; sx < x1; sx++) {
          const uint32_t p = pix_pixel(s, (int32_t)sx, (int32_t)sy);
          sum[0] += p & 0xFFu, sum[1] += (p >> 8) & 0xFFu, sum[2] += p >> 16;
        }
      const uint32_t n = (x1 - x0) * (y1 - y0);
      for (int c = 0; c < 3; c++)
        out[3u * ((size_t)y * ow + x) + (unsigned)c] = (uint8_t)((sum[c] + n / 2u) / n);
    }
  }
}

/* the bytes of dynamic LDS a box launch needs: 3 * max_src_w column sums of 32 bits */
static inline size_t pix_box_lds_bytes(int max_src_w) { return ((size_t)12 * (size_t)max_src_w + 15u) & ~(size_t)15u; }

/* The launchers (pix.hip); each returns a hipError_t.  Arguments are the host's to check: nothing is checked again there but
 * what keeps a grid legal.
 * sample: image i of n from sources[i] under frames[i]; max_pixels: the largest out_w * out_h among them */
int pix_launch_sample(const asciichat_pix_source_t *sources, const achip_frame_t *frames, int n, uint32_t max_pixels, uint8_t *images,
                      uint64_t pitch, void *stream);
/* whole: n images; max_w, max_h: the largest width and height among the sources; bpps: bit 0 set when some source has 3 bytes
 * per pixel, bit 1 when some has 4 -- one launch per bpp present, whose workgroups leave the images of the other alone */
int pix_launch_whole(const pix_whole_args_t *a, int n, int max_w, int max_h, unsigned bpps, void *stream);
/* box: n images (a->rows_per_image the largest out_h); max_src_w: the widest source of the launch */
int pix_launch_box(const pix_box_args_t *a, int n, int max_src_w, void *stream);

#ifdef __cplusplus
}
#endif
#endif
