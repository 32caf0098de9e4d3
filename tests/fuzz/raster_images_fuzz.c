/*
 * raster_images_fuzz.c -- sanitizer fuzz of the host-only C behind asciichat_raster_images_set (ascii-chat_amd/csrc/
 * raster_images.h, achip_desc.h): the palette and descriptor checks and the table building, fed with seeded random and
 * malformed palettes in exact-size heap blocks and with random descriptors.  A program of its own, built with
 * -fsanitize=address,undefined by tests/test_raster_images_emulated.py; any report aborts the run.  Host code only.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "raster_images.h"

static uint32_t rng = 2463534242u;
static uint32_t rnd(void) {
  rng ^= rng << 13;
  rng ^= rng >> 17;
  rng ^= rng << 5;
  return rng;
}

/* a NUL-terminated palette in a block of exactly its size: a read past the terminator trips ASan */
static char *mkpalette(void) {
  static const char *good[] = {"   ...',;:clodxkO0KXNWM", "   \xe2\x96\x91\xe2\x96\x91\xe2\x96\x92\xe2\x96\x92\xe2\x96\x93\xe2\x96\x93\xe2\x96\x88\xe2\x96\x88",
                               "#", ".:\xe2\x96\x92\xe2\x96\x88", "\xf0\x9f\x98\x80 \xc3\xa9"};
  const uint32_t kind = rnd() % 4;
  size_t n;
  char *s;
  if (kind == 0) {
    const char *g = good[rnd() % 5];
    n = strlen(g);
    s = malloc(n + 1);
    memcpy(s, g, n + 1);
    if (rnd() % 3 == 0 && n > 1) /* cut anywhere: a sequence may end early */
      s[rnd() % n] = '\0';
  } else {
    n = rnd() % (kind == 1 ? 8 : 300);
    s = malloc(n + 1);
    for (size_t i = 0; i < n; i++) {
      const uint32_t r = rnd() % 8;
      s[i] = (char)(r == 0 ? 0xC2 + rnd() % 0x33 : r == 1 ? 0x80 + rnd() % 0x40 : r == 2 ? 0xE0 + rnd() % 0x18 : r == 3 ? 1 + rnd() % 255 : ' ' + rnd() % 95);
      if (!s[i])
        s[i] = 'x';
    }
    s[n] = '\0';
  }
  char *exact = malloc(strlen(s) + 1);
  memcpy(exact, s, strlen(s) + 1);
  free(s);
  return exact;
}

static int32_t edge(void) {
  static const int32_t v[] = {0, 1, 2, -1, 3840, 10000, INT32_MAX, INT32_MIN, 65536, 1 << 24, (1 << 24) - 1};
  return rnd() % 3 ? (int32_t)(rnd() % 64) + 1 : v[rnd() % (sizeof v / sizeof v[0])];
}

int main(int argc, char **argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 5000;
  uint32_t codepoints[128];
  int ng = 0;
  for (uint32_t cp = 33; cp < 127; cp += 1 + (cp % 5 == 0)) /* ascending, with holes */
    codepoints[ng++] = cp;
  codepoints[ng++] = 0x2580;
  codepoints[ng++] = 0x2592;
  codepoints[ng++] = 0xE900;
  long taken = 0, refused = 0;
  static uint8_t pixel[4];
  for (int it = 0; it < iters; it++) {
    char *pal = mkpalette();
    const int n = (int)(rnd() % 5), max_frames = (int)(rnd() % 6);
    achip_frame_t *frames = n ? malloc((size_t)n * sizeof(*frames)) : NULL;
    for (int i = 0; i < n; i++) {
      achip_frame_t *f = &frames[i];
      memset(f, 0, sizeof(*f));
      f->src = rnd() % 16 ? pixel : NULL;
      f->comp = rnd() % 16 ? NULL : (const achip_composite_t *)pixel;
      f->src_w = edge(), f->src_h = edge(), f->out_w = edge(), f->out_h = edge();
      f->pad_left = rnd() % 4 ? (int32_t)(rnd() % 9) : edge(), f->pad_top = rnd() % 4 ? (int32_t)(rnd() % 5) : edge();
      f->x_ratio = rnd() % 4 ? (uint32_t)((((uint64_t)(uint32_t)f->src_w << 16) / (uint32_t)(f->out_w ? f->out_w : 1)) + 1u) : rnd();
      f->y_ratio = rnd() % 4 ? (uint32_t)((((uint64_t)(uint32_t)f->src_h << 16) / (uint32_t)(f->out_h ? f->out_h : 1)) + 1u) : rnd();
      f->src_stride = rnd() % 3 ? 0 : edge();
      f->ops = rnd() % 3 ? rnd() % 4 : rnd();
    }
    const int mode = (int)(rnd() % 12) - 1;
    int bad = 12345;
    const char *why = raster_images_check(mode, rnd() % 50 ? pal : NULL, frames, n, max_frames, &bad);
    if (bad < -1 || bad >= (n > 0 ? n : 1))
      abort();
    const char *pwhy = raster_images_palette_check(pal);
    if (!why) {
      taken++;
      if (pwhy || mode < 0 || mode > 8 || n < 1 || n > max_frames)
        abort();
    } else {
      refused++;
    }
    if (!pwhy) { /* the tables of every checked palette: every slot in the atlas or none, the flag only on one-byte glyphs */
      for (int m = 0; m <= 8; m++) {
        raster_img_tables_t *t = malloc(sizeof(*t));
        const uint32_t mixed = raster_images_tables(m, pal, codepoints, rnd() % 2 ? ng : 0, (int)(rnd() % 2), t);
        if (mixed > 1u || (mixed && m != ACHIP_MODE_TRUE_FG))
          abort();
        for (int y = 0; y < 256; y++) {
          const uint32_t s = t->slot[y] & 0xFFFFu;
          if ((t->slot[y] & ~(0xFFFFu | RASTER_IMG_ASCII)) || (s != RASTER_NO_GLYPH && s >= (uint32_t)ng))
            abort();
        }
        for (int k = 0; k < 8; k++)
          if (t->fixed[k] != RASTER_NO_GLYPH && t->fixed[k] >= (uint32_t)ng && !(k >= 5 && t->fixed[k] == 0u))
            abort();
        free(t);
      }
    }
    free(frames);
    free(pal);
  }
  if (!taken || !refused)
    abort();
  printf("raster images fuzz ok: %ld sets taken, %ld refused\n", taken, refused);
  return 0;
}
