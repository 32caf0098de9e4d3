/*
 * raster_dither_fuzz.c -- sanitizer fuzz of the host-only C behind asciichat_raster_images_set_dithered (ascii-chat_amd/csrc/
 * raster_images.h, achip_desc.h): the check of a batch, fed with seeded random descriptors in an exact-size heap block and
 * compared with a restatement of the rule and with images_set_composites' own check, and the glyph table of the mode's three
 * styles, built over an exact-size codepoint list and compared with the table of the plain modes.  The composite pointers are
 * never dereferenced by the host (they are device addresses): here they point at NOTHING readable (a freed block), so a read
 * through one trips ASan.  A program of its own, built with -fsanitize=address,undefined by
 * tests/test_raster_dither_emulated.py; any report aborts the run.  Host code only.
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

static int32_t edge(void) {
  static const int32_t v[] = {0, 1, 2, -1, 1024, 1025, 3840, INT32_MAX, INT32_MIN, 65536, 1 << 24, (1 << 24) - 1};
  return rnd() % 3 ? (int32_t)(rnd() % 64) + 1 : v[rnd() % (sizeof v / sizeof v[0])];
}

/* the rule of include/asciichat_raster.h for one frame of this entry, restated; *plain: images_set_composites' rule */
static int frame_ok(const achip_frame_t *f, int *plain) {
  *plain = 0;
  if (!f->src && !f->comp)
    return 0;
  if (f->src_w < 1 || f->src_h < 1 || f->out_w < 1 || f->out_h < 1 || f->pad_left < 0 || f->pad_top < 0)
    return 0;
  if ((uint64_t)(f->out_w - 1) * f->x_ratio >> 32 || (uint64_t)(f->out_h - 1) * f->y_ratio >> 32)
    return 0;
  if (!f->comp) {
    if (f->src_stride < 0)
      return 0;
    const uint64_t stride = f->src_stride ? (uint64_t)f->src_stride : 3ull * (uint64_t)f->src_w;
    if (stride >= (1ull << 24) || (uint64_t)(f->src_h - 1) * stride + 3ull * (uint64_t)f->src_w >= 0xFFFFFFF0ull)
      return 0;
  }
  if ((f->ops & ACHIP_OP_TINT) && (f->ops & ACHIP_OP_FG_OVERRIDE))
    return 0;
  *plain = !(f->ops & ACHIP_OP_DITHER_MASK);
  if (f->out_w > 1024)
    return 0;
  return (f->ops & ACHIP_OP_DITHER_MASK) != ACHIP_OP_DITHER_RAMP;
}

int main(int argc, char **argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 5000;
  static const char *palettes[] = {"   ...',;:clodxkO0KXNWM", ".:\xe2\x96\x92\xe2\x96\x88", "#", "", "a\x1b[0m", "a\xe2\x96"};
  static uint8_t pixel[4];
  void *gone = malloc(sizeof(achip_composite_t)); /* an address no host code may read */
  free(gone);
  long taken = 0, refused = 0, with_comp = 0, styled = 0, wide = 0, tables = 0;
  for (int it = 0; it < iters; it++) {
    const int n = (int)(rnd() % 5), max_frames = (int)(rnd() % 6);
    achip_frame_t *frames = n ? malloc((size_t)n * sizeof(*frames)) : NULL;
    int comps = 0, all_ok = 1, first_bad = -1, all_plain = 1, any_style = 0;
    for (int i = 0; i < n; i++) {
      achip_frame_t *f = &frames[i];
      memset(f, 0, sizeof(*f));
      f->src = rnd() % 3 ? pixel : NULL;
      f->comp = rnd() % 3 ? NULL : (const achip_composite_t *)gone;
      const int wild = rnd() % 6 == 0;
      f->src_w = wild ? edge() : 1 + (int32_t)(rnd() % 64), f->src_h = wild ? edge() : 1 + (int32_t)(rnd() % 64);
      f->out_w = wild ? edge() : 1 + (int32_t)(rnd() % 64), f->out_h = wild ? edge() : 1 + (int32_t)(rnd() % 64);
      if (rnd() % 16 == 0)
        f->out_w = 1023 + (int32_t)(rnd() % 4);
      f->pad_left = rnd() % 8 ? (int32_t)(rnd() % 9) : edge(), f->pad_top = rnd() % 8 ? (int32_t)(rnd() % 5) : edge();
      f->x_ratio = rnd() % 8 ? (uint32_t)((((uint64_t)(uint32_t)f->src_w << 16) / (uint32_t)(f->out_w ? f->out_w : 1)) + 1u) : rnd();
      f->y_ratio = rnd() % 8 ? (uint32_t)((((uint64_t)(uint32_t)f->src_h << 16) / (uint32_t)(f->out_h ? f->out_h : 1)) + 1u) : rnd();
      f->src_stride = rnd() % 4 ? 0 : edge();
      f->ops = rnd() % 8 ? (rnd() % 4) | (rnd() % 4 ? 0u : ACHIP_OP_FG_OVERRIDE) | (rnd() % 3 ? 0u : (rnd() % 4) << 4) : rnd();
      comps += f->comp != NULL;
      int plain = 0;
      const int ok = frame_ok(f, &plain);
      if (all_ok && !ok) {
        all_ok = 0;
        first_bad = i;
      }
      all_plain &= ok && plain;
      any_style |= (f->ops & ACHIP_OP_DITHER_MASK) != 0u;
      wide += ok && f->out_w == 1024;
    }
    const char *pal = rnd() % 40 ? palettes[rnd() % 6] : NULL;
    int bad = 12345, got_comps = 12345;
    const char *why = raster_images_dithered_check(pal, frames, n, max_frames, &bad, &got_comps);
    if (bad < -1 || bad >= (n > 0 ? n : 1))
      abort();
    const int head_ok = !raster_images_palette_check(pal) && frames && n >= 1 && n <= max_frames;
    if ((why == NULL) != (head_ok && all_ok)) /* taken exactly when the restated rule takes it */
      abort();
    if (!why) {
      taken++;
      if (bad != -1 || got_comps != comps)
        abort();
      with_comp += comps > 0;
      styled += any_style;
    } else {
      refused++;
      if (got_comps != 0 || (head_ok && bad != first_bad) || (!head_ok && bad != -1))
        abort();
    }
    /* optional outputs may be absent */
    if ((raster_images_dithered_check(pal, frames, n, max_frames, NULL, NULL) == NULL) != (why == NULL))
      abort();
    /* a set without a dither bit: taken here exactly when images_set_composites takes it in a mode of its own; one with a
     * dither bit that is taken here is refused there; and mode 9 is refused there whatever the set */
    const char *other = raster_images_composites_check(ACHIP_MODE_TRUE_FG, pal, frames, n, max_frames, NULL, NULL);
    if (head_ok && all_ok && (other == NULL) != (all_plain != 0))
      abort();
    if (!raster_images_composites_check(ACHIP_MODE_16_DITHER_BG, pal, frames, n, max_frames, NULL, NULL) ||
        !raster_images_check(ACHIP_MODE_16_DITHER_BG, pal, frames, n, max_frames, NULL))
      abort();
    free(frames);

    /* the table: over an exact-size ascending codepoint list; its low halves are the table of a cache[Y] mode, its high
     * halves that of the cache[ramp[Y >> 2]] mode */
    if (it % 16 == 0 && pal && !raster_images_palette_check(pal)) {
      const int ng = (int)(rnd() % 40), matrix = (int)(rnd() & 1u);
      uint32_t *cps = ng ? malloc((size_t)ng * sizeof(*cps)) : NULL;
      uint32_t cp = 0x20u + rnd() % 4u;
      for (int k = 0; k < ng; k++, cp += 1u + rnd() % (matrix ? 0x700u : 9u))
        cps[k] = k == ng / 2 && ng > 4 ? (cp = 0x2592u > cp ? 0x2592u : cp) : cp;
      raster_img_tables_t *t = malloc(sizeof(*t)), *a = malloc(sizeof(*a)), *b = malloc(sizeof(*b));
      raster_images_dither_tables(pal, cps, ng, matrix, t);
      (void)raster_images_tables(ACHIP_MODE_256_FG, pal, cps, ng, matrix, a);
      (void)raster_images_tables(ACHIP_MODE_16_FG, pal, cps, ng, matrix, b);
      for (int y = 0; y < 256; y++)
        if ((t->slot[y] & 0xFFFFu) != (a->slot[y] & 0xFFFFu) || t->slot[y] >> 16 != (b->slot[y] & 0xFFFFu))
          abort();
      for (int k = 0; k < 8; k++)
        if (t->fixed[k])
          abort();
      free(t), free(a), free(b), free(cps);
      tables++;
    }
  }
  if (!taken || !refused || !with_comp || !styled || !wide || !tables)
    abort();
  printf("raster dither fuzz ok: %ld sets taken (%ld with composites, %ld with a style), %ld refused, %ld tables\n", taken, with_comp, styled,
         refused, tables);
  return 0;
}
