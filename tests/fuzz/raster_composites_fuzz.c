/*
 * raster_composites_fuzz.c -- sanitizer fuzz of the host-only C behind asciichat_raster_images_set_composites (ascii-chat_amd/
 * csrc/raster_images.h, achip_desc.h): the check of a batch in which a frame may carry a composite, fed with seeded random
 * descriptors in an exact-size heap block and compared with a restatement of the rule and with images_set's own check.  The
 * composite pointers are never dereferenced by the host (they are device addresses): here they point at NOTHING readable (a
 * freed block), so a read through one trips ASan.  A program of its own, built with -fsanitize=address,undefined by
 * tests/test_raster_composites_emulated.py; any report aborts the run.  Host code only.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "raster_images.h"

static uint32_t rng = 88172645u;
static uint32_t rnd(void) {
  rng ^= rng << 13;
  rng ^= rng >> 17;
  rng ^= rng << 5;
  return rng;
}

static int32_t edge(void) {
  static const int32_t v[] = {0, 1, 2, -1, 3840, 10000, INT32_MAX, INT32_MIN, 65536, 1 << 24, (1 << 24) - 1};
  return rnd() % 3 ? (int32_t)(rnd() % 64) + 1 : v[rnd() % (sizeof v / sizeof v[0])];
}

/* the rule of include/asciichat_raster.h for one frame, restated */
static int frame_ok(const achip_frame_t *f) {
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
  if (f->ops & ACHIP_OP_DITHER_MASK)
    return 0;
  return !((f->ops & ACHIP_OP_TINT) && (f->ops & ACHIP_OP_FG_OVERRIDE));
}

int main(int argc, char **argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 5000;
  static const char *palettes[] = {"   ...',;:clodxkO0KXNWM", ".:\xe2\x96\x92\xe2\x96\x88", "#", "", "a\x1b[0m", "a\xe2\x96"};
  static uint8_t pixel[4];
  void *gone = malloc(sizeof(achip_composite_t)); /* an address no host code may read */
  free(gone);
  long taken = 0, refused = 0, with_comp = 0, plain_agree = 0;
  for (int it = 0; it < iters; it++) {
    const int n = (int)(rnd() % 5), max_frames = (int)(rnd() % 6);
    achip_frame_t *frames = n ? malloc((size_t)n * sizeof(*frames)) : NULL;
    int comps = 0, all_ok = 1, first_bad = -1;
    for (int i = 0; i < n; i++) {
      achip_frame_t *f = &frames[i];
      memset(f, 0, sizeof(*f));
      f->src = rnd() % 3 ? pixel : NULL;
      f->comp = rnd() % 3 ? NULL : (const achip_composite_t *)gone;
      const int wild = rnd() % 6 == 0;
      f->src_w = wild ? edge() : 1 + (int32_t)(rnd() % 64), f->src_h = wild ? edge() : 1 + (int32_t)(rnd() % 64);
      f->out_w = wild ? edge() : 1 + (int32_t)(rnd() % 64), f->out_h = wild ? edge() : 1 + (int32_t)(rnd() % 64);
      f->pad_left = rnd() % 8 ? (int32_t)(rnd() % 9) : edge(), f->pad_top = rnd() % 8 ? (int32_t)(rnd() % 5) : edge();
      f->x_ratio = rnd() % 8 ? (uint32_t)((((uint64_t)(uint32_t)f->src_w << 16) / (uint32_t)(f->out_w ? f->out_w : 1)) + 1u) : rnd();
      f->y_ratio = rnd() % 8 ? (uint32_t)((((uint64_t)(uint32_t)f->src_h << 16) / (uint32_t)(f->out_h ? f->out_h : 1)) + 1u) : rnd();
      f->src_stride = rnd() % 4 ? 0 : edge();
      f->ops = rnd() % 4 ? (rnd() % 4) | (rnd() % 3 ? 0u : ACHIP_OP_FG_OVERRIDE) : rnd();
      comps += f->comp != NULL;
      if (all_ok && !frame_ok(f)) {
        all_ok = 0;
        first_bad = i;
      }
    }
    const int mode = rnd() % 8 ? (int)(rnd() % 9) : (int)(rnd() % 14) - 2;
    const char *pal = rnd() % 40 ? palettes[rnd() % 6] : NULL;
    int bad = 12345, got_comps = 12345;
    const char *why = raster_images_composites_check(mode, pal, frames, n, max_frames, &bad, &got_comps);
    if (bad < -1 || bad >= (n > 0 ? n : 1))
      abort();
    const int head_ok = mode >= 0 && mode <= 8 && !raster_images_palette_check(pal) && frames && n >= 1 && n <= max_frames;
    if ((why == NULL) != (head_ok && all_ok)) /* taken exactly when the restated rule takes it */
      abort();
    if (!why) {
      taken++;
      if (bad != -1 || got_comps != comps)
        abort();
      with_comp += comps > 0;
    } else {
      refused++;
      if (got_comps != 0 || (head_ok && bad != first_bad) || (!head_ok && bad != -1))
        abort();
    }
    /* optional outputs may be absent */
    if ((raster_images_composites_check(mode, pal, frames, n, max_frames, NULL, NULL) == NULL) != (why == NULL))
      abort();
    /* a batch without a composite: the two checks agree; with one, images_set's refuses */
    const char *plain = raster_images_check(mode, pal, frames, n, max_frames, NULL);
    if (head_ok && comps == 0) {
      if ((plain == NULL) != (why == NULL))
        abort();
      plain_agree++;
    } else if (head_ok && comps > 0 && !plain) {
      abort();
    }
    free(frames);
  }
  if (!taken || !refused || !with_comp || !plain_agree)
    abort();
  printf("raster composites fuzz ok: %ld sets taken (%ld with composites), %ld refused\n", taken, with_comp, refused);
  return 0;
}
