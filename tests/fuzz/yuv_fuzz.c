/*
 * yuv_fuzz.c -- sanitizer fuzz of the host-only C behind libasciichat_yuv.so (ascii-chat_amd/csrc/yuv_math.h): the checks of a
 * source and of a set, fed with seeded random and edge-valued sources and descriptors, and the addressing, walked over every
 * pixel of the sources the checks take -- each plane an exact-size heap block of (rows - 1) * stride + row bytes, so that a
 * read outside what the header promises trips ASan -- and over every pixel a taken descriptor samples.  A program of its
 * own, built with -fsanitize=address,undefined by tests/test_yuv_emulated.py; any report aborts the run.  Host code only.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "yuv_math.h"

static uint32_t rng = 2463534242u;
static uint32_t rnd(void) {
  rng ^= rng << 13;
  rng ^= rng >> 17;
  rng ^= rng << 5;
  return rng;
}

static int32_t edge(void) {
  static const int32_t v[] = {0, 1, 2, -1, 3, 8191, 8192, 8193, INT32_MAX, INT32_MIN, 65536, 1 << 24, (1 << 24) - 1};
  return rnd() % 4 ? (int32_t)(rnd() % 40) + 1 : v[rnd() % (sizeof v / sizeof v[0])];
}

#define CHECK(c)                                                                                                                        \
  do {                                                                                                                                  \
    if (!(c)) {                                                                                                                         \
      fprintf(stderr, "yuv fuzz: %s fails at line %d (iteration %d)\n", #c, __LINE__, it);                                              \
      return 1;                                                                                                                         \
    }                                                                                                                                   \
  } while (0)

int main(int argc, char **argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 5000;
  static uint8_t one[1];
  long taken = 0, refused = 0, walked = 0, sampled = 0;
  for (int it = 0; it < iters; it++) {
    asciichat_yuv_source_t s;
    memset(&s, 0, sizeof(s));
    s.format = rnd() % 8 ? (int32_t)(rnd() % 4) : edge();
    s.width = edge();
    s.height = edge();
    const int planes = s.format >= 0 && s.format <= 3 ? yuv_planes(s.format) : 1;
    for (int k = 0; k < 3; k++) {
      const uint32_t r = rnd() % 8;
      if (k < planes ? r != 0 : r == 0)
        s.plane[k] = one; /* replaced by an exact block below, should the source be taken */
      const int32_t need = s.format >= 0 && s.format <= 3 && s.width > 0 && s.width <= YUV_MAX_SIDE ? yuv_plane_row_bytes(s.format, k, s.width) : 1;
      s.stride[k] = r == 1 ? need - 1 : r == 2 ? edge() : r == 3 ? need + (int32_t)(rnd() % 9) : r == 4 ? need : 0;
    }
    const char *why = yuv_source_check(&s);
    /* the rule, said again */
    int want = s.format >= 0 && s.format <= 3 && s.width >= 1 && s.width <= 8192 && s.height >= 1 && s.height <= 8192;
    if (want && (s.format == ASCIICHAT_YUV_YUYV || s.format == ASCIICHAT_YUV_UYVY) && (s.width & 1))
      want = 0;
    for (int k = 0; want && k < 3; k++) {
      if (k >= planes)
        want = s.plane[k] == NULL;
      else
        want = s.plane[k] != NULL && s.stride[k] >= 0 && s.stride[k] < (1 << 24) &&
               (s.stride[k] == 0 || s.stride[k] >= yuv_plane_row_bytes(s.format, k, s.width));
    }
    CHECK((why == NULL) == (want != 0));
    if (why) {
      refused++;
      continue;
    }
    taken++;
    const asciichat_yuv_source_t r = yuv_source_resolved(&s);
    size_t bytes[3] = {0, 0, 0}, total = 0;
    for (int k = 0; k < planes; k++) {
      CHECK(r.stride[k] >= yuv_plane_row_bytes(s.format, k, s.width));
      bytes[k] = (size_t)(yuv_plane_rows(s.format, k, s.height) - 1) * (size_t)r.stride[k] + (size_t)yuv_plane_row_bytes(s.format, k, s.width);
      total += bytes[k];
    }
    asciichat_yuv_source_t live = r;
    yuv_layout_t l = yuv_layout(&live);
    { /* the far corner lies inside its planes, whatever the size */
      const int32_t x = s.width - 1, y = s.height - 1;
      const int up = yuv_is_packed(s.format) ? 0 : 1, vp = s.format == ASCIICHAT_YUV_I420 ? 2 : up;
      CHECK(yuv_at_y(&l, x, y) >= 0 && (size_t)yuv_at_y(&l, x, y) < bytes[0]);
      CHECK(yuv_at_u(&l, x, y) >= 0 && (size_t)yuv_at_u(&l, x, y) < bytes[up]);
      CHECK(yuv_at_v(&l, x, y) >= 0 && (size_t)yuv_at_v(&l, x, y) < bytes[vp]);
      CHECK(yuv_at_y(&l, 0, 0) >= 0 && yuv_at_u(&l, 0, 0) >= 0 && yuv_at_v(&l, 0, 0) >= 0);
    }
    if (total > (1u << 20))
      continue;
    uint8_t *block[3] = {NULL, NULL, NULL};
    for (int k = 0; k < planes; k++) {
      block[k] = malloc(bytes[k]);
      for (size_t i = 0; i < bytes[k]; i++)
        block[k][i] = (uint8_t)rnd();
      live.plane[k] = block[k];
    }
    l = yuv_layout(&live);
    for (int32_t y = 0; y < s.height; y++)
      for (int32_t x = 0; x < s.width; x++) {
        const uint32_t p = yuv_pixel(&l, x, y);
        /* the table of asciichat_yuv.h, written out per format */
        uint32_t Y, U, V;
        const int64_t s0 = r.stride[0], s1 = r.stride[1], s2 = r.stride[2];
        switch (s.format) {
        case ASCIICHAT_YUV_I420: Y = block[0][y * s0 + x], U = block[1][(y / 2) * s1 + x / 2], V = block[2][(y / 2) * s2 + x / 2]; break;
        case ASCIICHAT_YUV_NV12: Y = block[0][y * s0 + x], U = block[1][(y / 2) * s1 + 2 * (x / 2)], V = block[1][(y / 2) * s1 + 2 * (x / 2) + 1]; break;
        case ASCIICHAT_YUV_UYVY: Y = block[0][y * s0 + 4 * (x / 2) + 1 + 2 * (x & 1)], U = block[0][y * s0 + 4 * (x / 2)], V = block[0][y * s0 + 4 * (x / 2) + 2]; break;
        default: Y = block[0][y * s0 + 4 * (x / 2) + 2 * (x & 1)], U = block[0][y * s0 + 4 * (x / 2) + 1], V = block[0][y * s0 + 4 * (x / 2) + 3]; break;
        }
        CHECK(p == yuv_rgb(Y, U, V) && (p >> 24) == 0u);
        walked++;
      }
    /* a descriptor over it: taken or refused by the rule, and what it samples lies inside the source */
    achip_frame_t f;
    memset(&f, 0, sizeof(f));
    f.src_w = rnd() % 8 ? s.width : edge();
    f.src_h = rnd() % 8 ? s.height : edge();
    f.out_w = rnd() % 8 ? (int32_t)(rnd() % 50) + 1 : edge();
    f.out_h = rnd() % 8 ? (int32_t)(rnd() % 20) + 1 : edge();
    f.x_ratio = rnd() % 6 ? (uint32_t)(((uint64_t)s.width << 16) / (uint64_t)(f.out_w > 0 ? f.out_w : 1)) + 1u : rnd();
    f.y_ratio = rnd() % 6 ? (uint32_t)(((uint64_t)s.height << 16) / (uint64_t)(f.out_h > 0 ? f.out_h : 1)) + 1u : rnd();
    f.ops = rnd() % 4u | (rnd() % 5 ? 0u : rnd());
    f.comp = rnd() % 16 ? NULL : (const achip_composite_t *)one;
    f.src_stride = edge();
    int bad = 7, unsupported = 7;
    const int max_frames = (int)(rnd() % 3);
    const char *refusal = yuv_frames_check(&live, rnd() % 8 ? &f : NULL, 1, max_frames, &bad, &unsupported);
    if (refusal) {
      CHECK(bad == -1 || bad == 0);
      CHECK(unsupported == (f.comp != NULL && max_frames >= 1 && bad == 0 && strstr(refusal, "composite") != NULL));
    } else if (bad == -1 && unsupported == 0 && f.out_w > 0 && f.out_h > 0 && (uint64_t)f.out_w * (uint64_t)f.out_h <= 4096u &&
               f.src_w == s.width && f.src_h == s.height) {
      for (int32_t y = 0; y < f.out_h; y++)
        for (int32_t x = 0; x < f.out_w; x++) {
          int32_t sx = -1, sy = -1;
          yuv_sample_at(&f, x, y, &sx, &sy);
          CHECK(sx >= 0 && sx < s.width && sy >= 0 && sy < s.height);
          (void)yuv_pixel(&l, sx, sy);
          sampled++;
        }
    } else {
      CHECK(bad == -1 && unsupported == 0);
    }
    for (int k = 0; k < planes; k++)
      free(block[k]);
  }
  if (taken < iters / 20 || refused < iters / 20 || walked < 1000 || sampled < 1000) {
    fprintf(stderr, "yuv fuzz: lopsided: %ld taken, %ld refused, %ld pixels walked, %ld sampled\n", taken, refused, walked, sampled);
    return 1;
  }
  printf("yuv fuzz ok: %ld sources taken, %ld refused, %ld pixels walked, %ld sampled\n", taken, refused, walked, sampled);
  return 0;
}
