/*
 * yuvbox_fuzz.c -- sanitizer fuzz of the host-only C behind libasciichat_yuvbox.so (ascii-chat_amd/csrc/yuvbox.h): the check of
 * a set, fed with seeded random and edge-valued sources and descriptors and compared with the rule said again, and the host
 * walk of the rule over the sets the check takes -- each plane an exact-size heap block of (rows - 1) * stride + row bytes and
 * the image an exact-size block of 3 * out_w * out_h bytes, so that a read or a store outside what the header promises trips
 * ASan --, its corner pixels summed again from the table of asciichat_yuv.h.  A program of its own, built with
 * -fsanitize=address,undefined by tests/test_yuvbox_emulated.py; any report aborts the run.  Host code only.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "yuvbox.h"

static uint32_t rng = 2463534242u;
static uint32_t rnd(void) {
  rng ^= rng << 13;
  rng ^= rng >> 17;
  rng ^= rng << 5;
  return rng;
}

static int32_t edge(void) {
  static const int32_t v[] = {0, 1, 2, -1, 3, 2160, 2161, 3840, 3841, 3842, 8192, 16384, 16385, INT32_MAX, INT32_MIN, 1 << 24, (1 << 24) - 1};
  return rnd() % 4 ? (int32_t)(rnd() % 40) + 1 : v[rnd() % (sizeof v / sizeof v[0])];
}

#define CHECK(c)                                                                                                                        \
  do {                                                                                                                                  \
    if (!(c)) {                                                                                                                         \
      fprintf(stderr, "yuvbox fuzz: %s fails at line %d (iteration %d)\n", #c, __LINE__, it);                                           \
      return 1;                                                                                                                         \
    }                                                                                                                                   \
  } while (0)

/* the samples of pixel (x, y): the table of asciichat_yuv.h, written out per format */
static uint32_t table_pixel(const asciichat_yuv_source_t *r, uint8_t *const block[3], int32_t x, int32_t y) {
  const int64_t s0 = r->stride[0], s1 = r->stride[1], s2 = r->stride[2];
  uint32_t Y, U, V;
  switch (r->format) {
  case ASCIICHAT_YUV_I420: Y = block[0][y * s0 + x], U = block[1][(y / 2) * s1 + x / 2], V = block[2][(y / 2) * s2 + x / 2]; break;
  case ASCIICHAT_YUV_NV12: Y = block[0][y * s0 + x], U = block[1][(y / 2) * s1 + 2 * (x / 2)], V = block[1][(y / 2) * s1 + 2 * (x / 2) + 1]; break;
  case ASCIICHAT_YUV_UYVY: Y = block[0][y * s0 + 4 * (x / 2) + 1 + 2 * (x & 1)], U = block[0][y * s0 + 4 * (x / 2)], V = block[0][y * s0 + 4 * (x / 2) + 2]; break;
  default: Y = block[0][y * s0 + 4 * (x / 2) + 2 * (x & 1)], U = block[0][y * s0 + 4 * (x / 2) + 1], V = block[0][y * s0 + 4 * (x / 2) + 3]; break;
  }
  return yuv_rgb(Y, U, V);
}

int main(int argc, char **argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 5000;
  static uint8_t one[1];
  long taken = 0, refused = 0, unsupported_seen = 0, walked = 0;
  for (int it = 0; it < iters; it++) {
    asciichat_yuv_source_t s;
    memset(&s, 0, sizeof(s));
    s.format = rnd() % 12 ? (int32_t)(rnd() % 4) : edge();
    s.width = edge();
    s.height = edge();
    if (rnd() % 3 && (s.format == ASCIICHAT_YUV_YUYV || s.format == ASCIICHAT_YUV_UYVY))
      s.width &= ~1;
    const int planes = s.format >= 0 && s.format <= 3 ? yuv_planes(s.format) : 1;
    for (int k = 0; k < 3; k++) {
      const uint32_t r = rnd() % 16;
      if (k < planes ? r != 0 : r == 0)
        s.plane[k] = one; /* replaced by an exact block below, should the set be taken */
      const int32_t need = s.format >= 0 && s.format <= 3 && s.width > 0 && s.width <= YUV_MAX_SIDE ? yuv_plane_row_bytes(s.format, k, s.width) : 1;
      s.stride[k] = r == 1 ? need - 1 : r == 2 ? edge() : r == 3 ? need + (int32_t)(rnd() % 9) : r == 4 ? need : 0;
    }
    achip_frame_t f;
    memset(&f, 0, sizeof(f));
    f.src_w = rnd() % 12 ? s.width : edge();
    f.src_h = rnd() % 12 ? s.height : edge();
    f.out_w = rnd() % 8 ? (int32_t)(rnd() % 24) + 1 : edge();
    f.out_h = rnd() % 8 ? (int32_t)(rnd() % 12) + 1 : edge();
    f.x_ratio = rnd(), f.y_ratio = rnd(); /* never read */
    f.src = rnd() % 2 ? NULL : one;
    f.src_stride = edge();
    f.ops = rnd() % 4u | (rnd() % 5 ? 0u : rnd());
    f.comp = rnd() % 16 ? NULL : (const achip_composite_t *)one;
    const int n = rnd() % 10 ? 1 : (int)(rnd() % 3), max_frames = rnd() % 10 ? 1 : (int)(rnd() % 3);
    const int null_frames = rnd() % 20 == 0, null_sources = rnd() % 20 == 0;
    int bad = 7, unsupported = 7;
    const char *why = yuvbox_set_check(null_sources ? NULL : &s, null_frames ? NULL : &f, n > 1 ? 1 : n, max_frames, &bad, &unsupported);
    /* the rule, said again */
    int src_ok = s.format >= 0 && s.format <= 3 && s.width >= 1 && s.width <= 3840 && s.height >= 1 && s.height <= 2160;
    if (src_ok && (s.format == ASCIICHAT_YUV_YUYV || s.format == ASCIICHAT_YUV_UYVY) && (s.width & 1))
      src_ok = 0;
    for (int k = 0; src_ok && k < 3; k++) {
      if (k >= planes)
        src_ok = s.plane[k] == NULL;
      else
        src_ok = s.plane[k] != NULL && s.stride[k] >= 0 && s.stride[k] < (1 << 24) &&
                 (s.stride[k] == 0 || s.stride[k] >= yuv_plane_row_bytes(s.format, k, s.width));
    }
    const int count_ok = !null_sources && !null_frames && (n > 1 ? 1 : n) >= 1 && (n > 1 ? 1 : n) <= max_frames;
    const int frame_ok = f.src_w == s.width && f.src_h == s.height && f.out_w >= 1 && f.out_w <= 16384 && f.out_h >= 1 && f.out_h <= 16384;
    const int want = count_ok && src_ok && !f.comp && frame_ok;
    CHECK((why == NULL) == (want != 0));
    if (why) {
      refused++;
      CHECK(bad == (count_ok ? 0 : -1));
      CHECK(unsupported == (count_ok && src_ok && f.comp != NULL));
      unsupported_seen += unsupported;
      continue;
    }
    CHECK(bad == -1 && unsupported == 0);
    taken++;
    const yuvbox_item_t it0 = yuvbox_item(&s, f.out_w, f.out_h, f.ops);
    CHECK(it0.flips == (f.ops & 3u) && it0._pad == 0u);
    size_t bytes[3] = {0, 0, 0}, total = 0;
    for (int k = 0; k < planes; k++) {
      CHECK(it0.src.stride[k] >= yuv_plane_row_bytes(s.format, k, s.width));
      bytes[k] = (size_t)(yuv_plane_rows(s.format, k, s.height) - 1) * (size_t)it0.src.stride[k] + (size_t)yuv_plane_row_bytes(s.format, k, s.width);
      total += bytes[k];
    }
    { /* the boxes tile each axis: they start at 0, never leave a gap going down, stay inside, and end at the source's end */
      uint32_t lo, hi, prev_hi = 0;
      for (uint32_t x = 0; x < (uint32_t)f.out_w; x += (uint32_t)f.out_w > 64u ? 97u : 1u) {
        yuvbox_bounds((uint32_t)s.width, (uint32_t)f.out_w, x, &lo, &hi);
        CHECK(lo < hi && hi <= (uint32_t)s.width && (x != 0 || lo == 0) && ((uint32_t)f.out_w > 64u || lo <= prev_hi));
        prev_hi = hi;
      }
      yuvbox_bounds((uint32_t)s.width, (uint32_t)f.out_w, (uint32_t)f.out_w - 1u, &lo, &hi);
      CHECK(hi == (uint32_t)s.width);
      yuvbox_bounds((uint32_t)s.height, (uint32_t)f.out_h, (uint32_t)f.out_h - 1u, &lo, &hi);
      CHECK(hi == (uint32_t)s.height && lo < hi);
    }
    const size_t image_bytes = 3u * (size_t)f.out_w * (size_t)f.out_h;
    if (total > (1u << 18) || image_bytes > (1u << 16))
      continue;
    uint8_t *block[3] = {NULL, NULL, NULL};
    yuvbox_item_t live = it0;
    for (int k = 0; k < planes; k++) {
      block[k] = malloc(bytes[k]);
      for (size_t i = 0; i < bytes[k]; i++)
        block[k][i] = rnd() % 3 ? (uint8_t)rnd() : (uint8_t)(rnd() % 2 ? 255 : 0);
      live.src.plane[k] = block[k];
    }
    uint8_t *image = malloc(image_bytes);
    memset(image, 0x5A, image_bytes);
    yuvbox_host_image(&live, image);
    /* the four corners of the image, summed again */
    for (int corner = 0; corner < 4; corner++) {
      const uint32_t x = corner & 1 ? (uint32_t)f.out_w - 1u : 0u, y = corner & 2 ? (uint32_t)f.out_h - 1u : 0u;
      const uint32_t ax = (f.ops & ACHIP_OP_FLIP_X) ? (uint32_t)f.out_w - 1u - x : x, ay = (f.ops & ACHIP_OP_FLIP_Y) ? (uint32_t)f.out_h - 1u - y : y;
      const uint32_t x0 = ax * (uint32_t)s.width / (uint32_t)f.out_w, y0 = ay * (uint32_t)s.height / (uint32_t)f.out_h;
      uint32_t x1 = (ax + 1u) * (uint32_t)s.width / (uint32_t)f.out_w, y1 = (ay + 1u) * (uint32_t)s.height / (uint32_t)f.out_h;
      x1 = x1 > x0 ? x1 : x0 + 1u, y1 = y1 > y0 ? y1 : y0 + 1u;
      uint32_t sum[3] = {0u, 0u, 0u};
      for (uint32_t sy = y0; sy < y1; sy++)
        for (uint32_t sx = x0; sx < x1; sx++) {
          const uint32_t p = table_pixel(&live.src, block, (int32_t)sx, (int32_t)sy);
          sum[0] += p & 0xFFu, sum[1] += (p >> 8) & 0xFFu, sum[2] += p >> 16;
          walked++;
        }
      const uint32_t cnt = (x1 - x0) * (y1 - y0);
      for (int c = 0; c < 3; c++)
        CHECK(image[3u * ((size_t)y * (uint32_t)f.out_w + x) + (unsigned)c] == (uint8_t)((sum[c] + cnt / 2u) / cnt));
    }
    free(image);
    for (int k = 0; k < planes; k++)
      free(block[k]);
  }
  if (taken < iters / 20 || refused < iters / 20 || unsupported_seen < 1 || walked < 1000) {
    fprintf(stderr, "yuvbox fuzz: lopsided: %ld taken, %ld refused (%ld unsupported), %ld pixels walked\n", taken, refused, unsupported_seen, walked);
    return 1;
  }
  printf("yuvbox fuzz ok: %ld sets taken, %ld refused (%ld unsupported), %ld pixels summed again\n", taken, refused, unsupported_seen, walked);
  return 0;
}
