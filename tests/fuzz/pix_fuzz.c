/*
 * pix_fuzz.c -- sanitizer fuzz of the host-only C behind libasciichat_pix.so (ascii-chat_amd/csrc/pix_math.h, pix.h): the check
 * of a set, fed with seeded random and edge-valued sources and descriptors and compared with the rule said again, and the host
 * walks of the three passes over the sets the check takes -- the source an exact-size heap block of (height - 1) * stride +
 * bpp * width bytes and every image an exact-size block, so that a read or a store outside what the header promises trips ASan
 * --, their corner pixels taken again from the table of asciichat_pix.h.  A program of its own, built with
 * -fsanitize=address,undefined by tests/test_pix_emulated.py; any report aborts the run.  Host code only.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pix.h"

static uint32_t rng = 2463534242u;
static uint32_t rnd(void) {
  rng ^= rng << 13;
  rng ^= rng >> 17;
  rng ^= rng << 5;
  return rng;
}

static int32_t edge(void) {
  static const int32_t v[] = {0, 1, 2, -1, 3, 4, 2160, 2161, 3840, 3841, 8192, 8193, 16384, 16385, INT32_MAX, INT32_MIN, 1 << 24, (1 << 24) - 1};
  return rnd() % 4 ? (int32_t)(rnd() % 40) + 1 : v[rnd() % (sizeof v / sizeof v[0])];
}

#define CHECK(c)                                                                                                                        \
  do {                                                                                                                                  \
    if (!(c)) {                                                                                                                         \
      fprintf(stderr, "pix fuzz: %s fails at line %d (iteration %d)\n", #c, __LINE__, it);                                              \
      return 1;                                                                                                                         \
    }                                                                                                                                   \
  } while (0)

/* the RGB24 value of pixel (x, y): the table of asciichat_pix.h, written out per format */
static void table_pixel(const asciichat_pix_source_t *r, const uint8_t *block, int32_t x, int32_t y, uint8_t rgb[3]) {
  const int64_t s = r->stride;
  switch (r->format) {
  case ASCIICHAT_PIX_RGB: rgb[0] = block[y * s + 3 * x], rgb[1] = block[y * s + 3 * x + 1], rgb[2] = block[y * s + 3 * x + 2]; break;
  case ASCIICHAT_PIX_RGBA: rgb[0] = block[y * s + 4 * x], rgb[1] = block[y * s + 4 * x + 1], rgb[2] = block[y * s + 4 * x + 2]; break;
  case ASCIICHAT_PIX_BGR: rgb[2] = block[y * s + 3 * x], rgb[1] = block[y * s + 3 * x + 1], rgb[0] = block[y * s + 3 * x + 2]; break;
  default: rgb[2] = block[y * s + 4 * x], rgb[1] = block[y * s + 4 * x + 1], rgb[0] = block[y * s + 4 * x + 2]; break;
  }
}

int main(int argc, char **argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 5000;
  static uint8_t one[1];
  long taken = 0, refused = 0, unsupported_seen = 0, walked = 0, boxed = 0;
  for (int it = 0; it < iters; it++) {
    asciichat_pix_source_t s;
    memset(&s, 0, sizeof(s));
    s.format = rnd() % 12 ? (int32_t)(rnd() % 4) : edge();
    s.width = edge();
    s.height = edge();
    s.pixels = rnd() % 16 ? one : NULL; /* replaced by an exact block below, should the set be taken */
    const int fmt_ok = s.format >= 0 && s.format <= 3;
    const int32_t bpp = fmt_ok ? (s.format == ASCIICHAT_PIX_RGBA || s.format == ASCIICHAT_PIX_BGRA ? 4 : 3) : 3;
    const int32_t need = s.width > 0 && s.width <= PIX_MAX_SIDE ? bpp * s.width : 1;
    {
      const uint32_t r = rnd() % 16;
      s.stride = r == 1 ? need - 1 : r == 2 ? edge() : r == 3 ? need + (int32_t)(rnd() % 19) : r == 4 ? need : r == 5 ? -need : 0;
    }
    achip_frame_t f;
    memset(&f, 0, sizeof(f));
    f.src_w = rnd() % 12 ? s.width : edge();
    f.src_h = rnd() % 12 ? s.height : edge();
    f.out_w = rnd() % 8 ? (int32_t)(rnd() % 24) + 1 : edge();
    f.out_h = rnd() % 8 ? (int32_t)(rnd() % 12) + 1 : edge();
    f.x_ratio = rnd() % 6 ? (uint32_t)(((uint64_t)(s.width > 0 ? s.width : 1) << 16) / (uint32_t)(f.out_w > 0 ? f.out_w : 1)) + 1u : rnd();
    f.y_ratio = rnd() % 6 ? (uint32_t)(((uint64_t)(s.height > 0 ? s.height : 1) << 16) / (uint32_t)(f.out_h > 0 ? f.out_h : 1)) + 1u : rnd() >> (rnd() % 16);
    f.src = rnd() % 2 ? NULL : one; /* never read */
    f.src_stride = edge();
    f.ops = rnd() % 4u | (rnd() % 5 ? 0u : rnd());
    f.comp = rnd() % 16 ? NULL : (const achip_composite_t *)one;
    const int n = rnd() % 10 ? 1 : (int)(rnd() % 3), max_frames = rnd() % 10 ? 1 : (int)(rnd() % 3);
    const int null_frames = rnd() % 10 == 0, null_sources = rnd() % 20 == 0;
    int bad = 7, unsupported = 7;
    const int count = n > 1 ? 1 : n;
    const char *why = pix_set_check(null_sources ? NULL : &s, null_frames ? NULL : &f, count, max_frames, &bad, &unsupported);
    /* the rule, said again */
    const int src_ok = fmt_ok && s.width >= 1 && s.width <= 8192 && s.height >= 1 && s.height <= 8192 && s.stride >= 0 && s.stride < (1 << 24) &&
                       (s.stride == 0 || s.stride >= bpp * s.width) && s.pixels != NULL;
    const int count_ok = !null_sources && count >= 1 && count <= max_frames;
    const int frame_ok = null_frames || (f.src_w == s.width && f.src_h == s.height && f.out_w >= 1 && f.out_h >= 1 &&
                                         (uint64_t)f.out_w * (uint64_t)f.out_h <= 0x7FFFFFFFull / 3u &&
                                         (uint64_t)(f.out_w - 1) * f.x_ratio < (1ull << 32) && (uint64_t)(f.out_h - 1) * f.y_ratio < (1ull << 32));
    const int comp = !null_frames && f.comp != NULL;
    const int want = count_ok && src_ok && !comp && frame_ok;
    CHECK((why == NULL) == (want != 0));
    if (why) {
      refused++;
      CHECK(bad == (count_ok ? 0 : -1));
      CHECK(unsupported == (count_ok && src_ok && comp));
      unsupported_seen += unsupported;
      continue;
    }
    CHECK(bad == -1 && unsupported == 0);
    taken++;
    asciichat_pix_source_t live = pix_source_resolved(&s);
    CHECK(live.stride >= bpp * s.width && pix_bpp(s.format) == bpp && (s.stride == 0 ? live.stride == bpp * s.width : live.stride == s.stride));
    const size_t bytes = (size_t)(s.height - 1) * (size_t)live.stride + (size_t)bpp * (size_t)s.width;
    const int boxable = !null_frames && s.width <= 3840 && s.height <= 2160 && f.out_w <= 16384 && f.out_h <= 16384;
    if (!null_frames)
      CHECK(pix_set_boxable(&s, &f, 1) == boxable);
    const size_t image_bytes = null_frames ? 0 : 3u * (size_t)f.out_w * (size_t)f.out_h, whole_bytes = 3u * (size_t)s.width * (size_t)s.height;
    if (bytes > (1u << 18) || image_bytes > (1u << 16) || whole_bytes > (1u << 18))
      continue;
    uint8_t *block = malloc(bytes);
    for (size_t i = 0; i < bytes; i++)
      block[i] = rnd() % 3 ? (uint8_t)rnd() : (uint8_t)(rnd() % 2 ? 255 : 0);
    live.pixels = block;
    uint8_t rgb[3];
    { /* the whole conversion: every pixel again */
      uint8_t *whole = malloc(whole_bytes);
      memset(whole, 0x5A, whole_bytes);
      pix_host_whole(&live, whole, 3u * (size_t)s.width);
      for (int32_t y = 0; y < s.height; y += s.height > 64 ? 61 : 1)
        for (int32_t x = 0; x < s.width; x += s.width > 64 ? 59 : 1) {
          table_pixel(&live, block, x, y, rgb);
          CHECK(memcmp(whole + 3u * ((size_t)y * (size_t)s.width + (size_t)x), rgb, 3) == 0);
          walked++;
        }
      free(whole);
    }
    if (!null_frames) {
      uint8_t *image = malloc(image_bytes);
      memset(image, 0x5A, image_bytes);
      pix_host_sample(&live, &f, image);
      for (int corner = 0; corner < 4; corner++) { /* the sampling rule, said again */
        const uint32_t x = corner & 1 ? (uint32_t)f.out_w - 1u : 0u, y = corner & 2 ? (uint32_t)f.out_h - 1u : 0u;
        uint32_t sx = (uint32_t)(((uint64_t)x * f.x_ratio) >> 16), sy = (uint32_t)(((uint64_t)y * f.y_ratio) >> 16);
        sx = sx > (uint32_t)s.width - 1u ? (uint32_t)s.width - 1u : sx, sy = sy > (uint32_t)s.height - 1u ? (uint32_t)s.height - 1u : sy;
        if (f.ops & ACHIP_OP_FLIP_X)
          sx = (uint32_t)s.width - 1u - sx;
        if (f.ops & ACHIP_OP_FLIP_Y)
          sy = (uint32_t)s.height - 1u - sy;
        table_pixel(&live, block, (int32_t)sx, (int32_t)sy, rgb);
        CHECK(memcmp(image + 3u * ((size_t)y * (uint32_t)f.out_w + x), rgb, 3) == 0);
      }
      if (boxable) {
        boxed++;
        memset(image, 0x5A, image_bytes);
        pix_host_box(&live, f.out_w, f.out_h, f.ops, image);
        for (int corner = 0; corner < 4; corner++) { /* the four corners of the image, summed again */
          const uint32_t x = corner & 1 ? (uint32_t)f.out_w - 1u : 0u, y = corner & 2 ? (uint32_t)f.out_h - 1u : 0u;
          const uint32_t ax = (f.ops & ACHIP_OP_FLIP_X) ? (uint32_t)f.out_w - 1u - x : x, ay = (f.ops & ACHIP_OP_FLIP_Y) ? (uint32_t)f.out_h - 1u - y : y;
          const uint32_t x0 = ax * (uint32_t)s.width / (uint32_t)f.out_w, y0 = ay * (uint32_t)s.height / (uint32_t)f.out_h;
          uint32_t x1 = (ax + 1u) * (uint32_t)s.width / (uint32_t)f.out_w, y1 = (ay + 1u) * (uint32_t)s.height / (uint32_t)f.out_h;
          x1 = x1 > x0 ? x1 : x0 + 1u, y1 = y1 > y0 ? y1 : y0 + 1u;
          uint32_t lo, hi;
          pix_bounds((uint32_t)s.width, (uint32_t)f.out_w, ax, &lo, &hi);
          CHECK(lo == x0 && hi == x1 && hi <= (uint32_t)s.width);
          uint32_t sum[3] = {0u, 0u, 0u};
          for (uint32_t sy = y0; sy < y1; sy++)
            for (uint32_t sx = x0; sx < x1; sx++) {
              table_pixel(&live, block, (int32_t)sx, (int32_t)sy, rgb);
              sum[0] += rgb[0], sum[1] += rgb[1], sum[2] += rgb[2];
              walked++;
            }
          const uint32_t cnt = (x1 - x0) * (y1 - y0);
          for (int c = 0; c < 3; c++)
            CHECK(image[3u * ((size_t)y * (uint32_t)f.out_w + x) + (unsigned)c] == (uint8_t)((sum[c] + cnt / 2u) / cnt));
        }
      }
      free(image);
    }
    free(block);
  }
  if (taken < iters / 20 || refused < iters / 20 || unsupported_seen < 1 || walked < 1000 || boxed < iters / 50) {
    fprintf(stderr, "pix fuzz: lopsided: %ld taken, %ld refused (%ld unsupported), %ld pixels walked, %ld sets boxed\n", taken, refused,
            unsupported_seen, walked, boxed);
    return 1;
  }
  printf("pix fuzz ok: %ld sets taken, %ld refused (%ld unsupported), %ld pixels taken again, %ld sets boxed\n", taken, refused, unsupported_seen,
         walked, boxed);
  return 0;
}
