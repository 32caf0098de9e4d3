/*
 * yuvgrid_fuzz.c -- sanitizer fuzz of the host-only C behind libasciichat_yuvgrid.so (ascii-chat_amd/csrc/yuvgrid_math.h): the
 * check of a set, fed with seeded random and edge-valued composites and sources and compared with the rule said again; the
 * offsets of the tiles; and, for the sets the check takes, the host fill of every tile -- each plane an exact-size heap block of
 * (rows - 1) * stride + row bytes, the slab a heap block that ends with the last tile's last byte, so that a read or a store
 * outside what the header promises trips ASan -- and the rewriting of the descriptors.  A program of its own, built with
 * -fsanitize=address,undefined by tests/test_yuvgrid_emulated.py; any report aborts the run.  Host code only.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "yuvgrid_math.h"

static uint32_t rng = 2463534242u;
static uint32_t rnd(void) {
  rng ^= rng << 13;
  rng ^= rng >> 17;
  rng ^= rng << 5;
  return rng;
}

static int32_t edge(void) {
  static const int32_t v[] = {0, 1, 2, -1, 9, 10, 8191, 8192, 8193, INT32_MAX, INT32_MIN, 65536, 1 << 24};
  return rnd() % 6 ? (int32_t)(rnd() % 24) + 1 : v[rnd() % (sizeof v / sizeof v[0])];
}

#define CHECK(c)                                                                                                                        \
  do {                                                                                                                                  \
    if (!(c)) {                                                                                                                         \
      fprintf(stderr, "yuvgrid fuzz: %s fails at line %d (iteration %d)\n", #c, __LINE__, it);                                          \
      return 1;                                                                                                                         \
    }                                                                                                                                   \
  } while (0)

#define MAX_COMPS 3

/* the rule of a YUV slot, said again */
static int slot_taken(const achip_composite_t *c, int k, const asciichat_yuv_source_t *y) {
  const achip_comp_src_t *s = &c->s[k];
  if (k >= c->n_src || !s->src || yuv_source_check(y))
    return 0;
  if (s->src_w != y->width || s->src_h != y->height || s->tile_w < 1 || s->tile_w > 8192 || s->tile_h < 1 || s->tile_h > 8192)
    return 0;
  return (uint64_t)(s->tile_w - 1) * s->x_ratio <= 0xFFFFFFFFull && (uint64_t)(s->tile_h - 1) * s->y_ratio <= 0xFFFFFFFFull;
}

int main(int argc, char **argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 5000;
  static uint8_t one[1];
  long taken = 0, refused = 0, tiles_filled = 0, pixels = 0;
  for (int it = 0; it < iters; it++) {
    achip_composite_t comp[MAX_COMPS];
    asciichat_yuv_source_t nine[MAX_COMPS][9];
    const achip_composite_t *comps[MAX_COMPS];
    const asciichat_yuv_source_t *sources[MAX_COMPS];
    memset(comp, 0, sizeof(comp));
    memset(nine, 0, sizeof(nine));
    const int n_comps = rnd() % 12 ? (int)(rnd() % MAX_COMPS) + 1 : (int)(rnd() % 5) - 1;
    const int max_tiles = rnd() % 6 ? 27 : (int)(rnd() % 6);
    const int careless = rnd() % 3 == 0; /* one set in three draws its fields without care for the rule */
    for (int c = 0; c < MAX_COMPS; c++) {
      comps[c] = rnd() % 40 ? &comp[c] : NULL;
      sources[c] = rnd() % 40 ? nine[c] : NULL;
      comp[c].n_src = careless && rnd() % 4 == 0 ? edge() : (int32_t)(rnd() % 10);
      for (int k = 0; k < 9; k++) {
        achip_comp_src_t *s = &comp[c].s[k];
        asciichat_yuv_source_t *y = &nine[c][k];
        if (rnd() % 3 == 0)
          continue; /* no YUV source: the slot is left as it stands, whatever it holds */
        y->format = (int32_t)(rnd() % 4);
        y->width = careless && rnd() % 8 == 0 ? edge() : (int32_t)(rnd() % 20) + 1;
        y->height = careless && rnd() % 8 == 0 ? edge() : (int32_t)(rnd() % 12) + 1;
        if (yuv_is_packed(y->format) && (y->width & 1) && y->width < INT32_MAX && !(careless && rnd() % 8 == 0))
          y->width++;
        for (int p = 0; p < yuv_planes(y->format); p++) {
          y->plane[p] = one; /* replaced by an exact block below, should the set be taken */
          const int32_t need = y->width > 0 && y->width <= YUV_MAX_SIDE ? yuv_plane_row_bytes(y->format, p, y->width) : 1;
          y->stride[p] = rnd() % 3 ? 0 : need + (int32_t)(rnd() % 7) - (careless && rnd() % 8 == 0);
        }
        s->src = careless && rnd() % 10 == 0 ? NULL : one;
        s->src_w = careless && rnd() % 10 == 0 ? edge() : y->width;
        s->src_h = careless && rnd() % 10 == 0 ? edge() : y->height;
        s->tile_w = careless && rnd() % 8 == 0 ? edge() : (int32_t)(rnd() % 30) + 1;
        s->tile_h = careless && rnd() % 8 == 0 ? edge() : (int32_t)(rnd() % 14) + 1;
        s->x_ratio = !careless || rnd() % 8 ? (rnd() % 4 ? 1u : 2u) * (uint32_t)(((uint64_t)(uint32_t)y->width << 16) / (uint64_t)(s->tile_w > 0 ? s->tile_w : 1)) + 1u : rnd(); /* (doubled: into the clamp) */
        s->y_ratio = !careless || rnd() % 8 ? (rnd() % 4 ? 1u : 2u) * (uint32_t)(((uint64_t)(uint32_t)y->height << 16) / (uint64_t)(s->tile_h > 0 ? s->tile_h : 1)) + 1u : rnd();
        if (!careless && k >= comp[c].n_src)
          comp[c].n_src = k + 1;
      }
    }
    int bad_comp = 7, bad_slot = 7, n_tiles = 7;
    const char *why = yuvgrid_set_check(rnd() % 50 ? comps : NULL, rnd() % 50 ? sources : NULL, n_comps, max_tiles, &bad_comp, &bad_slot, &n_tiles);
    /* the rule, said again (a NULL array is refused whatever else holds: only the call above draws it, so ask once more) */
    int want = n_comps >= 1 && n_comps <= max_tiles, count = 0;
    for (int c = 0; want && c < n_comps; c++) {
      if (!comps[c] || !sources[c] || comp[c].n_src < 0 || comp[c].n_src > 9) {
        want = 0;
        break;
      }
      for (int k = 0; want && k < 9; k++)
        if (nine[c][k].plane[0])
          want = slot_taken(&comp[c], k, &nine[c][k]) && ++count <= max_tiles;
    }
    const char *again = yuvgrid_set_check(comps, sources, n_comps, max_tiles, &bad_comp, &bad_slot, &n_tiles);
    CHECK((again == NULL) == (want != 0));
    CHECK(!(again && !why)); /* what the full arrays do not pass, nothing passes */
    if (again) {
      CHECK(n_tiles == 0 && (bad_comp == -1 || (bad_comp >= 0 && bad_comp < n_comps)) && bad_slot >= -1 && bad_slot < 9);
      refused++;
      continue;
    }
    CHECK(n_tiles == count && bad_comp == -1 && bad_slot == -1);
    taken++;
    /* the planes of every YUV source as exact blocks */
    uint8_t *blocks[MAX_COMPS * 9 * 3];
    int n_blocks = 0;
    for (int c = 0; c < n_comps; c++)
      for (int k = 0; k < 9; k++) {
        asciichat_yuv_source_t *y = &nine[c][k];
        if (!y->plane[0])
          continue;
        const asciichat_yuv_source_t r = yuv_source_resolved(y);
        for (int p = 0; p < yuv_planes(y->format); p++) {
          const size_t bytes = (size_t)(yuv_plane_rows(y->format, p, y->height) - 1) * (size_t)r.stride[p] + (size_t)yuv_plane_row_bytes(y->format, p, y->width);
          uint8_t *b = malloc(bytes);
          for (size_t i = 0; i < bytes; i++)
            b[i] = (uint8_t)rnd();
          y->plane[p] = blocks[n_blocks++] = b;
        }
      }
    yuvgrid_item_t items[27];
    uint16_t masks[MAX_COMPS];
    uint32_t max_pixels = 0u;
    CHECK(count <= 27);
    const uint64_t bytes = yuvgrid_fill(comps, sources, n_comps, items, masks, &max_pixels);
    /* the offsets: each tile behind the one before, 16-aligned, the slab rounded up to 128 */
    uint64_t at = 0, end = 0;
    uint32_t most = 0u;
    for (int t = 0; t < count; t++) {
      CHECK(items[t].at == at && !(at & 15u));
      end = at + 3ull * (uint64_t)items[t].tile_w * (uint64_t)items[t].tile_h;
      at = (end + 15u) & ~(uint64_t)15u;
      most = (uint32_t)(items[t].tile_w * items[t].tile_h) > most ? (uint32_t)(items[t].tile_w * items[t].tile_h) : most;
      for (int p = 0; p < 3; p++)
        CHECK((items[t].src.stride[p] != 0) == (p < yuv_planes(items[t].src.format)));
    }
    CHECK(bytes == ((at + 127u) & ~(uint64_t)127u) && bytes % 128u == 0 && (count > 0) == (bytes > 0) && max_pixels == most);
    /* the fill: the slab ends with the last tile's last byte */
    uint8_t *slab = malloc(end ? (size_t)end : 1u);
    memset(slab, 0xA5, end ? (size_t)end : 1u);
    for (int t = 0; t < count; t++) {
      yuvgrid_host_tile(&items[t], slab + items[t].at);
      const yuv_layout_t l = yuv_layout(&items[t].src);
      for (int32_t ly = 0; ly < items[t].tile_h; ly++)
        for (int32_t lx = 0; lx < items[t].tile_w; lx++) { /* the rule of the header, written out */
          uint64_t sx = ((uint64_t)(uint32_t)lx * items[t].x_ratio) >> 16, sy = ((uint64_t)(uint32_t)ly * items[t].y_ratio) >> 16;
          sx = sx > (uint64_t)items[t].src.width - 1u ? (uint64_t)items[t].src.width - 1u : sx;
          sy = sy > (uint64_t)items[t].src.height - 1u ? (uint64_t)items[t].src.height - 1u : sy;
          const uint32_t p = yuv_pixel(&l, (int32_t)sx, (int32_t)sy);
          const uint8_t *o = slab + items[t].at + 3u * ((size_t)ly * (size_t)items[t].tile_w + (size_t)lx);
          CHECK(o[0] == (uint8_t)p && o[1] == (uint8_t)(p >> 8) && o[2] == (uint8_t)(p >> 16));
          pixels++;
        }
      for (uint64_t i = items[t].at + 3ull * (uint64_t)(items[t].tile_w * items[t].tile_h); t + 1 < count && i < items[t + 1].at; i++)
        CHECK(slab[i] == 0xA5);
      tiles_filled++;
    }
    /* the rewrite: the YUV slots onto their tiles, everything else as it stands */
    at = 0;
    int t = 0;
    for (int c = 0; c < n_comps; c++) {
      achip_composite_t out;
      yuvgrid_rewrite(&comp[c], masks[c], slab, &at, &out);
      achip_composite_t back = out;
      for (int k = 0; k < 9; k++) {
        CHECK(((masks[c] >> k) & 1) == (nine[c][k].plane[0] != NULL));
        if (!((masks[c] >> k) & 1))
          continue;
        const achip_comp_src_t *s = &out.s[k];
        CHECK(s->src == slab + items[t].at && s->src_w == s->tile_w && s->src_h == s->tile_h && s->src_stride == 3 * s->tile_w);
        CHECK(s->x_ratio == 65537u && s->y_ratio == 65537u && s->tile_w == items[t].tile_w && s->tile_h == items[t].tile_h);
        back.s[k].src = comp[c].s[k].src, back.s[k].src_w = comp[c].s[k].src_w, back.s[k].src_h = comp[c].s[k].src_h;
        back.s[k].src_stride = comp[c].s[k].src_stride, back.s[k].x_ratio = comp[c].s[k].x_ratio, back.s[k].y_ratio = comp[c].s[k].y_ratio;
        t++;
      }
      CHECK(memcmp(&back, &comp[c], sizeof(back)) == 0);
    }
    CHECK(t == count && at == ((end + 15u) & ~(uint64_t)15u));
    free(slab);
    for (int b = 0; b < n_blocks; b++)
      free(blocks[b]);
  }
  if (taken < iters / 20 || refused < iters / 20 || tiles_filled < 1000 || pixels < 10000) {
    fprintf(stderr, "yuvgrid fuzz: lopsided: %ld taken, %ld refused, %ld tiles, %ld pixels\n", taken, refused, tiles_filled, pixels);
    return 1;
  }
  printf("yuvgrid fuzz ok: %ld sets taken, %ld refused, %ld tiles filled, %ld pixels\n", taken, refused, tiles_filled, pixels);
  return 0;
}
