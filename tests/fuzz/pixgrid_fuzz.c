/*
 * pixgrid_fuzz.c -- sanitizer fuzz of the host-only C behind libasciichat_pixgrid.so (ascii-chat_amd/csrc/pixgrid.h): the check
 * of a set, fed with seeded random and edge-valued composites and sources and compared with the rule said again; the fill -- the
 * offsets of the tiles, the cut of their rows at a random segment width, the workgroup table and the bisection over it, what
 * the two launches are given --; the rewriting of the descriptors; and, for the sets the check takes, the host walk of every
 * tile in both forms -- each source an exact-size heap block of (height - 1) * stride + bpp * width bytes, the slab a heap block
 * that ends with the last tile's last byte, so that a read or a store outside what the header promises trips ASan -- against
 * the rule written out.  A program of its own, built with -fsanitize=address,undefined by tests/test_pixgrid_emulated.py; any
 * report aborts the run.  Host code only.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pixgrid.h"

static uint32_t rng = 2463534242u;
static uint32_t rnd(void) {
  rng ^= rng << 13;
  rng ^= rng >> 17;
  rng ^= rng << 5;
  return rng;
}

static int32_t edge(void) {
  static const int32_t v[] = {0, 1, 2, -1, 9, 10, 3840, 3841, 2160, 2161, 8191, 8192, 8193, INT32_MAX, INT32_MIN, 65536, 1 << 24};
  return rnd() % 6 ? (int32_t)(rnd() % 24) + 1 : v[rnd() % (sizeof v / sizeof v[0])];
}

#define CHECK(c)                                                                                                                        \
  do {                                                                                                                                  \
    if (!(c)) {                                                                                                                         \
      fprintf(stderr, "pixgrid fuzz: %s fails at line %d (iteration %d)\n", #c, __LINE__, it);                                          \
      return 1;                                                                                                                         \
    }                                                                                                                                   \
  } while (0)

#define MAX_COMPS 3
#define MAX_TILES 27

/* THE RULE of a source (asciichat_pix.h), said again */
static int source_taken(const asciichat_pix_source_t *p) {
  if (p->format < 0 || p->format > 3 || p->width < 1 || p->width > 8192 || p->height < 1 || p->height > 8192)
    return 0;
  const int32_t bpp = (p->format & 1) ? 4 : 3;
  return p->stride >= 0 && p->stride < (1 << 24) && (p->stride == 0 || p->stride >= bpp * p->width) && p->pixels != NULL;
}

/* the rule of a packed slot, said again */
static int slot_taken(const achip_composite_t *c, int k, const asciichat_pix_source_t *p) {
  const achip_comp_src_t *s = &c->s[k];
  if (k >= c->n_src || !s->src || !source_taken(p))
    return 0;
  if (s->src_w != p->width || s->src_h != p->height || s->tile_w < 1 || s->tile_w > 8192 || s->tile_h < 1 || s->tile_h > 8192)
    return 0;
  return (uint64_t)(uint32_t)(s->tile_w - 1) * s->x_ratio < (1ull << 32) && (uint64_t)(uint32_t)(s->tile_h - 1) * s->y_ratio < (1ull << 32);
}

/* the RGB24 value of pixel (x, y), written out */
static void rgb_of(const asciichat_pix_source_t *s, uint32_t x, uint32_t y, uint32_t *rgb) {
  const uint32_t bpp = (s->format & 1) ? 4u : 3u;
  const uint8_t *p = s->pixels + (size_t)y * (size_t)s->stride + (size_t)bpp * x;
  const int blue_first = s->format >= 2;
  rgb[0] = p[blue_first ? 2 : 0], rgb[1] = p[1], rgb[2] = p[blue_first ? 0 : 2];
}

int main(int argc, char **argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 5000;
  static uint8_t one[1];
  static const uint32_t widths[] = {0u, 4u, 8u, 12u, 16u, 24u, 256u, 512u, 1024u};
  long taken = 0, refused = 0, tiles_walked = 0, pixels = 0, segments = 0, unboxable = 0;
  for (int it = 0; it < iters; it++) {
    achip_composite_t comp[MAX_COMPS];
    asciichat_pix_source_t nine[MAX_COMPS][9];
    const achip_composite_t *comps[MAX_COMPS];
    const asciichat_pix_source_t *sources[MAX_COMPS];
    memset(comp, 0, sizeof(comp));
    memset(nine, 0, sizeof(nine));
    const int n_comps = rnd() % 12 ? (int)(rnd() % MAX_COMPS) + 1 : (int)(rnd() % 5) - 1;
    const int max_tiles = rnd() % 6 ? MAX_TILES : (int)(rnd() % 6);
    const uint32_t seg_cols = widths[rnd() % (sizeof widths / sizeof widths[0])];
    const int careless = rnd() % 3 == 0; /* one set in three draws its fields without care for the rule */
    for (int c = 0; c < MAX_COMPS; c++) {
      comps[c] = rnd() % 40 ? &comp[c] : NULL;
      sources[c] = rnd() % 40 ? nine[c] : NULL;
      comp[c].n_src = careless && rnd() % 4 == 0 ? edge() : (int32_t)(rnd() % 10);
      for (int k = 0; k < 9; k++) {
        achip_comp_src_t *s = &comp[c].s[k];
        asciichat_pix_source_t *p = &nine[c][k];
        if (rnd() % 3 == 0)
          continue; /* no packed source: the slot is left as it stands, whatever it holds */
        p->format = careless && rnd() % 12 == 0 ? (int32_t)(rnd() % 7) - 1 : (int32_t)(rnd() % 4);
        p->width = careless && rnd() % 8 == 0 ? edge() : (int32_t)(rnd() % (rnd() % 8 ? 20 : 90)) + 1;
        p->height = careless && rnd() % 8 == 0 ? edge() : (int32_t)(rnd() % 12) + 1;
        if (rnd() % 60 == 0)
          p->width = 3841, p->height = 1; /* beyond the box pass, and small enough to walk */
        p->pixels = one; /* replaced by an exact block below, should the set be taken */
        const int32_t need = p->width > 0 && p->width <= 8192 ? (3 + (p->format & 1)) * p->width : 1;
        p->stride = rnd() % 3 ? 0 : need + (int32_t)(rnd() % 7) - (careless && rnd() % 8 == 0);
        if (careless && rnd() % 30 == 0)
          p->stride = rnd() % 2 ? -p->stride : 1 << 24;
        s->src = careless && rnd() % 10 == 0 ? NULL : one;
        s->src_w = careless && rnd() % 10 == 0 ? edge() : p->width;
        s->src_h = careless && rnd() % 10 == 0 ? edge() : p->height;
        s->tile_w = careless && rnd() % 8 == 0 ? edge() : (int32_t)(rnd() % 30) + 1;
        s->tile_h = careless && rnd() % 8 == 0 ? edge() : (int32_t)(rnd() % 14) + 1;
        /* the reference's ratios, ratios into the clamp, and now and then anything */
        s->x_ratio = careless && rnd() % 8 == 0 ? rnd() : s->tile_w > 0 && p->width > 0 ? (uint32_t)(((uint64_t)(uint32_t)p->width << 16) / (uint32_t)s->tile_w + 1u) << (rnd() % 4 == 0) : 0u;
        s->y_ratio = careless && rnd() % 8 == 0 ? rnd() : s->tile_h > 0 && p->height > 0 ? (uint32_t)(((uint64_t)(uint32_t)p->height << 16) / (uint32_t)s->tile_h + 1u) << (rnd() % 4 == 0) : 0u;
        if (!careless && k >= comp[c].n_src)
          comp[c].n_src = k + 1;
      }
    }
    int bad_comp = 7, bad_slot = 7, n_tiles = 7;
    const char *why = pixgrid_set_check(rnd() % 50 ? comps : NULL, rnd() % 50 ? sources : NULL, n_comps, max_tiles, seg_cols, &bad_comp, &bad_slot, &n_tiles);
    /* the rule, said again (a NULL array is refused whatever else holds: only the call above draws it, so ask once more) */
    int want = n_comps >= 1 && n_comps <= max_tiles, count = 0;
    for (int c = 0; want && c < n_comps; c++) {
      if (!comps[c] || !sources[c] || comp[c].n_src < 0 || comp[c].n_src > 9) {
        want = 0;
        break;
      }
      for (int k = 0; want && k < 9; k++)
        if (nine[c][k].pixels)
          want = slot_taken(&comp[c], k, &nine[c][k]) && ++count <= max_tiles;
    }
    const char *again = pixgrid_set_check(comps, sources, n_comps, max_tiles, seg_cols, &bad_comp, &bad_slot, &n_tiles);
    CHECK((again == NULL) == (want != 0));
    CHECK(!(again && !why)); /* what the full arrays do not pass, nothing passes */
    if (again) {
      CHECK(n_tiles == 0 && (bad_comp == -1 || (bad_comp >= 0 && bad_comp < n_comps)) && bad_slot >= -1 && bad_slot < 9);
      refused++;
      continue;
    }
    CHECK(n_tiles == count && bad_comp == -1 && bad_slot == -1 && count <= MAX_TILES);
    taken++;
    /* every packed source as an exact block; a taken edge value may make a source or a tile too large to walk */
    uint8_t *blocks[MAX_COMPS * 9];
    int n_blocks = 0, walk = 1, boxable = 1;
    for (int c = 0; c < n_comps; c++)
      for (int k = 0; k < 9; k++)
        if (nine[c][k].pixels) {
          if ((int64_t)nine[c][k].width * nine[c][k].height > 4096 || (int64_t)comp[c].s[k].tile_w * comp[c].s[k].tile_h > 4096)
            walk = 0;
          if (nine[c][k].width > 3840 || nine[c][k].height > 2160)
            boxable = 0;
        }
    for (int c = 0; walk && c < n_comps; c++)
      for (int k = 0; k < 9; k++) {
        asciichat_pix_source_t *p = &nine[c][k];
        if (!p->pixels)
          continue;
        const asciichat_pix_source_t r = pix_source_resolved(p);
        const size_t bytes = (size_t)(p->height - 1) * (size_t)r.stride + (size_t)pix_bpp(p->format) * (size_t)p->width;
        uint8_t *b = malloc(bytes);
        for (size_t i = 0; i < bytes; i++)
          b[i] = (uint8_t)rnd();
        p->pixels = blocks[n_blocks++] = b;
      }
    pixgrid_item_t items[MAX_TILES + 1];
    uint16_t masks[MAX_COMPS];
    pixgrid_launches_t l = {7u, 7u, 7u, 7};
    const uint64_t bytes = pixgrid_fill(comps, sources, n_comps, seg_cols, items, masks, &l);
    /* the offsets: each tile behind the one before, 16-aligned, the slab rounded up to 128; the table: a prefix sum */
    uint64_t at = 0, end = 0;
    uint32_t first = 0u, most = 0u, widest = 0u;
    for (int t = 0; t < count; t++) {
      const pixgrid_item_t *i = &items[t];
      CHECK(i->at == at && !(at & 15u) && i->first_wg == first);
      end = at + 3ull * (uint64_t)i->tile_w * (uint64_t)i->tile_h;
      at = (end + 15u) & ~(uint64_t)15u;
      CHECK(i->src.stride >= pix_bpp(i->src.format) * i->src.width); /* resolved */
      most = (uint32_t)(i->tile_w * i->tile_h) > most ? (uint32_t)(i->tile_w * i->tile_h) : most;
      /* the cut: segments of seg_out boxes cover the row; each one's columns, the first rounded down to four and the groups
       * that touch them, fit the stage; within the width unless a segment is one box */
      const uint32_t w = (uint32_t)i->src.width, ow = (uint32_t)i->tile_w;
      CHECK(i->segs >= 1u && i->seg_out >= 1u && (uint64_t)(i->segs - 1u) * i->seg_out < ow && (uint64_t)i->segs * i->seg_out >= ow);
      CHECK(seg_cols != 0u || i->segs == 1u);
      /* the row slices: a lane of a slice a group of its own, all slices within the launch's stage */
      CHECK((i->slices == 1u || i->slices == 2u || i->slices == 4u) && i->stage_cols % 4u == 0u && i->slices * i->stage_cols <= l.stage_cols);
      CHECK(i->slices == 1u || i->stage_cols / 4u * i->slices <= PIX_BLOCK);
      widest = i->slices * i->stage_cols > widest ? i->slices * i->stage_cols : widest;
      for (uint32_t s = 0; s < i->segs; s++) {
        const uint32_t xa = s * i->seg_out, xb = xa + i->seg_out < ow ? xa + i->seg_out : ow;
        const uint32_t c0 = (uint32_t)((uint64_t)xa * w / ow) & ~3u, hi = (uint32_t)((uint64_t)xb * w / ow), lo = (uint32_t)((uint64_t)(xb - 1u) * w / ow);
        const uint32_t c1 = hi > lo + 1u ? hi : lo + 1u;
        CHECK(c0 < c1 && c1 <= w && ((c1 + 3u) & ~3u) - c0 <= i->stage_cols);
        CHECK(seg_cols == 0u || c1 - c0 <= seg_cols || xb - xa == 1u);
        segments++;
      }
      /* the bisection: the first and the last workgroup of the tile, and no other tile's */
      const uint32_t wgs = i->segs * (uint32_t)i->tile_h;
      CHECK(pixgrid_tile_of(items, (uint32_t)count, first) == (uint32_t)t && pixgrid_tile_of(items, (uint32_t)count, first + wgs - 1u) == (uint32_t)t);
      first += wgs;
    }
    CHECK(bytes == ((at + 127u) & ~(uint64_t)127u) && (count > 0) == (bytes > 0));
    CHECK(l.workgroups == first && l.max_pixels == most && l.stage_cols == widest && l.boxable == boxable);
    CHECK(count == 0 || !boxable || (l.stage_cols >= 4u && l.stage_cols <= 3840u));
    unboxable += !boxable;
    /* the walks: the slab ends with the last tile's last byte */
    const size_t slab_bytes = walk && end ? (size_t)end : 1u; /* (not walked: only the rewrite's addresses are taken) */
    uint8_t *slab = malloc(slab_bytes);
    for (int box = 0; box < 2; box++) {
      memset(slab, 0xA5, slab_bytes);
      for (int t = 0; walk && t < count; t++) {
        const pixgrid_item_t *i = &items[t];
        if (box)
          pixgrid_host_box_tile(i, slab + i->at);
        else
          pixgrid_host_tile(i, slab + i->at);
        const uint32_t w = (uint32_t)i->src.width, h = (uint32_t)i->src.height, ow = (uint32_t)i->tile_w, oh = (uint32_t)i->tile_h;
        for (uint32_t y = 0; y < oh; y++)
          for (uint32_t x = 0; x < ow; x++) { /* the rules of the header, written out */
            const uint8_t *o = slab + i->at + 3u * ((size_t)y * ow + x);
            if (!box) {
              uint32_t sx = (uint32_t)(x * i->x_ratio) >> 16, sy = (uint32_t)(y * i->y_ratio) >> 16, rgb[3];
              sx = sx > w - 1u ? w - 1u : sx, sy = sy > h - 1u ? h - 1u : sy;
              rgb_of(&i->src, sx, sy, rgb);
              CHECK(o[0] == rgb[0] && o[1] == rgb[1] && o[2] == rgb[2]);
            } else {
              const uint32_t x0 = x * w / ow, xh = (x + 1u) * w / ow, x1 = xh > x0 + 1u ? xh : x0 + 1u;
              const uint32_t y0 = y * h / oh, yh = (y + 1u) * h / oh, y1 = yh > y0 + 1u ? yh : y0 + 1u;
              uint32_t s[3] = {0u, 0u, 0u}, rgb[3];
              for (uint32_t sy = y0; sy < y1; sy++)
                for (uint32_t sx = x0; sx < x1; sx++) {
                  rgb_of(&i->src, sx, sy, rgb);
                  s[0] += rgb[0], s[1] += rgb[1], s[2] += rgb[2];
                }
              const uint32_t n = (x1 - x0) * (y1 - y0);
              for (int c = 0; c < 3; c++)
                CHECK(o[c] == (uint8_t)((s[c] + n / 2u) / n));
            }
            pixels++;
          }
        for (uint64_t b = i->at + 3ull * (uint64_t)(i->tile_w * i->tile_h); t + 1 < count && b < items[t + 1].at; b++)
          CHECK(slab[b] == 0xA5);
        tiles_walked++;
      }
    }
    /* the rewrite: the packed slots onto their tiles, everything else as it stands */
    at = 0;
    int t = 0;
    for (int c = 0; c < n_comps; c++) {
      achip_composite_t out;
      yuvgrid_rewrite(&comp[c], masks[c], slab, &at, &out);
      achip_composite_t back = out;
      for (int k = 0; k < 9; k++) {
        CHECK(((masks[c] >> k) & 1) == (nine[c][k].pixels != NULL));
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
  if (taken < iters / 20 || refused < iters / 20 || tiles_walked < 1000 || pixels < 10000 || segments < 5000) {
    fprintf(stderr, "pixgrid fuzz: lopsided: %ld taken, %ld refused, %ld tiles, %ld pixels, %ld segments\n", taken, refused, tiles_walked, pixels, segments);
    return 1;
  }
  printf("pixgrid fuzz ok: %ld sets taken, %ld refused, %ld tiles walked, %ld pixels, %ld segments, %ld sets beyond the box pass\n", taken, refused,
         tiles_walked, pixels, segments, unboxable);
  return 0;
}
