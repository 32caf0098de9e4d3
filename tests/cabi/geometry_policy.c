/* Enumerates achip_choose_geometry over a grid of launches that straddles every boundary the policy tests, and prints one
 * digest per group (mode, all-ASCII palette, forced geometry, caps set) -- tests/test_geometry_policy.py compares them with
 * tests/golden/geometry_policy.json, so that a change of the policy's code that moves any choice names the group it moved.
 * Plain C, linked against achip_host.c alone.
 *   geometry_policy full   the whole grid
 *   geometry_policy small  small launches of the automatic choice only (run once per ASCIICHAT_HIP_*_PARTS setting: the
 *                          policy reads those once per process)
 *   geometry_policy refuse for every forced id that is no geometry (5..15): the launches of the small grid it was tried on
 *                          (every mode, palette and caps set) and how many of them it was NOT refused for (rc != -1) */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "achip_host.h"

#define MAX_FRAMES 1024

static const int CAPS[2][5] = {{4096, 2048, 1024, 0, 2048}, {4096, 2048, 1024, 256, 2048}};
static const int CUS[] = {1, 3, 63, 64, 85, 127, 128, 129, 255, 256, 304};
/* n_frames / n_cus ratios the policy compares against (num, den) */
static const int RATIOS[][2] = {{3, 4}, {1, 2}, {3, 8}, {5, 16}, {1, 4}, {1, 1}, {3, 2}, {2, 1}, {3, 1}};
static const int SPLITS[] = {-1, 0, 1, 2, 1000};

/* padded row widths around 64 * 2, 200, 220, 256, 448, 512, 2048, 2560, 4096 and the caps */
static const int WIDTHS[] = {1,   64,  80,  119, 120, 121, 127,  128,  129,  159,  160,  161,  199,  200,  201,  219,  220,
                             221, 255, 256, 257, 320, 447, 448,  449,  511,  512,  513,  1000, 1023, 1024, 1025, 2047, 2048,
                             2049, 2559, 2560, 2561, 4095, 4096, 4097};
/* out_h (pixel rows) of the width sweep */
static const int WIDTH_HEIGHTS[] = {2, 24, 90};
/* terminal sizes of the frame-count sweep (80x48 / 80x50 half blocks: eight / nine blocks of geometry 25) */
static const int SIZES[][2] = {{80, 24}, {80, 48}, {80, 50}, {120, 40}, {160, 45}, {160, 48}, {200, 60}, {238, 70},
                               {256, 30}, {320, 90}, {400, 120}, {640, 90}, {1000, 40}, {2000, 20}};
/* cell counts around one, four and sixteen blocks per wave and ACHIP_STREAM_MAXBLK x (128 - ghost) / (64 * cpl - ghost),
 * reached as one-column frames (cells = out_h) and as 64-column ones */
static const int CELLS[] = {127, 128, 129, 508, 512, 516, 2032, 2048, 2064, 8128, 8192, 8256,
                            129024, 131072, 131200, 260096, 262144, 262272};

enum { K_DENSE, K_1080P, K_4K, K_ONE, K_COMP, K_W21845, K_W21846, K_RAGGED, K_COUNT };

static achip_frame_t frames[MAX_FRAMES];
static achip_composite_t comp;

static void set_frame(achip_frame_t *f, int kind, int out_w, int out_h, int pad_left) {
  memset(f, 0, sizeof *f);
  f->out_w = out_w, f->out_h = out_h, f->pad_left = pad_left;
  switch (kind) {
  case K_DENSE: f->src_w = out_w, f->src_h = out_h; break;
  case K_1080P: f->src_w = 1920, f->src_h = 1080; break;
  case K_4K: f->src_w = 3840, f->src_h = 2160; break;
  case K_ONE: f->src_w = 1, f->src_h = 1; break;
  case K_COMP: f->comp = &comp, f->src_w = 2 * out_w, f->src_h = out_h; break;
  case K_W21845: f->src_w = 21845, f->src_h = 4; break;
  case K_W21846: f->src_w = 21846, f->src_h = 4; break;
  }
}

/* n frames of one shape and source kind; K_RAGGED: 80x24 frames from 1080p sources behind a first, dense frame of the shape */
static void fill(int n, int kind, int out_w, int out_h, int pad_left) {
  for (int i = 0; i < n; i++) {
    if (kind != K_RAGGED)
      set_frame(&frames[i], kind, out_w, out_h, pad_left);
    else if (i == 0)
      set_frame(&frames[i], K_DENSE, out_w, out_h, pad_left);
    else
      set_frame(&frames[i], K_1080P, 80, 24, 0);
  }
}

typedef struct {
  uint64_t h;
  long n, seen, accepted; /* launches digested, launches of the grid, launches not refused (rc != -1) */
} digest_t;
/* a forced geometry takes few of the rules: its groups sample every FORCED_STRIDE-th batch of the grid */
#define FORCED_STRIDE 13
static bool skip(digest_t *d, int forced) { return forced >= 0 && d->seen++ % FORCED_STRIDE; }

static void mix(digest_t *d, int v) { /* FNV-1a, 64 bits, over the four results' bytes */
  for (int b = 0; b < 4; b++) {
    d->h ^= (uint8_t)((unsigned)v >> (8 * b));
    d->h *= 0x100000001b3ull;
  }
}

static void run_case(digest_t *d, int mode, bool ascii, const int *caps, int forced, int n, int cus, int split) {
  int variant = -7, parts = -7, rpp = -7;
  const int rc = achip_choose_geometry(mode, frames, n, ascii, caps, cus, split, forced, &variant, &parts, &rpp);
  mix(d, rc);
  mix(d, variant);
  mix(d, parts);
  mix(d, rpp);
  d->n++;
  d->accepted += rc != -1;
}

/* frame counts of a CU count: 1, 2, 9, and one below, at and above every ratio */
static int frame_counts(int cus, int *out) {
  int k = 0;
  const int base[] = {1, 2, 9};
  for (int i = 0; i < 3; i++)
    out[k++] = base[i];
  for (size_t r = 0; r < sizeof RATIOS / sizeof RATIOS[0]; r++) {
    const int at = cus * RATIOS[r][0] / RATIOS[r][1];
    for (int dn = -1; dn <= 1; dn++)
      if (at + dn >= 1 && at + dn <= MAX_FRAMES)
        out[k++] = at + dn;
  }
  return k;
}

#define N_OF(a) ((int)(sizeof(a) / sizeof((a)[0])))

/* every launch of the full grid for one group */
static void full_group(digest_t *d, int mode, bool ascii, const int *caps, int forced) {
  int counts[64];
  /* frame-count sweep: terminal sizes x source kinds x CU counts x frame counts x split requests */
  for (int s = 0; s < N_OF(SIZES); s++)
    for (int kind = 0; kind < K_COUNT; kind++)
      for (int c = 0; c < N_OF(CUS); c++) {
        const int nc = frame_counts(CUS[c], counts);
        for (int i = 0; i < nc; i++) {
          if (skip(d, forced))
            continue;
          fill(counts[i], kind, SIZES[s][0], SIZES[s][1], kind == K_DENSE && s == 0 ? 8 : 0);
          for (int sp = 0; sp < N_OF(SPLITS); sp++)
            run_case(d, mode, ascii, caps, forced, counts[i], CUS[c], SPLITS[sp]);
        }
      }
  /* width sweep: padded widths (with and without pad_left) x heights x source kinds x a few launches */
  static const int launches[][2] = {{1, 256}, {9, 256}, {48, 256}, {96, 256}, {200, 256}, {257, 256}, {600, 256},
                                    {1, 64}, {48, 64}, {64, 64}, {100, 64}, {129, 64}, {200, 128}};
  for (int w = 0; w < N_OF(WIDTHS); w++)
    for (int pad = 0; pad <= 1; pad++)
      for (int h = 0; h < N_OF(WIDTH_HEIGHTS); h++)
        for (int kind = 0; kind < K_COUNT; kind++)
          for (int l = 0; l < N_OF(launches); l++) {
            const int pl = pad && WIDTHS[w] > 3 ? 3 : 0;
            if (skip(d, forced))
              continue;
            fill(launches[l][0], kind, WIDTHS[w] - pl, WIDTH_HEIGHTS[h], pl);
            for (int sp = 0; sp < N_OF(SPLITS); sp++)
              run_case(d, mode, ascii, caps, forced, launches[l][0], launches[l][1], SPLITS[sp]);
          }
  /* cell sweep: frames of given cell counts, one column or 64 columns wide */
  static const int cell_launches[][2] = {{1, 256}, {16, 256}, {96, 256}, {200, 256}, {300, 256}, {513, 256}, {64, 64}, {129, 64}};
  for (int cc = 0; cc < N_OF(CELLS); cc++)
    for (int wide = 0; wide <= 1; wide++)
      for (int kind = 0; kind < K_COUNT; kind++)
        for (int l = 0; l < N_OF(cell_launches); l++) {
          const int w = wide ? 64 : 1;
          for (int dh = 0; dh <= 1; dh++) {
            if (skip(d, forced))
              continue;
            fill(cell_launches[l][0], kind, w, CELLS[cc] / w + dh, 0);
            run_case(d, mode, ascii, caps, forced, cell_launches[l][0], cell_launches[l][1], 0);
          }
        }
}

/* small launches only: what the ASCIICHAT_HIP_*_PARTS switches act on */
static void small_group(digest_t *d, int mode, bool ascii, const int *caps, int forced) {
  static const int sizes[][2] = {{80, 24}, {120, 40}, {128, 30}, {160, 48}, {200, 60}, {256, 30}, {400, 30}, {512, 20}};
  static const int counts[] = {1, 2, 4, 9, 16, 33};
  static const int cus[] = {3, 64, 256};
  for (int s = 0; s < N_OF(sizes); s++)
    for (int kind = 0; kind < K_COUNT; kind++)
      for (int c = 0; c < N_OF(cus); c++)
        for (int i = 0; i < N_OF(counts); i++) {
          if (skip(d, forced))
            continue;
          fill(counts[i], kind, sizes[s][0], sizes[s][1], 0);
          for (int sp = 0; sp <= 2; sp++)
            run_case(d, mode, ascii, caps, forced, counts[i], cus[c], sp);
        }
}

static bool forced_ids(int i, int *id) { /* -1..4, 16..34, 99 */
  static const int ids[] = {-1, 0, 1, 2, 3, 4, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 99};
  if (i >= N_OF(ids))
    return false;
  *id = ids[i];
  return true;
}

int main(int argc, char **argv) {
  const char *cmd = argc > 1 ? argv[1] : "full";
  const bool full = !strcmp(cmd, "full"), small = !strcmp(cmd, "small");
  if (!strcmp(cmd, "refuse")) {
    for (int id = 5; id <= 15; id++) {
      digest_t d = {0xcbf29ce484222325ull, 0, 0, 0};
      for (int mode = 0; mode < ACHIP_MODE_COUNT; mode++)
        for (int ascii = 0; ascii <= 1; ascii++)
          for (int caps = 0; caps < 2; caps++)
            small_group(&d, mode, ascii, CAPS[caps], id);
      printf("%d %ld %ld\n", id, d.n, d.accepted);
    }
    return 0;
  }
  if (!full && !small) {
    fprintf(stderr, "usage: %s full|small|refuse\n", argv[0]);
    return 2;
  }
  for (int mode = 0; mode < ACHIP_MODE_COUNT; mode++)
    for (int ascii = 0; ascii <= 1; ascii++)
      for (int caps = 0; caps < 2; caps++) {
        int forced;
        for (int i = 0; forced_ids(i, &forced); i++) {
          if (small && forced >= 0)
            break;
          digest_t d = {0xcbf29ce484222325ull, 0, 0, 0};
          if (full)
            full_group(&d, mode, ascii, CAPS[caps], forced);
          else
            small_group(&d, mode, ascii, CAPS[caps], forced);
          printf("%d %d %d %d %ld %016llx\n", mode, ascii, forced, caps, d.n, (unsigned long long)d.h);
        }
      }
  return 0;
}
