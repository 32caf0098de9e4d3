/* pixgrid_emu_driver.cpp -- the two kernels of libasciichat_pixgrid.so (ascii-chat_amd/csrc/pixgrid_kernels.hpp) under the fiber
 * emulator, from composites and sources as pixgrid.c takes them -- checked, cut and laid out by pixgrid.h's own text at the
 * segment width this driver is built with (-DPIXGRID_SEG_COLS=N; the shipped one without) -- and launched as pixgrid.hip
 * launches them; beside them the checks and the host walks of the rule as they stand, and the launchers pixgrid.c calls when
 * the tests link it against the mock HIP runtime.  TESTS ONLY. */
#include "pixgrid_kernels.hpp"

#include <vector>

typedef const achip_composite_t *const *comps_t;
typedef const asciichat_pix_source_t *const *sources_t;

static long g_launches = 0;

/* ---- the launchers of pixgrid.hip on the emulator: also what pixgrid.c calls when the tests link it against the mock HIP
 * runtime (tests/mockhip/mock_hip.c), where device memory is host memory ---- */
extern "C" int pixgrid_launch_tiles(const pixgrid_item_t *items, int n, uint32_t max_pixels, uint8_t *tiles, void *) {
  if (!items || n <= 0 || n > PIXGRID_MAX_TILES || max_pixels == 0u || !tiles)
    return 1; /* hipErrorInvalidValue */
  const unsigned lanes = (max_pixels + 3u) / 4u, groups = (lanes + PIX_BLOCK - 1u) / PIX_BLOCK;
  g_launches++;
  hipemu::launch(dim3(groups, (unsigned)n), dim3(PIX_BLOCK), 0, [&] { achip::pixgrid::tiles_kernel(items, tiles); });
  return 0;
}

extern "C" int pixgrid_launch_box(const pixgrid_item_t *items, int n, uint32_t workgroups, uint32_t stage_cols, uint8_t *tiles, void *) {
  if (!items || n <= 0 || n > PIXGRID_MAX_TILES || workgroups == 0u || workgroups > PIXGRID_MAX_WORKGROUPS || stage_cols == 0u ||
      stage_cols > PIX_BOX_MAX_SRC_W || !tiles)
    return 1;
  g_launches++;
  hipemu::launch(dim3(workgroups), dim3(PIX_BLOCK), pixgrid_lds_bytes(stage_cols), [&] { achip::pixgrid::box_tiles_kernel(items, (uint32_t)n, tiles); });
  return 0;
}

/* the launches made through the two launchers above, by whoever called them */
extern "C" long emu_pixgrid_launches(void) { return g_launches; }

/* the segment width this driver was built with */
extern "C" uint32_t emu_pixgrid_seg_cols(void) { return PIXGRID_SEG_COLS; }

/* what the host decides about a set: 0 taken, 1 refused (why receives the reason) */
extern "C" int emu_pixgrid_set_check(comps_t comps, sources_t sources, int n_comps, int max_tiles, int *bad_comp, int *bad_slot, int *n_tiles,
                                     const char **why) {
  const char *w = pixgrid_set_check(comps, sources, n_comps, max_tiles, PIXGRID_SEG_COLS, bad_comp, bad_slot, n_tiles);
  if (why)
    *why = w;
  return w ? 1 : 0;
}

/* the layout of a taken set: the slab's bytes; per tile t (room for max_tiles each) its offset, its first workgroup, its
 * segments, their output columns, the columns of its stage and its row slices; launch[4]: max_pixels, workgroups, stage_cols,
 * boxable.  -1: the set is refused */
extern "C" int64_t emu_pixgrid_layout(comps_t comps, sources_t sources, int n_comps, int max_tiles, uint64_t *at, uint32_t *first_wg, uint32_t *segs,
                                      uint32_t *seg_out, uint32_t *cols, uint32_t *slices, uint32_t *launch) {
  int n_tiles = 0;
  if (pixgrid_set_check(comps, sources, n_comps, max_tiles, PIXGRID_SEG_COLS, nullptr, nullptr, &n_tiles))
    return -1;
  std::vector<pixgrid_item_t> items((size_t)n_tiles + 1u);
  pixgrid_launches_t l;
  const uint64_t bytes = pixgrid_fill(comps, sources, n_comps, PIXGRID_SEG_COLS, items.data(), nullptr, &l);
  for (int t = 0; t < n_tiles; t++) {
    const pixgrid_item_t &it = items[(size_t)t];
    at[t] = it.at, first_wg[t] = it.first_wg, segs[t] = it.segs, seg_out[t] = it.seg_out, cols[t] = it.stage_cols, slices[t] = it.slices;
  }
  launch[0] = l.max_pixels, launch[1] = l.workgroups, launch[2] = l.stage_cols, launch[3] = (uint32_t)l.boxable;
  return (int64_t)bytes;
}

/* create(max_tiles) + set + run(tiles) (box == 0) or run_box(tiles) (box != 0), or with host != 0 the host walk of pixgrid.h in
 * the kernel's place.  -1: the set is refused, -2: the slab is refused, -3: the launcher refuses, -4: run_box does not support
 * the set */
extern "C" int emu_pixgrid_run(comps_t comps, sources_t sources, int n_comps, int max_tiles, uint8_t *tiles, int box, int host) {
  int n_tiles = 0;
  if (pixgrid_set_check(comps, sources, n_comps, max_tiles, PIXGRID_SEG_COLS, nullptr, nullptr, &n_tiles))
    return -1;
  if (n_tiles && (!tiles || ((uintptr_t)tiles & 15u)))
    return -2;
  if (!n_tiles)
    return 0;
  std::vector<pixgrid_item_t> items((size_t)n_tiles);
  pixgrid_launches_t l;
  (void)pixgrid_fill(comps, sources, n_comps, PIXGRID_SEG_COLS, items.data(), nullptr, &l);
  if (box && !l.boxable)
    return -4;
  if (host) {
    for (const pixgrid_item_t &it : items) {
      if (box)
        pixgrid_host_box_tile(&it, tiles + it.at);
      else
        pixgrid_host_tile(&it, tiles + it.at);
    }
    return 0;
  }
  if (box)
    return pixgrid_launch_box(items.data(), n_tiles, l.workgroups, l.stage_cols, tiles, nullptr) ? -3 : 0;
  return pixgrid_launch_tiles(items.data(), n_tiles, l.max_pixels, tiles, nullptr) ? -3 : 0;
}

/* create + set + composites(tiles, out) */
extern "C" int emu_pixgrid_composites(comps_t comps, sources_t sources, int n_comps, int max_tiles, const uint8_t *tiles, achip_composite_t *out) {
  int n_tiles = 0;
  if (pixgrid_set_check(comps, sources, n_comps, max_tiles, PIXGRID_SEG_COLS, nullptr, nullptr, &n_tiles))
    return -1;
  if ((n_tiles && (!tiles || ((uintptr_t)tiles & 15u))) || !out)
    return -2;
  std::vector<pixgrid_item_t> items((size_t)n_tiles + 1u);
  std::vector<uint16_t> masks((size_t)n_comps);
  (void)pixgrid_fill(comps, sources, n_comps, PIXGRID_SEG_COLS, items.data(), masks.data(), nullptr);
  uint64_t at = 0;
  for (int c = 0; c < n_comps; c++)
    yuvgrid_rewrite(comps[c], masks[(size_t)c], tiles, &at, &out[c]);
  return 0;
}
