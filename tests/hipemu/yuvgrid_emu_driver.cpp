/* yuvgrid_emu_driver.cpp -- the kernel of libasciichat_yuvgrid.so (ascii-chat_amd/csrc/yuvgrid_kernels.hpp) under the fiber
 * emulator, from composites and sources as yuvgrid.c takes them -- checked, laid out and rewritten by yuvgrid_math.h's own text
 * -- and launched as yuvgrid.hip launches it; beside it the host fill of yuvgrid_math.h as it stands, and the launcher yuvgrid.c
 * calls when the tests link it against the mock HIP runtime.  TESTS ONLY. */
#include "yuvgrid_kernels.hpp"

#include <vector>

typedef const achip_composite_t *const *comps_t;
typedef const asciichat_yuv_source_t *const *sources_t;

/* the layout of a taken set: the slab's bytes; at[t] (room for max_tiles) the offset of tile t.  -1: the set is refused */
extern "C" int64_t emu_yuvgrid_layout(comps_t comps, sources_t sources, int n_comps, int max_tiles, uint64_t *at) {
  int n_tiles = 0;
  if (yuvgrid_set_check(comps, sources, n_comps, max_tiles, nullptr, nullptr, &n_tiles))
    return -1;
  std::vector<yuvgrid_item_t> items((size_t)n_tiles + 1u);
  const uint64_t bytes = yuvgrid_fill(comps, sources, n_comps, items.data(), nullptr, nullptr);
  for (int t = 0; t < n_tiles && at; t++)
    at[t] = items[(size_t)t].at;
  return (int64_t)bytes;
}

/* create(max_tiles) + set + run(tiles), or with host != 0 the host fill of yuvgrid_math.h in the kernel's place.
 * -1: the set is refused, -2: run refuses its slab */
extern "C" int emu_yuvgrid_run(comps_t comps, sources_t sources, int n_comps, int max_tiles, uint8_t *tiles, int host) {
  int n_tiles = 0;
  if (yuvgrid_set_check(comps, sources, n_comps, max_tiles, nullptr, nullptr, &n_tiles))
    return -1;
  if (n_tiles && (!tiles || ((uintptr_t)tiles & 15u)))
    return -2;
  if (!n_tiles)
    return 0;
  std::vector<yuvgrid_item_t> items((size_t)n_tiles);
  uint32_t max_pixels = 0u;
  (void)yuvgrid_fill(comps, sources, n_comps, items.data(), nullptr, &max_pixels);
  if (host) {
    for (const yuvgrid_item_t &it : items)
      yuvgrid_host_tile(&it, tiles + it.at);
    return 0;
  }
  const yuvgrid_item_t *dev = items.data();
  hipemu::launch(dim3(yuvgrid_groups(max_pixels), (unsigned)n_tiles), dim3(YUV_BLOCK), 0, [&] { achip::yuvgrid::tiles_kernel(dev, tiles); });
  return 0;
}

/* create + set + composites(tiles, out) */
extern "C" int emu_yuvgrid_composites(comps_t comps, sources_t sources, int n_comps, int max_tiles, const uint8_t *tiles, achip_composite_t *out) {
  int n_tiles = 0;
  if (yuvgrid_set_check(comps, sources, n_comps, max_tiles, nullptr, nullptr, &n_tiles))
    return -1;
  if ((n_tiles && (!tiles || ((uintptr_t)tiles & 15u))) || !out)
    return -2;
  std::vector<yuvgrid_item_t> items((size_t)n_tiles + 1u);
  std::vector<uint16_t> masks((size_t)n_comps);
  (void)yuvgrid_fill(comps, sources, n_comps, items.data(), masks.data(), nullptr);
  uint64_t at = 0;
  for (int c = 0; c < n_comps; c++)
    yuvgrid_rewrite(comps[c], masks[(size_t)c], tiles, &at, &out[c]);
  return 0;
}

/* the launcher of yuvgrid.hip on the emulator: what yuvgrid.c calls when the tests link it against the mock HIP runtime
 * (tests/mockhip/mock_hip.c), where device memory is host memory */
extern "C" int yuvgrid_launch_tiles(const yuvgrid_item_t *items, int n, uint32_t max_pixels, uint8_t *tiles, void *) {
  if (!items || n <= 0 || n > YUVGRID_MAX_TILES || max_pixels == 0u || !tiles)
    return 1; /* hipErrorInvalidValue */
  hipemu::launch(dim3(yuvgrid_groups(max_pixels), (unsigned)n), dim3(YUV_BLOCK), 0, [&] { achip::yuvgrid::tiles_kernel(items, tiles); });
  return 0;
}
