/* yuvgrid.h -- what the host side of libasciichat_yuvgrid.so (yuvgrid.c) and its launcher (yuvgrid.hip, the kernel in
 * yuvgrid_kernels.hpp) share.  Not installed. */
#ifndef ASCIICHAT_YUVGRID_PRIV_H
#define ASCIICHAT_YUVGRID_PRIV_H

#include "yuvgrid_math.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the grid of the tile launch over n tiles whose largest has max_pixels pixels: (groups, tile), a lane four pixels */
static inline unsigned yuvgrid_groups(uint32_t max_pixels) {
  const unsigned lanes = (max_pixels + 3u) / 4u;
  return (lanes + YUV_BLOCK - 1u) / YUV_BLOCK;
}

/* The launcher (yuvgrid.hip); returns a hipError_t.  Arguments are the host's to check: nothing is checked again there but what
 * keeps a grid legal.  items: device, n of them; max_pixels: the largest tile_w * tile_h among them */
int yuvgrid_launch_tiles(const yuvgrid_item_t *items, int n, uint32_t max_pixels, uint8_t *tiles, void *stream);

#ifdef __cplusplus
}
#endif
#endif
