/*
 * yuvgrid_kernels.hpp -- YUV sources (I420, NV12, YUYV, UYVY) to the RGB24 tiles of grid composites on the device; the rule and
 * the layouts are stated in include/asciichat_yuv.h, the arithmetic and the addressing are yuv_math.h's, the item and the
 * sampling yuvgrid_math.h's.
 *
 * tiles_kernel: only the pixels the composite samplers read.  Grid (groups, tile): the item -- the resolved source, the tile's
 * size, the ratios, where the tile goes -- is uniform per workgroup (scalar loads).  A lane owns four consecutive pixels of the
 * tile's linear order -- they may straddle a tile row: one division per lane, then a carry per pixel --, gathers their Y, U and
 * V, converts, and stores 12 bytes as three dwords (tiles start 16-aligned, 12 * lane keeps that to 4); the last lane of a tile
 * whose pixel count is no multiple of four stores its bytes singly.  Lanes behind the tile leave.  The stores are plain: the
 * render that follows reads the tiles from the L2.  Nothing is read outside a plane's (rows - 1) * stride + row bytes: every
 * sample is clamped into the source.  No LDS, no scratch.
 *
 * Row offsets are 64-bit.  Only plain HIP and gfx950_ops.hpp: the same source runs under the CPU emulator (tests/hipemu).
 */
#pragma once

#include <gfx950_ops.hpp>

#include "yuvgrid.h"

namespace achip {
namespace yuvgrid {

/* pixel (sx, sy) of a layout, converted: R | G << 8 | B << 16 (the planes are global memory: pointers read out of an item are
 * generic) */
__device__ inline uint32_t pixel(const yuv_layout_t &l, int32_t sx, int32_t sy) {
  return yuv_rgb(((const ACHIP_GLOBAL uint8_t *)l.y_plane)[yuv_at_y(&l, sx, sy)], ((const ACHIP_GLOBAL uint8_t *)l.u_plane)[yuv_at_u(&l, sx, sy)],
                 ((const ACHIP_GLOBAL uint8_t *)l.v_plane)[yuv_at_v(&l, sx, sy)]);
}

__global__ void __launch_bounds__(YUV_BLOCK) tiles_kernel(const yuvgrid_item_t *__restrict__ items, uint8_t *__restrict__ tiles) {
  const yuvgrid_item_t it = items[blockIdx.y];
  const uint32_t tile_w = (uint32_t)it.tile_w, total = tile_w * (uint32_t)it.tile_h;
  const uint32_t p0 = 4u * (blockIdx.x * YUV_BLOCK + threadIdx.x);
  if (p0 >= total)
    return;
  const yuv_layout_t l = yuv_layout(&it.src);
  uint32_t y = p0 / tile_w, x = p0 - y * tile_w;
  uint32_t px[4];
#pragma unroll
  for (int k = 0; k < 4; k++) { /* (a pixel behind the tile samples row tile_h: clamped into the source like any other, never stored) */
    int32_t sx, sy;
    yuvgrid_sample_at(&it, x, y, &sx, &sy);
    px[k] = pixel(l, sx, sy);
    if (++x == tile_w)
      x = 0u, y++;
  }
  uint8_t *out = tiles + it.at + 3ull * p0;
  if (p0 + 4u <= total) {
    uint32_t *o = reinterpret_cast<uint32_t *>(out);
    o[0] = px[0] | px[1] << 24;
    o[1] = px[1] >> 8 | px[2] << 16;
    o[2] = px[2] >> 16 | px[3] << 8;
  } else {
    for (uint32_t k = 0; k < total - p0; k++) {
      out[3u * k + 0u] = (uint8_t)px[k];
      out[3u * k + 1u] = (uint8_t)(px[k] >> 8);
      out[3u * k + 2u] = (uint8_t)(px[k] >> 16);
    }
  }
}

} // namespace yuvgrid
} // namespace achip
