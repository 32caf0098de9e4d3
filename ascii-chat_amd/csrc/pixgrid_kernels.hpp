/*
 * pixgrid_kernels.hpp -- packed RGB sources (RGB24, RGBA, BGR24, BGRA) to the RGB24 tiles of grid composites on the device, in
 * both tile forms; the rule is stated in include/asciichat_pixgrid.h, the addressing and the permutation are pix_math.h's, the
 * item, the sampling and the workgroup table pixgrid.h's.  A format is a uniform fact of a workgroup in both kernels: its bytes
 * per pixel pick the loads, its channel order is a uniform branch.
 *
 * tiles_kernel: only the pixels the composite samplers read; yuvgrid::tiles_kernel's shape over pix::sample_kernel's fetch.
 * Grid (groups, tile): the item -- the resolved source, the tile's size, the ratios, where the tile goes -- is uniform per
 * workgroup (scalar loads).  A lane owns four consecutive pixels of the tile's linear order -- they may straddle a tile row: one
 * division per lane, then a carry per pixel --, gathers them, permutes, and stores 12 bytes as three dwords (tiles start
 * 16-aligned, 12 * lane keeps that to 4); the last lane of a tile whose pixel count is no multiple of four stores its bytes
 * singly.  A 4-byte format loads one dword per pixel, aligned where base and stride are multiples of 4, else as four unaligned
 * bytes in one access (the last pixel of a source is read to its fourth byte, inside bpp * width); a 3-byte format loads three
 * bytes.  Lanes behind the tile leave.  The stores are plain: the render that follows reads the tiles from the L2.  Every
 * sample is clamped into the source.  No LDS.
 *
 * box_tiles_kernel: the box average of the whole conversion; yuvboxgrid::tiles_kernel's decomposition over pix::column_sums.
 * The shape of the work is few, small images from large sources, so a workgroup is (tile, stored row, segment of output columns
 * [xa, xb)):
 *   - the workgroup table is in the item block: items[t].first_wg is the prefix sum of the earlier tiles' workgroups, tile_h *
 *     segs each; a workgroup finds its tile by bisection over the table (at most 12 uniform steps for 4096 tiles: scalar loads)
 *     and then its row and segment by one division;
 *   - a box's columns are contiguous (pix_bounds), so the boxes [xa, xb) cover source columns [lo(xa), hi(xb - 1)) and segments
 *     share no output: no atomics;
 *   - the first source column is rounded down to a multiple of four, so group loads stay as they are; the extra columns are
 *     summed and never read;
 *   - the LDS stage holds that span (yuvboxgrid_cut bounds it), not 3 * width words: 12 bytes a column, 6 KB at 512 columns,
 *     against the 45 KB of a whole 3840-pixel row, so many workgroups share a CU's 160 KB;
 *   - a lane owns a group of four columns, so a span of 64 groups would leave three waves of four idle through phase 1, the
 *     part that walks the source: the host then cuts the rows of the box into it.slices (2 or 4) slices -- anywhere: there is no
 *     chroma to keep paired --, and each part of the workgroup (PIX_BLOCK / slices lanes) sums its slice into a stage of its
 *     own, side by side in LDS; a slice without rows stages zeros.  The sums of a column are added up in phase 2.
 * Phase 1 stores a group's twelve sums as three 16-byte words at a 48-byte lane pitch; phase 2 reads single words, three
 * neighbouring lanes the three channels of one column, a box further on every third lane.  Phase 2, after the one
 * barrier, is box_kernel's: 3 * (xb - xa) lanes each add their box's columns at pitch 3 over the slices, divide and store one
 * byte.  Exactly 3 * tile_w * tile_h bytes of a tile are stored.  No flips: the composite samplers apply none.
 *
 * Row offsets are 64-bit, sums are 32-bit (pix_kernels.hpp says why that holds at 3840 x 2160).  No atomics, no inline
 * assembly, no scratch, and only vector stores.  Only plain HIP and gfx950_ops.hpp: the same source runs under the CPU emulator
 * (tests/hipemu).
 */
#pragma once

#include <gfx950_ops.hpp>

#include "pix_kernels.hpp"
#include "pixgrid.h"

namespace achip {
namespace pixgrid {

__global__ void __launch_bounds__(PIX_BLOCK) tiles_kernel(const pixgrid_item_t *__restrict__ items, uint8_t *__restrict__ tiles) {
  const pixgrid_item_t it = items[blockIdx.y];
  const uint32_t tile_w = (uint32_t)it.tile_w, total = tile_w * (uint32_t)it.tile_h;
  const uint32_t p0 = 4u * (blockIdx.x * pix::kBlock + threadIdx.x);
  if (p0 >= total)
    return;
  const bool bpp4 = pix_bpp(it.src.format) == 4, swapped = pix_swapped(it.src.format) != 0;
  const bool aligned4 = pix::multiple_of(it.src.pixels, it.src.stride, 4u);
  uint32_t y = p0 / tile_w, x = p0 - y * tile_w;
  uint32_t px[4];
#pragma unroll
  for (int k = 0; k < 4; k++) { /* (a pixel behind the tile samples row tile_h: clamped into the source like any other, never stored) */
    int32_t sx, sy;
    pixgrid_sample_at(&it, x, y, &sx, &sy);
    px[k] = pix::pixel(it.src, bpp4, swapped, aligned4, sx, sy);
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

__global__ void __launch_bounds__(PIX_BLOCK)
    box_tiles_kernel(const pixgrid_item_t *__restrict__ items, const uint32_t n, uint8_t *__restrict__ tiles) {
  const pixgrid_item_t it = items[pixgrid_tile_of(items, n, blockIdx.x)];
  const uint32_t local = blockIdx.x - it.first_wg;
  const uint32_t y = local / it.segs, seg = local - y * it.segs;
  const uint32_t src_w = (uint32_t)it.src.width, src_h = (uint32_t)it.src.height, out_w = (uint32_t)it.tile_w, out_h = (uint32_t)it.tile_h;
  const uint32_t xa = seg * it.seg_out;
  if (y >= out_h || xa >= out_w) /* (never, by the table: kept so that no table can make a workgroup store outside its tile) */
    return;
  const uint32_t xb = xa + it.seg_out < out_w ? xa + it.seg_out : out_w;
  uint32_t y0, y1, c0, c1, unused;
  pix_bounds(src_h, out_h, y, &y0, &y1);
  pix_bounds(src_w, out_w, xa, &c0, &unused);
  pix_bounds(src_w, out_w, xb - 1u, &unused, &c1);
  c0 &= ~3u;
  /* this lane's slice of the rows [y0, y1) */
  const uint32_t slices = it.slices, lanes = pix::kBlock / slices, slice = threadIdx.x / lanes, pitch = 3u * it.stage_cols;
  const uint32_t rows = y1 - y0;
  const uint32_t ya = y0 + rows * slice / slices, yb = y0 + rows * (slice + 1u) / slices;
  uint32_t *stage = reinterpret_cast<uint32_t *>(ACHIP_SMEM);
  const pix::Lanes part{threadIdx.x - slice * lanes, lanes, stage + slice * pitch};
  if (pix_bpp(it.src.format) == 4)
    pix::column_sums<4>(it.src, ya, yb, c0, c1, part);
  else
    pix::column_sums<3>(it.src, ya, yb, c0, c1, part);
  __syncthreads();
  const uint32_t *sums = stage;
  uint8_t *out = tiles + it.at + (uint64_t)y * (3u * out_w) + 3u * xa;
  for (uint32_t j = threadIdx.x; j < 3u * (xb - xa); j += pix::kBlock) {
    const uint32_t x = j / 3u, c = j - 3u * x;
    uint32_t x0, x1;
    pix_bounds(src_w, out_w, xa + x, &x0, &x1);
    uint32_t s = 0u;
    for (uint32_t r = 0; r < slices; r++)
      for (uint32_t k = x0; k < x1; k++)
        s += sums[r * pitch + 3u * (k - c0) + c];
    const uint32_t n_px = (x1 - x0) * (y1 - y0);
    out[j] = (uint8_t)((s + n_px / 2u) / n_px);
  }
}

} // namespace pixgrid
} // namespace achip
