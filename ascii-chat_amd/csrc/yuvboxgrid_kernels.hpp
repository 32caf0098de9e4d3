/*
 * yuvboxgrid_kernels.hpp -- the YUV tiles of grid composites box-averaged straight from their planes: the tile of a slot is the
 * box average of the whole conversion of its source to tile_w x tile_h.  The rule is stated in include/asciichat_yuvboxgrid.h;
 * the arithmetic is yuv_math.h's, the box bounds yuvbox.h's, and phase 1 -- the per-column sums of a row's box, four columns a
 * lane, whole-line loads, the 4:2:0 head / pair / tail row walk -- is yuvbox_kernels.hpp's own code, called with a column range.
 *
 * The shape of the work is few, small images from large sources: nine 1080p sources to 26 x 15 tiles are 135 stored rows, each
 * over 72 source rows of 1920 columns.  A workgroup per stored row (yuvbox's shape) would fill half of 256 CUs with 45 KB
 * stages.  So tiles_kernel's workgroup is (tile, stored row, segment of output columns [xa, xb)):
 *   - the workgroup table is in the item block: items[t].first_wg is the prefix sum of the earlier tiles' workgroups, tile_h *
 *     segs each, so tiles of any sizes share a launch without idle workgroups; a workgroup finds its tile by bisection over the
 *     table (at most 12 uniform steps for 4096 tiles: scalar loads) and then its row and segment by one division;
 *   - a box's columns are contiguous (yuvbox_bounds), so the boxes [xa, xb) cover source columns [lo(xa), hi(xb - 1)) and no
 *     other segment's boxes need them summed over this row's box: segments share no output and need no atomics;
 *   - the first source column is rounded down to a multiple of four, so group loads and chroma pairs stay as they are; the extra
 *     columns are summed and never read;
 *   - the LDS stage holds that span (yuvboxgrid_cut bounds it), not 3 * width words;
 *   - a lane owns a group of four columns, so a span of 64 groups would leave three waves of four idle through all of phase 1,
 *     the part that walks the source: the host then cuts the rows of the box into it.slices (2 or 4) slices at even rows, so that
 *     chroma pairs stay whole, and each part of the workgroup (YUV_BLOCK / slices lanes) sums its slice into a stage of its own,
 *     side by side in LDS; a slice without rows stages zeros.  The sums of a column are added up in phase 2: no atomics.
 * Phase 2, after the one barrier, is box_kernel's: 3 * (xb - xa) lanes each add their box's columns at pitch 3, divide and store
 * one byte.  Exactly 3 * tile_w * tile_h bytes of a tile are stored.  No flips: the composite samplers apply none.
 *
 * Row offsets are 64-bit, sums are 32-bit.  No atomics, no inline assembly, no scratch.  Only plain HIP and gfx950_ops.hpp: the
 * same source runs under the CPU emulator (tests/hipemu).
 */
#pragma once

#include <gfx950_ops.hpp>

#include "yuvbox_kernels.hpp"
#include "yuvboxgrid.h"

namespace achip {
namespace yuvboxgrid {

__global__ void __launch_bounds__(YUV_BLOCK)
    tiles_kernel(const yuvboxgrid_item_t *__restrict__ items, const uint32_t n, uint8_t *__restrict__ tiles) {
  const yuvboxgrid_item_t it = items[yuvboxgrid_tile_of(items, n, blockIdx.x)];
  const uint32_t local = blockIdx.x - it.first_wg;
  const uint32_t y = local / it.segs, seg = local - y * it.segs;
  const uint32_t src_w = (uint32_t)it.src.width, src_h = (uint32_t)it.src.height, out_w = (uint32_t)it.tile_w, out_h = (uint32_t)it.tile_h;
  const uint32_t xa = seg * it.seg_out;
  if (y >= out_h || xa >= out_w) /* (never, by the table: kept so that no table can make a workgroup store outside its tile) */
    return;
  const uint32_t xb = xa + it.seg_out < out_w ? xa + it.seg_out : out_w;
  uint32_t y0, y1, c0, c1, unused;
  yuvbox_bounds(src_h, out_h, y, &y0, &y1);
  yuvbox_bounds(src_w, out_w, xa, &c0, &unused);
  yuvbox_bounds(src_w, out_w, xb - 1u, &unused, &c1);
  c0 &= ~3u;
  /* this lane's slice of the rows: cut at even rows between y0 and y1 */
  const uint32_t slices = it.slices, lanes = yuvbox::kBlock / slices, slice = threadIdx.x / lanes, pitch = 3u * it.stage_cols;
  const uint32_t rows = y1 - y0;
  uint32_t ya = slice == 0u ? y0 : (y0 + rows * slice / slices + 1u) & ~1u, yb = slice + 1u == slices ? y1 : (y0 + rows * (slice + 1u) / slices + 1u) & ~1u;
  ya = ya < y1 ? ya : y1, yb = yb < y1 ? yb : y1;
  uint32_t *stage = reinterpret_cast<uint32_t *>(ACHIP_SMEM);
  yuvbox::column_sums(it.src, ya, yb, c0, c1, yuvbox::Lanes{threadIdx.x - slice * lanes, lanes, stage + slice * pitch});
  __syncthreads();
  const uint32_t *sums = stage;
  uint8_t *out = tiles + it.at + (uint64_t)y * (3u * out_w) + 3u * xa;
  for (uint32_t j = threadIdx.x; j < 3u * (xb - xa); j += yuvbox::kBlock) {
    const uint32_t x = j / 3u, c = j - 3u * x;
    uint32_t x0, x1;
    yuvbox_bounds(src_w, out_w, xa + x, &x0, &x1);
    uint32_t s = 0u;
    for (uint32_t r = 0; r < slices; r++)
      for (uint32_t k = x0; k < x1; k++)
        s += sums[r * pitch + 3u * (k - c0) + c];
    const uint32_t n_px = (x1 - x0) * (y1 - y0);
    out[j] = (uint8_t)((s + n_px / 2u) / n_px);
  }
}

} // namespace yuvboxgrid
} // namespace achip
