/*
 * raster_yuv_kernels.hpp -- the rasteriser's draw straight to YUV 4:2:0 planes (include/asciichat_raster.h: I420 or NV12), for
 * an encoder.  The parse stage is raster_kernels.hpp's and unchanged; this is a second draw over the same cells.  Every pixel
 * is resolved exactly as draw_kernel resolves it (resolve_pixel below), converted by raster_yuv.h, and only the planes are
 * stored: no RGBA reaches memory or LDS.
 *
 *   A lane owns RASTER_YUV_LANE_PX = 4 pixel columns of TWO image rows, i.e. two whole 2x2 blocks: each of its 8 pixels is
 *   resolved once, its Y packed into a dword per row and its channels summed per block in registers, so every chroma sample
 *   comes from four pixels of one lane.  (8 columns would halve the stores; the draw is bound by the per-pixel candidate
 *   tests, and 4 keep the unrolled resolve at 8 pixels and the kernel under 64 VGPRs.)
 *
 *   Image rows pair up from row 0, so a workgroup owns an even number of them: one cell row when cell_h is even, two when it
 *   is odd (H is even, so rows is then even) -- the last image row of the upper cell row pairs with the first of the lower,
 *   and the lower pixels' candidates reach one cell row further: three cell rows of records in LDS, two when cell_h is even.
 *
 *   A tile is RASTER_YUV_TILE_CELLS = 256 cell columns of the workgroup's cell rows -- the records of 256 + 2 cells per row
 *   are what the RGBA draw keeps in LDS too; most grids are one tile.  Its 4-column slots, row pair by row pair, are ONE
 *   sequence that the threads walk with stride: an 800-pixel row is 200 slots, and ten row pairs of it are 2000 slots for 256
 *   threads, not ten times four waves of which the last is an eighth full.  Small batches spread the sequence over the
 *   workgroups of gridDim.y (raster_yuv_split).  Consecutive lanes hold consecutive slots, so a wave stores runs of whole
 *   rows; it may straddle two row pairs.
 *
 *   Stores go by address, one choice per image row.  Y rows begin at even bytes (W is even, images are 4-byte aligned): a
 *   lane's 4 Y of a row are one dword where the row begins on a multiple of 4, else two halfwords.  I420 chroma rows are W / 2
 *   bytes and begin anywhere (the V plane at W H 5/4, byte 15 of a 6x2 image): a lane's two samples are one halfword where
 *   the row begins even, else two bytes.  NV12 pairs begin at even bytes: one dword U V U V, else two halfwords.  The last
 *   slot of a row with W = 2 mod 4 holds one block and takes the narrow form.  With W a multiple of 16 every plane takes its
 *   wide form.  All are non-temporal (store_plane), as draw_kernel's are: written once, never read back here.
 */
#pragma once

#include "raster_kernels.hpp"
#include "raster_yuv.h"

namespace achip {
namespace raster {

static_assert(RASTER_YUV_TILE_CELLS + 2u <= kTileCells, "a tile's cells and their two neighbours fit a row of records");
static_assert(RASTER_YUV_LANE_PX == 4, "two 2x2 blocks per lane: the Y of a row is one dword");

/* the one place that says how plane bytes leave: T at an address aligned to T */
template <typename T> __device__ inline void store_plane(uint8_t *p, T v) {
#if defined(ACHIP_EMULATED) || defined(ACHIP_NO_NT_STORE)
  *reinterpret_cast<T *>(p) = v;
#else
  __builtin_nontemporal_store(v, reinterpret_cast<T *>(p));
#endif
}

/* a tile's cell records in LDS: the cell below a cell is kTileCells words further on */
struct TileCells {
  const uint32_t *box, *fg, *bg, *pitch, *off;
  const uint8_t *atlas; /* the staged coverage when in_lds, else unused */
};

/* One pixel as R | G << 8 | B << 16 | 255 << 24: column lx, row y of the cell whose record is LDS index `own`.  draw_kernel's
 * candidate loop, restated here so that draw_kernel's code stays as it is: last writer first -- down-right, down, down-left,
 * right, own glyph, {LDS index, dx, dy} relative to that cell's origin --, then the own background, with the same blend.  The
 * GPU tests convert the RGBA draw's own output and compare: the two must agree on every pixel. */
__device__ inline uint32_t resolve_pixel(const TileCells &t, const raster_params_t &p, const bool in_lds, const uint32_t own, const uint32_t lx,
                                         const uint32_t y, const uint32_t cw, const uint32_t ch) {
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const uint32_t below = k < 3 ? 1u : 0u;
    const int32_t dc = k == 0 ? 1 : k == 1 ? 0 : k == 2 ? -1 : k == 3 ? 1 : 0;
    const uint32_t at = below * kTileCells + (uint32_t)((int32_t)own + dc);
    const uint32_t box = t.box[at];
    const uint32_t bx = (uint32_t)((int32_t)lx - dc * (int32_t)cw + 32), by = y + 64u - below * ch;
    const uint32_t x0 = box & 255u, y0 = (box >> 8) & 255u, x1 = (box >> 16) & 255u, y1 = box >> 24;
    if (bx >= x0 && bx < x1 && by >= y0 && by < y1) {
      const uint32_t idx = t.off[at] + (by - y0) * t.pitch[at] + (bx - x0);
      const uint32_t a = in_lds ? t.atlas[idx] : p.coverage[idx];
      return blend(t.fg[at], t.bg[at], a);
    }
  }
  return opaque_rgb(t.bg[own]);
}

/* workgroup (x, y): frame x / groups, cell rows [(x % groups) * span, + span) with span = raster_yuv_span; of every tile's
 * slot sequence the slots y * 256 + thread, + gridDim.y * 256, ...  LDS: span + 1 cell rows of records (raster_yuv_lds),
 * then the staged atlas. */
__global__ void __launch_bounds__(RASTER_BLOCK)
    draw_yuv_kernel(const raster_params_t p, const raster_cell_t *__restrict__ cells, uint8_t *__restrict__ yuv, const uint64_t image_pitch,
                    const uint32_t nv12) {
  const uint32_t tid = threadIdx.x;
  const uint32_t rows = (uint32_t)p.rows, cols = (uint32_t)p.cols, cw = (uint32_t)p.cell_w, ch = (uint32_t)p.cell_h;
  const uint32_t span = (ch & 1u) ? 2u : 1u, groups = rows / span, nrec = (span + 1u) * kTileCells;
  const uint32_t f = blockIdx.x / groups, r0 = (blockIdx.x - f * groups) * span, W = cols * cw, H = rows * ch;
  uint32_t *l_box = reinterpret_cast<uint32_t *>(ACHIP_SMEM);
  uint32_t *l_fg = l_box + nrec, *l_bg = l_fg + nrec, *l_pitch = l_bg + nrec, *l_off = l_pitch + nrec;
  uint8_t *l_atlas = ACHIP_SMEM + nrec * 20u; /* (a multiple of 16) */
  const bool in_lds = p.atlas_in_lds != 0u;
  const TileCells t = {l_box, l_fg, l_bg, l_pitch, l_off, l_atlas};
  if (in_lds) { /* (the device copy of the coverage is 16-byte aligned and padded to 16) */
    uint4 *dst = reinterpret_cast<uint4 *>(l_atlas);
    const uint4 *__restrict__ srcv = reinterpret_cast<const uint4 *>(p.coverage);
    for (uint32_t i = tid; i < (p.coverage_bytes + 15u) / 16u; i += kBlock)
      dst[i] = srcv[i];
  }
  const raster_cell_t *__restrict__ frame_cells = cells + (uint64_t)f * rows * cols;
  uint8_t *__restrict__ image = yuv + (uint64_t)f * image_pitch;
  uint8_t *__restrict__ chroma = image + (uint64_t)W * H; /* I420: U, then V a quarter of W H further; NV12: the pairs */
  const uint32_t half_w = W >> 1, quarter = half_w * (H >> 1), pairs = span * ch / 2u, step = gridDim.y * kBlock;
  for (uint32_t c_lo = 0u; c_lo < cols; c_lo += RASTER_YUV_TILE_CELLS) {
    const uint32_t ncol = min(cols - c_lo, (uint32_t)RASTER_YUV_TILE_CELLS), ncell = ncol + 2u; /* LDS index 0 is cell c_lo - 1 */
    /* the tile's pixels [px_lo, px_lo + tile_w): px_lo a multiple of 4, tile_w even as W is */
    const uint32_t px_lo = c_lo * cw, tile_w = ncol * cw, slots = (tile_w + RASTER_YUV_LANE_PX - 1u) / RASTER_YUV_LANE_PX;
    __syncthreads(); /* the tile before has been drawn */
    for (uint32_t i = tid; i < (span + 1u) * ncell; i += kBlock) {
      const uint32_t lr = i / ncell, k = i - lr * ncell;
      const int32_t cc = (int32_t)(c_lo + k) - 1;
      const uint32_t at = lr * kTileCells + k;
      uint32_t box = 0u, fg = 0u, bg = 0u, pitch = 0u, off = 0u;
      if (cc >= 0 && cc < (int32_t)cols && r0 + lr < rows) {
        const raster_cell_t c = frame_cells[(uint64_t)(r0 + lr) * cols + (uint32_t)cc];
        fg = c.fg, bg = c.bg;
        const uint32_t slot = c.slot & 0xFFFFu;
        if (slot != RASTER_NO_GLYPH) {
          const raster_glyph_t g = p.glyphs[slot];
          box = g.box, pitch = g.pitch, off = g.offset;
        }
      }
      l_box[at] = box, l_fg[at] = fg, l_bg[at] = bg, l_pitch[at] = pitch, l_off[at] = off;
    }
    __syncthreads();
    /* slot s of the sequence is slot s % slots of row pair s / slots; from one of a thread's slots to its next both move by
     * the same amounts */
    const uint32_t step_pr = step / slots, step_k = step - step_pr * slots;
    const uint32_t s0 = blockIdx.y * kBlock + tid;
    uint32_t pr = s0 / slots, k = s0 - pr * slots;
    while (pr < pairs) {
      const uint32_t xt = RASTER_YUV_LANE_PX * k, x0 = px_lo + xt; /* the slot's first column, in the tile and in the image */
      const bool two = xt + 4u <= tile_w;                         /* else the row's last block alone (W = 2 mod 4) */
      const uint32_t ct = xt / cw, lx0 = xt - ct * cw;
      const uint32_t row = r0 * ch + 2u * pr; /* the pair's upper image row: even */
      uint32_t ys[2] = {0u, 0u}, sr[2] = {0u, 0u}, sg[2] = {0u, 0u}, sb[2] = {0u, 0u};
#pragma unroll
      for (int dy = 0; dy < 2; dy++) {
        const uint32_t yy = 2u * pr + (uint32_t)dy, lr = yy >= ch ? 1u : 0u, y = yy - lr * ch;
        uint32_t own = lr * kTileCells + ct + 1u, lx = lx0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          if (j >= 2 && !two)
            break;
          const uint32_t v = resolve_pixel(t, p, in_lds, own, lx, y, cw, ch);
          const uint32_t r = v & 255u, g = (v >> 8) & 255u, b = (v >> 16) & 255u;
          ys[dy] |= raster_yuv_y(r, g, b) << (8 * j);
          sr[j >> 1] += r, sg[j >> 1] += g, sb[j >> 1] += b;
          if (++lx == cw) {
            lx = 0u;
            own++;
          }
        }
      }
      uint32_t u[2], v[2];
#pragma unroll
      for (int b = 0; b < 2; b++) {
        const uint32_t ar = raster_yuv_avg(sr[b]), ag = raster_yuv_avg(sg[b]), ab = raster_yuv_avg(sb[b]);
        u[b] = raster_yuv_u(ar, ag, ab), v[b] = raster_yuv_v(ar, ag, ab);
      }
      /* Y: (row + dy) W + x0 into the image, an even byte */
#pragma unroll
      for (int dy = 0; dy < 2; dy++) {
        uint8_t *out = image + (uint64_t)(row + (uint32_t)dy) * W + x0;
        if (two && ((uintptr_t)out & 3u) == 0u) {
          store_plane<uint32_t>(out, ys[dy]);
        } else {
          store_plane<uint16_t>(out, (uint16_t)ys[dy]);
          if (two)
            store_plane<uint16_t>(out + 2, (uint16_t)(ys[dy] >> 16));
        }
      }
      const uint32_t crow = row >> 1;
      if (nv12) {
        uint8_t *out = chroma + (uint64_t)crow * W + x0; /* an even byte */
        const uint32_t w = u[0] | v[0] << 8 | u[1] << 16 | v[1] << 24;
        if (two && ((uintptr_t)out & 3u) == 0u) {
          store_plane<uint32_t>(out, w);
        } else {
          store_plane<uint16_t>(out, (uint16_t)w);
          if (two)
            store_plane<uint16_t>(out + 2, (uint16_t)(w >> 16));
        }
      } else {
#pragma unroll
        for (int pl = 0; pl < 2; pl++) {
          uint8_t *out = chroma + (uint64_t)pl * quarter + (uint64_t)crow * half_w + (x0 >> 1); /* any byte */
          const uint32_t c0 = pl ? v[0] : u[0], c1 = pl ? v[1] : u[1];
          if (two && ((uintptr_t)out & 1u) == 0u) {
            store_plane<uint16_t>(out, (uint16_t)(c0 | c1 << 8));
          } else {
            store_plane<uint8_t>(out, (uint8_t)c0);
            if (two)
              store_plane<uint8_t>(out + 1, (uint8_t)c1);
          }
        }
      }
      pr += step_pr, k += step_k;
      if (k >= slots) {
        k -= slots;
        pr++;
      }
    }
  }
}

} // namespace raster
} // namespace achip
