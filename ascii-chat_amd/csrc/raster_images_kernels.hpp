/*
 * raster_images_kernels.hpp -- the rasteriser's cell grids straight from frame descriptors (asciichat_raster_images_set and the
 * entries behind it, include/asciichat_raster.h): what the parse of raster_kernels.hpp recovers from the text a plan renders
 * for a descriptor -- a glyph, a foreground and a background per cell -- is a function of the sampled pixels, so this stage
 * samples and writes the cells, and the text is never written.  The draw kernels take the cells from there.
 *
 * One launch: workgroup (x, y) owns cells [256 x, 256 x + 256) of frame y's cols x rows grid in row-major order, one lane per
 * cell; the frame index is uniform per workgroup, so its descriptor arrives by scalar loads; a wave stores 768 contiguous
 * bytes.  A cell costs one sample (two in the half-block modes), its look-ups (the luminance -> slot table and the indexed
 * colours, 3 KB in all, read through the caches) and one 12-byte store.  The sampler, the tints and the quantisers are the
 * render kernels' own (render_kernels.hpp), unchanged.
 *
 * The rule, per mode, is the renderers' (render_kernels.hpp build_token and the reference lines it cites) read through the
 * parser's grammar.  Every cell outside the frame's text -- rows above pad_top, rows behind the text, columns behind pad_left + out_w --
 * is blank; a pad cell and a transparent half-block cell are spaces, which draw nothing, under the pen that is current there.
 * Three places need more than the cell's own sample:
 *   TRUE_FG pads        no reset ends a row, so the pad cells of text row y > 0 carry the pen row y - 1 ended with.
 *   TRUE_FG mixed       with one-byte AND multi-byte glyphs in a palette the reference keeps its last colour for one-byte
 *                       glyphs only, while a multi-byte glyph always sets the pen: a one-byte cell whose colour equals that
 *                       of the one-byte cell before it emits nothing and shows the pen a multi-byte cell in between left.
 *                       The lane walks back through the text until it knows (a step or two on natural images, as far as an
 *                       evenly coloured stretch reaches on flat ones; `mixed` is 0 for every other palette).
 *   HB_256 / HB_16      runs are cells of equal quantised pairs, and the run's FIRST cell decides by its raw bytes whether the
 *                       run is transparent.  Only a cell quantised like black on both halves can belong to such a run; it
 *                       walks left to its run's first cell.
 *
 * Grid composites (images_set_composites): COMP = true is the kernel of a set in which some frame carries comp; COMP = false is
 * the kernel of every other set, with no barrier and no LDS, as before.  A workgroup whose frame is a composite copies the
 * 464-byte descriptor and the reciprocals of the two cell sizes into LDS (comp_stage, ACHIP_COMP_LDS_BYTES at offset 0), passes
 * ONE barrier -- every lane of the workgroup, the idle ones behind the grid's last cell too, which is why those lanes are masked
 * and not returned early --, reads the descriptor's uniform head once (comp_head) and samples through sample_frame_raw<true, 0>
 * and sample_finish<true>, the three walks above included; a plain frame of such a set takes the plain sampler.  The staged
 * sampler and not the global one (sample_composite), although tests/test_composite_boundaries.py holds the two equal: the walks
 * are chains of dependent samples, and the global sampler makes each of them two divisions and three dependent global loads
 * (cell size -> tile record -> pixel) where the staged one has a multiply-high, LDS reads and one global request; and it is the
 * sampler the renderers of these frames use (stream, rows and phase kernels), so text path and this stage read a descriptor the
 * same way -- its _pad word for every sample outside the tiles included.  Flips and tints do not apply to a composite frame
 * (sample_frame_raw, sample_finish); FG_OVERRIDE does, as the token builder applies it.
 * Only plain HIP and gfx950_ops.hpp: the same source runs under the CPU emulator (tests/hipemu).
 */
#pragma once

#include "raster_images.h"
#include "render_kernels.hpp"

namespace achip {
namespace raster {

/* a sample (0x00BBGGRR) as a cell colour (0x00RRGGBB) */
__device__ inline uint32_t cell_rgb(uint32_t p) { return (p & 0xFFu) << 16 | (p & 0xFF00u) | ((p >> 16) & 0xFFu); }

/* Sample (x, y) of the frame.  COMP: the launch may hold composite frames, whose descriptor the workgroup staged at LDS offset 0
 * (`head`: its wave-uniform fields, comp_head); a plain frame in such a launch takes the plain sampler, as in the renderers. */
template <bool COMP> __device__ inline uint32_t image_sample(const achip_frame_t &f, const CompHead *head, uint32_t x, uint32_t y) {
  if (!COMP)
    return px_rgb(sample_frame<false>(f, x, y));
  uint32_t kind;
  const uint32_t v = sample_frame_raw<true, 0>(f, x, y, kind, head);
  return px_rgb(sample_finish<true>(f, v, kind));
}

/* TRUE_FG: the pen (as a sample) behind cell (x, y) of the frame's text -- the colour the cell itself shows */
template <bool COMP>
__device__ inline uint32_t truecolor_pen(const achip_frame_t &f, const CompHead *head, const uint32_t *__restrict__ slot, bool mixed,
                                         uint32_t x, uint32_t y) {
  const uint32_t p = image_sample<COMP>(f, head, x, y);
  if (!mixed || !(slot[luma601(p)] & RASTER_IMG_ASCII))
    return p; /* every cell sets the pen it needs, or a multi-byte glyph: always its own colour */
  /* a one-byte cell of colour p sets the pen when the one-byte cell before it, multi-byte cells skipped, has another colour
   * (or there is none); else it shows the pen behind the cell right in front of it -- a multi-byte cell's own colour, or
   * whatever that equal one-byte cell shows in its turn */
  const auto back = [&]() -> bool { /* to the cell in front, in the text's order; false at the frame's first cell */
    if (x) {
      x--;
    } else if (y) {
      y--;
      x = (uint32_t)f.out_w - 1u;
    } else {
      return false;
    }
    return true;
  };
  for (;;) {
    if (!back())
      return p;
    uint32_t q = image_sample<COMP>(f, head, x, y);
    if (slot[luma601(q)] & RASTER_IMG_ASCII) {
      if (q != p)
        return p;
      continue; /* an equal one-byte cell right in front: what it shows */
    }
    const uint32_t wide = q; /* a multi-byte cell right in front: its colour is the pen unless this cell sets its own */
    do {
      if (!back())
        return p;
      q = image_sample<COMP>(f, head, x, y);
    } while (!(slot[luma601(q)] & RASTER_IMG_ASCII));
    return q != p ? p : wide;
  }
}

template <int MODE> __device__ inline uint32_t indexed_key(uint32_t p) { return MODE == ACHIP_MODE_HB_256 || MODE == ACHIP_MODE_256_FG ? quant256(p) : quant16(p); }

template <int MODE, bool COMP = false>
__global__ void __launch_bounds__(RASTER_BLOCK)
    cells_images_kernel(const raster_params_t p, const raster_img_args_t a, raster_cell_t *__restrict__ cells, uint32_t *__restrict__ status) {
  constexpr bool HB = mode_is_halfblock(MODE);
  const uint32_t fi = blockIdx.y, tid = threadIdx.x;
  const uint32_t cols = (uint32_t)p.cols, rows = (uint32_t)p.rows;
  achip_frame_t f = a.frames[fi];
  if (f.src_stride == 0) /* tightly packed, as the render kernels read it */
    f.src_stride = 3 * f.src_w;
  const uint32_t *__restrict__ slot = a.tables->slot;
  const uint32_t *__restrict__ fixed = a.tables->fixed;
  const int32_t T = HB ? f.out_h - (f.out_h >> 1) : f.out_h; /* text rows */
  if (blockIdx.x == 0u && tid == 0u) { /* what the parser would report: a character beyond the grid's columns in a row of the
                                          grid, a character behind its rows */
    uint32_t st = 0u;
    if ((long long)f.pad_left + f.out_w > (long long)cols && f.pad_top < (int32_t)rows)
      st |= ASCIICHAT_RASTER_OVERFLOW_COLS;
    if ((long long)f.pad_top + T > (long long)rows)
      st |= ASCIICHAT_RASTER_OVERFLOW_ROWS;
    status[fi] = st;
  }
  const uint32_t c = blockIdx.x * RASTER_IMG_CELLS + tid;
  const bool live = c < rows * cols; /* the last workgroup of a grid: lanes behind its cells */
  if (!COMP && !live)
    return;
  CompHead chead = {}; /* the staged descriptor's head: read for the composite frames of a COMP launch only */
  const CompHead *ch = &chead;
  if (COMP) { /* every lane reaches the barrier, the idle ones of the last workgroup too; f.comp is uniform per workgroup */
    if (f.comp)
      comp_stage<0, RASTER_BLOCK>(f.comp, (int)tid);
    __syncthreads();
    if (f.comp)
      chead = comp_head<0>();
  }
  if (live) {
    const uint32_t row = c / cols, col = c - row * cols;
    raster_cell_t v;
    v.slot = RASTER_NO_GLYPH;
    v.fg = p.default_fg;
    v.bg = p.default_bg;
    const int32_t ty = (int32_t)row - f.pad_top, x = (int32_t)col - f.pad_left;
    const bool given = (f.ops & ACHIP_OP_FG_OVERRIDE) != 0u; /* every truecolor foreground SGR carries this colour instead */
    const uint32_t given_rgb = cell_rgb(f.ops >> ACHIP_OP_TINT_SHIFT);
    if (ty >= 0 && ty < T && x < f.out_w) {
      if (x < 0) { /* a pad space: blank, but for the pen no reset has cleared */
        if (MODE == ACHIP_MODE_TRUE_FG && ty > 0)
          v.fg = given ? given_rgb : cell_rgb(truecolor_pen<COMP>(f, ch, slot, a.mixed != 0u, (uint32_t)f.out_w - 1u, (uint32_t)ty - 1u));
      } else if (!HB) {
        const uint32_t px = image_sample<COMP>(f, ch, (uint32_t)x, (uint32_t)ty);
        const uint32_t Y = luma601(px);
        v.slot = slot[Y] & 0xFFFFu;
        if (MODE == ACHIP_MODE_TRUE_FG) {
          v.fg = given ? given_rgb : a.mixed ? cell_rgb(truecolor_pen<COMP>(f, ch, slot, true, (uint32_t)x, (uint32_t)ty)) : cell_rgb(px);
        } else if (MODE == ACHIP_MODE_256_FG || MODE == ACHIP_MODE_16_FG) {
          v.fg = p.lut[indexed_key<MODE>(px)];
        } else if (MODE == ACHIP_MODE_TRUE_BG) {
          v.bg = cell_rgb(px);
          v.fg = given ? given_rgb : Y < 128u ? 0xFFFFFFu : 0u;
        }
      } else {
        const uint32_t yt = 2u * (uint32_t)ty, yb = yt + 1u;
        const bool twin = yb >= (uint32_t)f.out_h; /* an odd height: the last row's lower half repeats the upper */
        const uint32_t pt = image_sample<COMP>(f, ch, (uint32_t)x, yt);
        const uint32_t pb = twin ? pt : image_sample<COMP>(f, ch, (uint32_t)x, yb);
        if (MODE == ACHIP_MODE_HB_MONO) {
          const uint32_t lt = (76u * px_r(pt) + 150u * px_g(pt) + 29u * px_b(pt)) >> 8;
          const uint32_t lb = (76u * px_r(pb) + 150u * px_g(pb) + 29u * px_b(pb)) >> 8;
          if (lt >= 16u || lb >= 16u)
            v.slot = fixed[1u + (lt >> 6)];
        } else if (MODE == ACHIP_MODE_HB_TRUE) {
          if ((pt | pb) != 0u) {
            v.slot = fixed[0];
            v.fg = given ? given_rgb : cell_rgb(pt);
            v.bg = cell_rgb(pb);
          }
        } else {
          const uint32_t black = indexed_key<MODE>(0u);
          const uint32_t kt = indexed_key<MODE>(pt), kb = indexed_key<MODE>(pb);
          uint32_t head = pt | pb; /* the raw bytes of the run's first cell */
          if (kt == black && kb == black)
            for (uint32_t hx = (uint32_t)x; hx > 0u; hx--) {
              const uint32_t qt = image_sample<COMP>(f, ch, hx - 1u, yt);
              const uint32_t qb = twin ? qt : image_sample<COMP>(f, ch, hx - 1u, yb);
              if (indexed_key<MODE>(qt) != black || indexed_key<MODE>(qb) != black)
                break;
              head = qt | qb;
            }
          if (head != 0u) {
            v.slot = fixed[0];
            v.fg = p.lut[kt];
            v.bg = p.lut[256u + kb];
          }
        }
      }
    }
    cells[(uint64_t)fi * rows * cols + c] = v;
  }
}

} // namespace raster
} // namespace achip
