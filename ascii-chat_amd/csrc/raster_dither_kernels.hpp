/*
 * raster_dither_kernels.hpp -- the rasteriser's cell grids straight from frame descriptors in the Floyd-Steinberg mode
 * (asciichat_raster_images_set_dithered, include/asciichat_raster.h): ACHIP_MODE_16_DITHER_BG, the one mode whose cell is no
 * function of its own sample.  The colour index of a sample depends on the error diffused from every sample before it, so the
 * frame is dithered here as the renderer dithers it -- dither16_rows (render_kernels.hpp), unchanged, through an LDS layout of this
 * file's -- and what the renderer would write as text and the parser read back is written as cells at once.
 *
 * One workgroup of RASTER_BLOCK threads per frame.  The frame's text rows that lie in the grid are walked in BANDS of as many
 * whole rows as RASTER_DITHER_CAP samples hold (a multiple of 64 rows where more than 64 fit, so that a band is whole sweeps):
 *   A  all waves sample the band into LDS (four requests in flight per lane), one dword per sample, row-major without padding;
 *   B  wave 0 runs the error wavefront over the band: lane y walks row y two columns behind lane y - 1, sweeps of up to 64 rows
 *      chained through the 3 x int per column error line, which also carries the state from band to band; it leaves the colour
 *      index in bits 31..24 of every sample;
 *   C  all waves turn the band's grid rows -- pad cells, text cells, the cells behind the text -- into 12-byte cells, cell c of the
 *      band by lane c mod 256: a wave stores 768 contiguous bytes.
 * Three barriers per band (A | B | C | the next A overwrites what C read).  The cells of the grid rows above pad_top and behind the
 * text are blanked by all waves in front of the first band.  Every cell of the frame's grid is written exactly once.
 *
 * All out_w columns of a row are dithered, the ones beyond the grid's columns too: they diffuse into visible cells of the row
 * below.  Text rows behind the grid's last row are not: nothing flows upwards.  The error line bounds out_w by
 * RASTER_DITHER_MAX_W (= ASCIICHAT_RASTER_MAX_COLS: no handle shows a wider row); the host refuses a wider frame
 * (raster_images_dithered_check), and a workgroup that met one all the same would blank its grid and touch no LDS.
 *
 * The rule per cell is build_token's branch for this mode (render_kernels.hpp) read through the parser's grammar: with idx the
 * dithered index and Y the luminance of the ORIGINAL sample,
 *   background form          bg = lut[256 + idx], fg = lut[15] when the palette colour's 77/150/29 / 256 luminance is below 127,
 *                            else lut[0], glyph cache[Y];
 *   ACHIP_OP_DITHER_FG       fg = lut[idx], bg the default, glyph cache[Y] -- with ACHIP_OP_DITHER_RAMP cache[ramp[Y >> 2]].
 * Every text row ends in a reset, so pad cells and everything outside the text are blank under the default pen.  Flips and tints
 * act through the sampler (not on a composite frame); FG_OVERRIDE changes nothing, for the mode emits no truecolor SGR.
 * COMP as in raster_images_kernels.hpp: the kernel of a set in which some frame carries comp stages the 464-byte descriptor at LDS
 * offset 0 behind one barrier and samples through the staged sampler.
 * Only plain HIP and gfx950_ops.hpp: the same source runs under the CPU emulator (tests/hipemu).
 */
#pragma once

#include "raster_images.h"
#include "raster_images_kernels.hpp"
#include "render_kernels.hpp"

namespace achip {
namespace raster {

/* the LDS block: the staged composite descriptor (COMP launches), the error line, the band; dither16_rows reads o_pixT, o_carry */
struct DitherLds {
  static constexpr int o_comp = 0;
  static constexpr int o_carry = (ACHIP_COMP_LDS_BYTES + 15) & ~15;
  static constexpr int o_pixT = o_carry + 12 * RASTER_DITHER_MAX_W;
  static constexpr int bytes = o_pixT + 4 * RASTER_DITHER_CAP;
};
static_assert(DitherLds::bytes == RASTER_DITHER_LDS_BYTES, "raster_images.h states the launch's LDS");
static_assert(RASTER_DITHER_CAP >= RASTER_DITHER_MAX_W, "a band holds one row at least");

/* text rows of a band for a frame out_w (1..RASTER_DITHER_MAX_W) samples wide */
__device__ inline int dither_band_rows(int out_w) {
  const int fit = RASTER_DITHER_CAP / out_w;
  return fit > 64 ? fit & ~63 : fit;
}

template <bool COMP>
__global__ void __launch_bounds__(RASTER_BLOCK)
    cells_dither_kernel(const raster_params_t p, const raster_img_args_t a, raster_cell_t *__restrict__ cells, uint32_t *__restrict__ status) {
  using L = DitherLds;
  const uint32_t fi = blockIdx.x;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  const int cols = p.cols, rows = p.rows;
  achip_frame_t f = a.frames[fi];
  if (f.src_stride == 0) /* tightly packed, as the render kernels read it */
    f.src_stride = 3 * f.src_w;
  const uint32_t *__restrict__ slot = a.tables->slot;
  if (tid == 0) { /* what the parser would report, by cells_images_kernel's two conditions */
    uint32_t st = 0u;
    if ((long long)f.pad_left + f.out_w > (long long)cols && f.pad_top < rows)
      st |= ASCIICHAT_RASTER_OVERFLOW_COLS;
    if ((long long)f.pad_top + f.out_h > (long long)rows)
      st |= ASCIICHAT_RASTER_OVERFLOW_ROWS;
    status[fi] = st;
  }
  raster_cell_t *__restrict__ grid = cells + (uint64_t)fi * (uint32_t)rows * (uint32_t)cols;
  raster_cell_t blank;
  blank.slot = RASTER_NO_GLYPH;
  blank.fg = p.default_fg;
  blank.bg = p.default_bg;

  /* the text rows to dither: those in the grid */
  const int top = min(max(f.pad_top, 0), rows);
  int proc = min(max(f.out_h, 0), rows - top);
  if (f.out_w < 1 || f.out_w > RASTER_DITHER_MAX_W)
    proc = 0; /* (the host refuses such a frame) */
  {           /* the grid rows above and behind them */
    const int head = top * cols, tail_from = (top + proc) * cols, total = rows * cols;
    for (int c = tid; c < head; c += RASTER_BLOCK)
      grid[c] = blank;
    for (int c = tail_from + tid; c < total; c += RASTER_BLOCK)
      grid[c] = blank;
  }

  if (proc == 0) /* (uniform: the whole workgroup leaves) */
    return;
  CompHead chead = {};
  const CompHead *ch = &chead;
  if (COMP) { /* f.comp is uniform: the workgroup is the frame's */
    if (f.comp)
      comp_stage<L::o_comp, RASTER_BLOCK>(f.comp, tid);
    __syncthreads();
    if (f.comp)
      chead = comp_head<L::o_comp>();
  }

  uint32_t *pixT = lds_ptr<uint32_t>(L::o_pixT);
  int *carry = lds_ptr<int>(L::o_carry);
  const int w = f.out_w;
  for (int k = tid; k < 3 * w; k += RASTER_BLOCK) /* no error enters the first row */
    carry[k] = 0;
  const bool fg_form = (f.ops & ACHIP_OP_DITHER_FG) != 0u, ramp_glyph = (f.ops & ACHIP_OP_DITHER_RAMP) != 0u;
  const uint32_t fg_dark = p.lut[15], fg_bright = p.lut[0];
  const int band = dither_band_rows(w);

  for (int r0 = 0; r0 < proc; r0 += band) {
    const int r1 = min(proc, r0 + band);
    const int n = (r1 - r0) * w;
    /* ---- A: the band's samples ---- */
    for (int base = tid; base < n; base += 4 * RASTER_BLOCK) {
      uint32_t v[4], kind[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int i = base + k * RASTER_BLOCK;
        v[k] = 0u;
        kind[k] = RAW_FINAL;
        if (i < n) {
          const int rr = i / w;
          v[k] = sample_frame_raw<COMP, COMP ? L::o_comp : -1>(f, (uint32_t)(i - rr * w), (uint32_t)(r0 + rr), kind[k], ch);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int i = base + k * RASTER_BLOCK;
        if (i < n)
          pixT[i] = px_rgb(sample_finish<COMP>(f, v[k], kind[k]));
      }
    }
    __syncthreads();
    /* ---- B: one wave diffuses the errors and leaves the colour index in the key byte ---- */
    if (wave == 0)
      dither16_rows<L>(lane, r1 - r0, w, 0, w, r0, proc);
    __syncthreads();
    /* ---- C: the band's grid rows as cells ---- */
    raster_cell_t *__restrict__ out = grid + (uint32_t)(top + r0) * (uint32_t)cols;
    const int ncell = (r1 - r0) * cols;
    for (int c = tid; c < ncell; c += RASTER_BLOCK) {
      const int rr = c / cols, x = c - rr * cols - f.pad_left;
      raster_cell_t cell = blank;
      if (x >= 0 && x < w) {
        const uint32_t px = pixT[rr * w + x];
        const uint32_t idx = px_key(px), s = slot[luma601(px)];
        if (fg_form) {
          cell.slot = ramp_glyph ? s >> 16 : s & 0xFFFFu;
          cell.fg = p.lut[idx];
        } else {
          const uint32_t pal = ansi16_rgb(idx);
          const uint32_t bl = (77u * px_r(pal) + 150u * px_g(pal) + 29u * px_b(pal)) / 256u;
          cell.slot = s & 0xFFFFu;
          cell.fg = bl < 127u ? fg_dark : fg_bright;
          cell.bg = p.lut[256u + idx];
        }
      }
      out[c] = cell;
    }
    if (r1 < proc)
      __syncthreads(); /* the next band's samples overwrite what C read */
  }
}

} // namespace raster
} // namespace achip
