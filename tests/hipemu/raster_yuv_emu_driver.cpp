/* raster_yuv_emu_driver.cpp -- the rasteriser's YUV 4:2:0 draw (ascii-chat_amd/csrc/raster_yuv_kernels.hpp) under the fiber
 * emulator: the parse kernels, then draw_yuv_kernel launched as raster.hip launches it; and the conversion arithmetic of
 * raster_yuv.h on its own.  TESTS ONLY. */
#include "raster_yuv_kernels.hpp"

#include <vector>

/* the pixels of an image row whose cells a workgroup holds at a time: the tests place images across its multiples */
extern "C" int emu_raster_yuv_tile(int cell_w) { return RASTER_YUV_TILE_CELLS * cell_w; }

/* raster_yuv.h, unclamped: out = {Y(r, g, b), U(r, g, b), V(r, g, b)} */
extern "C" void emu_raster_yuv_convert(uint32_t r, uint32_t g, uint32_t b, int32_t *out) {
  out[0] = (int32_t)raster_yuv_y(r, g, b), out[1] = (int32_t)raster_yuv_u(r, g, b), out[2] = (int32_t)raster_yuv_v(r, g, b);
}
extern "C" uint32_t emu_raster_yuv_avg(uint32_t sum4) { return raster_yuv_avg(sum4); }
/* ... over all 2^24 inputs, index r << 16 | g << 8 | b */
extern "C" void emu_raster_yuv_all(int32_t *y, int32_t *u, int32_t *v) {
  for (uint32_t i = 0; i < (1u << 24); i++) {
    const uint32_t r = i >> 16, g = (i >> 8) & 255u, b = i & 255u;
    y[i] = (int32_t)raster_yuv_y(r, g, b), u[i] = (int32_t)raster_yuv_u(r, g, b), v[i] = (int32_t)raster_yuv_v(r, g, b);
  }
}

/* asciichat_raster_create + asciichat_raster_run_yuv420 over host memory.  atlas_through_l2: read the coverage from memory
 * although it would fit the LDS stage.  split: the workgroups a strip's slots are spread over, 0 for raster.hip's choice (the
 * kernel takes any; small test batches would otherwise never give a thread a second slot).  Returns -1 when raster.h refuses the font or the grid, -2 for what run_yuv420 refuses
 * (an odd size, an unknown layout). */
extern "C" int emu_raster_yuv(const asciichat_raster_font_t *font, int cols, int rows, const uint8_t *frames, uint64_t stride,
                              const uint32_t *len, int n, uint8_t *yuv, uint64_t pitch, int layout, uint32_t *status,
                              int atlas_through_l2, int split) {
  if (raster_check(font, cols, rows, n))
    return -1;
  if (((cols * font->cell_w) & 1) || ((rows * font->cell_h) & 1) ||
      (layout != ASCIICHAT_RASTER_YUV_I420 && layout != ASCIICHAT_RASTER_YUV_NV12))
    return -2;
  const size_t ng = (size_t)font->n_glyphs;
  std::vector<uint32_t> cps(ng + 1), lut(512);
  std::vector<raster_glyph_t> glyphs(ng + 1);
  raster_tables(font, cps.data(), glyphs.data(), lut.data());
  std::vector<uint4> cov((font->coverage_bytes + 15u) / 16u + 1u); /* 16-byte aligned, padded to 16 as the device copy is */
  if (font->coverage_bytes)
    memcpy(cov.data(), font->coverage, font->coverage_bytes);
  raster_params_t p;
  memset(&p, 0, sizeof(p));
  p.cols = cols, p.rows = rows, p.cell_w = font->cell_w, p.cell_h = font->cell_h;
  p.n_glyphs = font->n_glyphs, p.matrix_map = font->matrix_map != 0;
  p.default_fg = font->default_fg & 0xFFFFFFu, p.default_bg = font->default_bg & 0xFFFFFFu;
  p.codepoints = cps.data(), p.glyphs = glyphs.data(), p.lut = lut.data();
  p.coverage = reinterpret_cast<const uint8_t *>(cov.data());
  p.coverage_bytes = (uint32_t)font->coverage_bytes;
  p.atlas_in_lds = font->coverage_bytes <= RASTER_ATLAS_LDS && !atlas_through_l2;

  const size_t nr = (size_t)rows, nc = (size_t)cols;
  std::vector<uint32_t> starts((size_t)n * (nr + 2), 0xDEADBEEFu);
  std::vector<raster_rowrec_t> recs((size_t)n * (nr + 1));
  std::vector<raster_cell_t> cells((size_t)n * nr * nc);
  memset(recs.data(), 0xEE, recs.size() * sizeof(recs[0]));
  memset(cells.data(), 0xEE, cells.size() * sizeof(cells[0]));
  hipemu::launch(dim3((unsigned)n), dim3(RASTER_BLOCK), 64, [&] { achip::raster::starts_kernel(p, frames, stride, len, starts.data()); });
  const unsigned bpf = ((unsigned)rows + 1u + RASTER_ROWS_PER_BLOCK - 1u) / RASTER_ROWS_PER_BLOCK;
  hipemu::launch(dim3((unsigned)n * bpf), dim3(RASTER_BLOCK), raster_parse_lds(),
                 [&] { achip::raster::parse_kernel(p, frames, stride, len, starts.data(), recs.data(), cells.data()); });
  const unsigned groups = ((unsigned)rows + RASTER_FIX_ROWS - 1u) / RASTER_FIX_ROWS;
  hipemu::launch(dim3((unsigned)n * groups), dim3(RASTER_BLOCK), (2u * RASTER_FIX_ROWS + RASTER_BLOCK) * 4u,
                 [&] { achip::raster::resolve_kernel(p, recs.data(), cells.data(), status); });
  const unsigned strips = (unsigned)n * ((unsigned)rows / raster_yuv_span(&p));
  hipemu::launch(dim3(strips, split > 0 ? (unsigned)split : raster_yuv_split(&p, n)), dim3(RASTER_BLOCK), raster_yuv_lds(&p),
                 [&] { achip::raster::draw_yuv_kernel(p, cells.data(), yuv, pitch, layout == ASCIICHAT_RASTER_YUV_NV12 ? 1u : 0u); });
  return 0;
}
