/* raster_emu_driver.cpp -- the rasteriser's kernels (ascii-chat_amd/csrc/raster_kernels.hpp) under the fiber emulator, from a
 * font as raster.c takes it and launched as raster.hip launches them.  TESTS ONLY. */
#include "raster_kernels.hpp"

#include <vector>

/* the bytes of a text row a wave stages at a time: the tests place tokens across its multiples */
extern "C" int emu_raster_chunk(void) { return RASTER_CHUNK; }

/* asciichat_raster_create + asciichat_raster_run over host memory.  atlas_through_l2: read the coverage from memory although
 * it would fit the LDS stage.  cells_out (optional): the n * rows * cols resolved cells.  Returns -1 when raster.h refuses
 * the font or the grid. */
extern "C" int emu_raster(const asciichat_raster_font_t *font, int cols, int rows, const uint8_t *frames, uint64_t stride,
                          const uint32_t *len, int n, uint8_t *pixels, uint64_t pitch, uint32_t *status, int atlas_through_l2,
                          raster_cell_t *cells_out) {
  if (raster_check(font, cols, rows, n))
    return -1;
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
  if (cells_out)
    memcpy(cells_out, cells.data(), cells.size() * sizeof(cells[0]));
  const unsigned tiles = (unsigned)raster_tiles(&p);
  hipemu::launch(dim3((unsigned)n * (unsigned)rows, raster_draw_split(&p, n)), dim3(RASTER_BLOCK), raster_draw_lds(&p),
                 [&] { achip::raster::draw_kernel(p, cells.data(), pixels, pitch, tiles); });
  return 0;
}
