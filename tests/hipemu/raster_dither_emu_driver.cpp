/* raster_dither_emu_driver.cpp -- the rasteriser's dithered cells-from-images kernel in both its forms (ascii-chat_amd/csrc/
 * raster_dither_kernels.hpp: COMP = true with the staged composite sampler, COMP = false without) and the unchanged draw kernel
 * (raster_kernels.hpp) under the fiber emulator, from a font, a palette and descriptors as raster.c takes them for
 * asciichat_raster_images_set_dithered and launched as raster.hip launches them.  The composite descriptors are host memory
 * here.  TESTS ONLY. */
#include "raster_dither_kernels.hpp"
#include "raster_kernels.hpp"

#include <vector>

extern "C" int emu_raster_dither_cap(void) { return RASTER_DITHER_CAP; }
extern "C" int emu_raster_dither_max_w(void) { return RASTER_DITHER_MAX_W; }
extern "C" int emu_raster_dither_lds_bytes(void) { return RASTER_DITHER_LDS_BYTES; }
/* text rows of a band for a frame out_w samples wide: the kernel's own rule */
extern "C" int emu_raster_dither_band_rows(int out_w) { return achip::raster::dither_band_rows(out_w); }

/* what asciichat_raster_images_set_dithered decides on the host: 0 taken, 1 refused (why, bad and composites receive the
 * reason, the offending frame and the number of composite frames, when given) */
extern "C" int emu_raster_dither_check(const char *palette, const achip_frame_t *frames, int n, int max_frames, const char **why, int *bad,
                                       int *composites) {
  const char *w = raster_images_dithered_check(palette, frames, n, max_frames, bad, composites);
  if (why)
    *why = w;
  return w ? 1 : 0;
}

/* asciichat_raster_create + a set of n_set descriptors through images_set_dithered + run_images of the first n over host
 * memory.  force_comp: the COMP form whatever the set holds.  cells_out (optional): the n * rows * cols cells.  Returns -1 when
 * raster.h refuses the font or the grid, -2 when raster_images.h refuses the set or n is outside 1..n_set. */
extern "C" int emu_raster_dither(const asciichat_raster_font_t *font, int cols, int rows, int max_frames, const char *palette,
                                 const achip_frame_t *frames, int n_set, int n, int force_comp, uint8_t *pixels, uint64_t pitch,
                                 uint32_t *status, raster_cell_t *cells_out) {
  if (raster_check(font, cols, rows, max_frames))
    return -1;
  int composites = 0;
  if (raster_images_dithered_check(palette, frames, n_set, max_frames, nullptr, &composites) || n < 1 || n > n_set)
    return -2;
  const bool comp = composites > 0 || force_comp != 0;
  const size_t ng = (size_t)font->n_glyphs;
  std::vector<uint32_t> cps(ng + 1), lut(512);
  std::vector<raster_glyph_t> glyphs(ng + 1);
  raster_tables(font, cps.data(), glyphs.data(), lut.data());
  std::vector<uint4> cov((font->coverage_bytes + 15u) / 16u + 1u);
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
  p.atlas_in_lds = font->coverage_bytes <= RASTER_ATLAS_LDS;

  /* the set as the handle stages it: the table, then exactly the descriptors that were set */
  std::vector<uint8_t> block(raster_images_bytes(n_set));
  raster_img_args_t a;
  a.mode = ACHIP_MODE_16_DITHER_BG;
  a.mixed = 0u;
  raster_images_dither_tables(palette, cps.data(), font->n_glyphs, p.matrix_map, reinterpret_cast<raster_img_tables_t *>(block.data()));
  memcpy(block.data() + raster_images_at_frames(), frames, (size_t)n_set * sizeof(achip_frame_t));
  a.tables = reinterpret_cast<const raster_img_tables_t *>(block.data());
  a.frames = reinterpret_cast<const achip_frame_t *>(block.data() + raster_images_at_frames());

  std::vector<raster_cell_t> cells((size_t)n * (size_t)rows * (size_t)cols);
  memset(cells.data(), 0xEE, cells.size() * sizeof(cells[0]));
  if (comp)
    hipemu::launch(dim3((unsigned)n), dim3(RASTER_BLOCK), RASTER_DITHER_LDS_BYTES,
                   [&] { achip::raster::cells_dither_kernel<true>(p, a, cells.data(), status); });
  else
    hipemu::launch(dim3((unsigned)n), dim3(RASTER_BLOCK), RASTER_DITHER_LDS_BYTES,
                   [&] { achip::raster::cells_dither_kernel<false>(p, a, cells.data(), status); });
  if (cells_out)
    memcpy(cells_out, cells.data(), cells.size() * sizeof(cells[0]));
  const unsigned tiles = (unsigned)raster_tiles(&p);
  hipemu::launch(dim3((unsigned)n * (unsigned)rows, raster_draw_split(&p, n)), dim3(RASTER_BLOCK), raster_draw_lds(&p),
                 [&] { achip::raster::draw_kernel(p, cells.data(), pixels, pitch, tiles); });
  return 0;
}
