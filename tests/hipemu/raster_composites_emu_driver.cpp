/* raster_composites_emu_driver.cpp -- the rasteriser's cells-from-images kernel in both its forms (ascii-chat_amd/csrc/
 * raster_images_kernels.hpp: COMP = true with the staged composite sampler, COMP = false without) and the unchanged draw kernel
 * (raster_kernels.hpp) under the fiber emulator, from a font, a mode, a palette and descriptors as raster.c takes them for
 * asciichat_raster_images_set_composites and launched as raster.hip launches them.  The composite descriptors are host memory
 * here.  TESTS ONLY. */
#include "raster_images_kernels.hpp"
#include "raster_kernels.hpp"

#include <vector>

extern "C" int emu_raster_composites_cells_per_group(void) { return RASTER_IMG_CELLS; }
extern "C" int emu_raster_composites_lds_bytes(void) { return ACHIP_COMP_LDS_BYTES; }

/* what asciichat_raster_images_set_composites decides on the host: 0 taken, 1 refused (why, bad and composites receive the
 * reason, the offending frame and the number of composite frames, when given) */
extern "C" int emu_raster_composites_check(int mode, const char *palette, const achip_frame_t *frames, int n, int max_frames,
                                           const char **why, int *bad, int *composites) {
  const char *w = raster_images_composites_check(mode, palette, frames, n, max_frames, bad, composites);
  if (why)
    *why = w;
  return w ? 1 : 0;
}

template <int MODE, bool COMP>
static void launch_form(const raster_params_t &p, const raster_img_args_t &a, int n, raster_cell_t *cells, uint32_t *status) {
  const unsigned groups = ((unsigned)p.rows * (unsigned)p.cols + RASTER_IMG_CELLS - 1u) / RASTER_IMG_CELLS;
  hipemu::launch(dim3(groups, (unsigned)n), dim3(RASTER_BLOCK), COMP ? ACHIP_COMP_LDS_BYTES : 0,
                 [&] { achip::raster::cells_images_kernel<MODE, COMP>(p, a, cells, status); });
}

template <int MODE>
static void launch_cells(const raster_params_t &p, const raster_img_args_t &a, bool comp, int n, raster_cell_t *cells, uint32_t *status) {
  if (comp)
    launch_form<MODE, true>(p, a, n, cells, status);
  else
    launch_form<MODE, false>(p, a, n, cells, status);
}

/* asciichat_raster_create + a set of n_set descriptors + run_images of the first n over host memory.  entry 0: the set goes
 * through images_set_composites (the kernel form follows the set: COMP when a frame carries a composite); entry 1: through
 * images_set.  force_comp: the COMP form whatever the set holds (a plain set in the form with the barrier).  cells_out
 * (optional): the n * rows * cols cells.  form_out (optional): 1 when the COMP form ran.  Returns -1 when raster.h refuses the
 * font or the grid, -2 when raster_images.h refuses the set or n is outside 1..n_set. */
extern "C" int emu_raster_composites(const asciichat_raster_font_t *font, int cols, int rows, int max_frames, int mode, const char *palette,
                                     const achip_frame_t *frames, int n_set, int n, int entry, int force_comp, uint8_t *pixels,
                                     uint64_t pitch, uint32_t *status, raster_cell_t *cells_out, int *form_out) {
  if (raster_check(font, cols, rows, max_frames))
    return -1;
  int composites = 0;
  const char *why = entry == 0 ? raster_images_composites_check(mode, palette, frames, n_set, max_frames, nullptr, &composites)
                               : raster_images_check(mode, palette, frames, n_set, max_frames, nullptr);
  if (why || n < 1 || n > n_set)
    return -2;
  const bool comp = composites > 0 || force_comp != 0;
  if (form_out)
    *form_out = comp ? 1 : 0;
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
  a.mode = mode;
  a.mixed = raster_images_tables(mode, palette, cps.data(), font->n_glyphs, p.matrix_map, reinterpret_cast<raster_img_tables_t *>(block.data()));
  memcpy(block.data() + raster_images_at_frames(), frames, (size_t)n_set * sizeof(achip_frame_t));
  a.tables = reinterpret_cast<const raster_img_tables_t *>(block.data());
  a.frames = reinterpret_cast<const achip_frame_t *>(block.data() + raster_images_at_frames());

  std::vector<raster_cell_t> cells((size_t)n * (size_t)rows * (size_t)cols);
  memset(cells.data(), 0xEE, cells.size() * sizeof(cells[0]));
  switch (mode) {
  case ACHIP_MODE_MONO: launch_cells<ACHIP_MODE_MONO>(p, a, comp, n, cells.data(), status); break;
  case ACHIP_MODE_TRUE_FG: launch_cells<ACHIP_MODE_TRUE_FG>(p, a, comp, n, cells.data(), status); break;
  case ACHIP_MODE_256_FG: launch_cells<ACHIP_MODE_256_FG>(p, a, comp, n, cells.data(), status); break;
  case ACHIP_MODE_16_FG: launch_cells<ACHIP_MODE_16_FG>(p, a, comp, n, cells.data(), status); break;
  case ACHIP_MODE_TRUE_BG: launch_cells<ACHIP_MODE_TRUE_BG>(p, a, comp, n, cells.data(), status); break;
  case ACHIP_MODE_HB_TRUE: launch_cells<ACHIP_MODE_HB_TRUE>(p, a, comp, n, cells.data(), status); break;
  case ACHIP_MODE_HB_256: launch_cells<ACHIP_MODE_HB_256>(p, a, comp, n, cells.data(), status); break;
  case ACHIP_MODE_HB_16: launch_cells<ACHIP_MODE_HB_16>(p, a, comp, n, cells.data(), status); break;
  default: launch_cells<ACHIP_MODE_HB_MONO>(p, a, comp, n, cells.data(), status); break;
  }
  if (cells_out)
    memcpy(cells_out, cells.data(), cells.size() * sizeof(cells[0]));
  const unsigned tiles = (unsigned)raster_tiles(&p);
  hipemu::launch(dim3((unsigned)n * (unsigned)rows, raster_draw_split(&p, n)), dim3(RASTER_BLOCK), raster_draw_lds(&p),
                 [&] { achip::raster::draw_kernel(p, cells.data(), pixels, pitch, tiles); });
  return 0;
}
