/* raster.hip -- the launchers of the rasteriser (raster_kernels.hpp, raster_yuv_kernels.hpp, raster_images_kernels.hpp,
 * raster_dither_kernels.hpp); the host side is raster.c. */
#include <hip/hip_runtime.h>

#include "launch_common.hpp"
#include "raster.h"
#include "raster_dither_kernels.hpp"
#include "raster_images_kernels.hpp"
#include "raster_kernels.hpp"
#include "raster_yuv_kernels.hpp"

extern "C" int raster_launch_parse(const raster_params_t *p, const uint8_t *frames, uint64_t frame_stride, const uint32_t *len, int n,
                                   uint32_t *starts, raster_rowrec_t *recs, raster_cell_t *cells, uint32_t *status, void *stream) {
  if (!p || !frames || !len || n <= 0 || !starts || !recs || !cells || !status)
    return (int)hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned rows = (unsigned)p->rows;
  hipLaunchKernelGGL(achip::raster::starts_kernel, dim3((unsigned)n), dim3(RASTER_BLOCK), 64, s, *p, frames, frame_stride, len, starts);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return (int)e;
  const unsigned bpf = (rows + 1u + RASTER_ROWS_PER_BLOCK - 1u) / RASTER_ROWS_PER_BLOCK;
  hipLaunchKernelGGL(achip::raster::parse_kernel, dim3((unsigned)n * bpf), dim3(RASTER_BLOCK), raster_parse_lds(), s, *p, frames,
                     frame_stride, len, starts, recs, cells);
  e = hipGetLastError();
  if (e != hipSuccess)
    return (int)e;
  const unsigned groups = (rows + RASTER_FIX_ROWS - 1u) / RASTER_FIX_ROWS;
  hipLaunchKernelGGL(achip::raster::resolve_kernel, dim3((unsigned)n * groups), dim3(RASTER_BLOCK), (2u * RASTER_FIX_ROWS + RASTER_BLOCK) * 4u,
                     s, *p, recs, cells, status);
  return (int)hipGetLastError();
}

extern "C" int raster_launch_draw(const raster_params_t *p, const raster_cell_t *cells, int n, uint8_t *pixels, uint64_t image_pitch,
                                  void *stream) {
  if (!p || !cells || n <= 0 || !pixels)
    return (int)hipErrorInvalidValue;
  const int lds = (int)raster_draw_lds(p);
  const hipError_t e = achip::ensure_dynamic_lds<achip::raster::draw_kernel>(lds);
  if (e != hipSuccess)
    return (int)e;
  const unsigned tiles = (unsigned)raster_tiles(p), strips = (unsigned)n * (unsigned)p->rows, split = raster_draw_split(p, n);
  hipLaunchKernelGGL(achip::raster::draw_kernel, dim3(strips, split), dim3(RASTER_BLOCK), (size_t)lds, static_cast<hipStream_t>(stream), *p,
                     cells, pixels, image_pitch, tiles);
  return (int)hipGetLastError();
}

extern "C" int raster_launch_draw_yuv(const raster_params_t *p, const raster_cell_t *cells, int n, uint8_t *yuv, uint64_t image_pitch,
                                      int layout, void *stream) {
  if (!p || !cells || n <= 0 || !yuv || ((p->cols * p->cell_w) & 1) || ((p->rows * p->cell_h) & 1) ||
      (layout != ASCIICHAT_RASTER_YUV_I420 && layout != ASCIICHAT_RASTER_YUV_NV12))
    return (int)hipErrorInvalidValue;
  const int lds = (int)raster_yuv_lds(p);
  const hipError_t e = achip::ensure_dynamic_lds<achip::raster::draw_yuv_kernel>(lds);
  if (e != hipSuccess)
    return (int)e;
  const unsigned strips = (unsigned)n * ((unsigned)p->rows / raster_yuv_span(p));
  hipLaunchKernelGGL(achip::raster::draw_yuv_kernel, dim3(strips, raster_yuv_split(p, n)), dim3(RASTER_BLOCK), (size_t)lds,
                     static_cast<hipStream_t>(stream), *p, cells, yuv, image_pitch, layout == ASCIICHAT_RASTER_YUV_NV12 ? 1u : 0u);
  return (int)hipGetLastError();
}

template <int MODE>
static void launch_cells_images(const raster_params_t *p, const raster_img_args_t *a, bool composites, int n, raster_cell_t *cells,
                                uint32_t *status, hipStream_t s) {
  const unsigned groups = ((unsigned)p->rows * (unsigned)p->cols + RASTER_IMG_CELLS - 1u) / RASTER_IMG_CELLS;
  if (composites) /* the staged composite descriptor is this form's only LDS */
    hipLaunchKernelGGL((achip::raster::cells_images_kernel<MODE, true>), dim3(groups, (unsigned)n), dim3(RASTER_BLOCK), ACHIP_COMP_LDS_BYTES, s,
                       *p, *a, cells, status);
  else
    hipLaunchKernelGGL((achip::raster::cells_images_kernel<MODE, false>), dim3(groups, (unsigned)n), dim3(RASTER_BLOCK), 0, s, *p, *a, cells,
                       status);
}

extern "C" int raster_launch_cells_images(const raster_params_t *p, const raster_img_args_t *a, int composites, int n, raster_cell_t *cells,
                                          uint32_t *status, void *stream) {
  if (!p || !a || !a->tables || !a->frames || n <= 0 || !cells || !status)
    return (int)hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool c = composites != 0;
  switch (a->mode) { /* a missing instantiation is an error, never another mode's kernel */
  case ACHIP_MODE_MONO: launch_cells_images<ACHIP_MODE_MONO>(p, a, c, n, cells, status, s); break;
  case ACHIP_MODE_TRUE_FG: launch_cells_images<ACHIP_MODE_TRUE_FG>(p, a, c, n, cells, status, s); break;
  case ACHIP_MODE_256_FG: launch_cells_images<ACHIP_MODE_256_FG>(p, a, c, n, cells, status, s); break;
  case ACHIP_MODE_16_FG: launch_cells_images<ACHIP_MODE_16_FG>(p, a, c, n, cells, status, s); break;
  case ACHIP_MODE_TRUE_BG: launch_cells_images<ACHIP_MODE_TRUE_BG>(p, a, c, n, cells, status, s); break;
  case ACHIP_MODE_HB_TRUE: launch_cells_images<ACHIP_MODE_HB_TRUE>(p, a, c, n, cells, status, s); break;
  case ACHIP_MODE_HB_256: launch_cells_images<ACHIP_MODE_HB_256>(p, a, c, n, cells, status, s); break;
  case ACHIP_MODE_HB_16: launch_cells_images<ACHIP_MODE_HB_16>(p, a, c, n, cells, status, s); break;
  case ACHIP_MODE_HB_MONO: launch_cells_images<ACHIP_MODE_HB_MONO>(p, a, c, n, cells, status, s); break;
  default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

/* the dithered mode: one workgroup per frame, the band and the error line in dynamic LDS (above 48 KB: announced once) */
template <bool COMP>
static hipError_t launch_cells_dither(const raster_params_t *p, const raster_img_args_t *a, int n, raster_cell_t *cells, uint32_t *status,
                                      hipStream_t s) {
  const hipError_t e = achip::ensure_dynamic_lds<achip::raster::cells_dither_kernel<COMP>>(RASTER_DITHER_LDS_BYTES);
  if (e != hipSuccess)
    return e;
  hipLaunchKernelGGL((achip::raster::cells_dither_kernel<COMP>), dim3((unsigned)n), dim3(RASTER_BLOCK), RASTER_DITHER_LDS_BYTES, s, *p, *a,
                     cells, status);
  return hipGetLastError();
}

extern "C" int raster_launch_cells_dither(const raster_params_t *p, const raster_img_args_t *a, int composites, int n, raster_cell_t *cells,
                                          uint32_t *status, void *stream) {
  if (!p || !a || !a->tables || !a->frames || a->mode != ACHIP_MODE_16_DITHER_BG || n <= 0 || !cells || !status)
    return (int)hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return (int)(composites ? launch_cells_dither<true>(p, a, n, cells, status, s) : launch_cells_dither<false>(p, a, n, cells, status, s));
}
