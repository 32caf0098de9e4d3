/* pixgrid.hip -- the launchers of libasciichat_pixgrid.so (pixgrid_kernels.hpp); the host side is pixgrid.c. */
#include <hip/hip_runtime.h>

#include "pixgrid.h"
#include "pixgrid_kernels.hpp"

extern "C" int pixgrid_launch_tiles(const pixgrid_item_t *items, int n, uint32_t max_pixels, uint8_t *tiles, void *stream) {
  if (!items || n <= 0 || n > PIXGRID_MAX_TILES || max_pixels == 0u || !tiles)
    return (int)hipErrorInvalidValue;
  const unsigned lanes = (max_pixels + 3u) / 4u, groups = (lanes + PIX_BLOCK - 1u) / PIX_BLOCK;
  hipLaunchKernelGGL(achip::pixgrid::tiles_kernel, dim3(groups, (unsigned)n), dim3(PIX_BLOCK), 0, static_cast<hipStream_t>(stream), items, tiles);
  return (int)hipGetLastError();
}

extern "C" int pixgrid_launch_box(const pixgrid_item_t *items, int n, uint32_t workgroups, uint32_t stage_cols, uint8_t *tiles, void *stream) {
  if (!items || n <= 0 || n > PIXGRID_MAX_TILES || workgroups == 0u || workgroups > PIXGRID_MAX_WORKGROUPS || stage_cols == 0u ||
      stage_cols > PIX_BOX_MAX_SRC_W || !tiles)
    return (int)hipErrorInvalidValue;
  /* (the stage of the widest source is 46 080 bytes: below the 48 KB a launch may ask for without saying so first) */
  hipLaunchKernelGGL(achip::pixgrid::box_tiles_kernel, dim3(workgroups), dim3(PIX_BLOCK), pixgrid_lds_bytes(stage_cols),
                     static_cast<hipStream_t>(stream), items, (uint32_t)n, tiles);
  return (int)hipGetLastError();
}
