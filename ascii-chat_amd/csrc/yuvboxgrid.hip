/* yuvboxgrid.hip -- the launcher of libasciichat_yuvboxgrid.so (yuvboxgrid_kernels.hpp); the host side is yuvboxgrid.c. */
#include <hip/hip_runtime.h>

#include "yuvboxgrid.h"
#include "yuvboxgrid_kernels.hpp"

extern "C" int yuvboxgrid_launch(const yuvboxgrid_item_t *items, int n, uint32_t workgroups, uint32_t stage_cols, uint8_t *tiles, void *stream) {
  if (!items || n <= 0 || n > YUVGRID_MAX_TILES || workgroups == 0u || workgroups > YUVBOXGRID_MAX_WORKGROUPS || stage_cols == 0u ||
      stage_cols > YUVBOX_MAX_SRC_W || !tiles)
    return (int)hipErrorInvalidValue;
  /* (the stage of the widest source is 46 080 bytes: below the 48 KB a launch may ask for without saying so first) */
  hipLaunchKernelGGL(achip::yuvboxgrid::tiles_kernel, dim3(workgroups), dim3(YUV_BLOCK), yuvboxgrid_lds_bytes(stage_cols),
                     static_cast<hipStream_t>(stream), items, (uint32_t)n, tiles);
  return (int)hipGetLastError();
}
