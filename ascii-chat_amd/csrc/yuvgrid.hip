/* yuvgrid.hip -- the launcher of libasciichat_yuvgrid.so (yuvgrid_kernels.hpp); the host side is yuvgrid.c. */
#include <hip/hip_runtime.h>

#include "yuvgrid.h"
#include "yuvgrid_kernels.hpp"

extern "C" int yuvgrid_launch_tiles(const yuvgrid_item_t *items, int n, uint32_t max_pixels, uint8_t *tiles, void *stream) {
  if (!items || n <= 0 || n > YUVGRID_MAX_TILES || max_pixels == 0u || max_pixels > (uint32_t)YUVGRID_MAX_SIDE * YUVGRID_MAX_SIDE || !tiles)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(achip::yuvgrid::tiles_kernel, dim3(yuvgrid_groups(max_pixels), (unsigned)n), dim3(YUV_BLOCK), 0,
                     static_cast<hipStream_t>(stream), items, tiles);
  return (int)hipGetLastError();
}
