/* box.hip -- the launchers of the area-average downscale pass (box_kernels.hpp); the host side is box.c. */
#include <hip/hip_runtime.h>

#include "box.h"
#include "box_kernels.hpp"
#include "launch_common.hpp"

extern "C" int achip_launch_box(const achip_box_desc_t *desc_dev, const achip_box_uniform_t *uniform, int n, int max_out_h,
                                int max_src_w, uint8_t *images, uint64_t pitch, void *stream) {
  if (n <= 0)
    return (int)hipSuccess;
  achip_box_uniform_t uni = {};
  if (uniform && uniform->enabled)
    uni = *uniform;
  if ((!uni.enabled && !desc_dev) || !images || max_out_h <= 0 || max_out_h > ACHIP_BOX_MAX_OUT || max_src_w <= 0 ||
      max_src_w > ACHIP_BOX_MAX_SRC_W || (uint64_t)n * (uint64_t)max_out_h > 0x7FFFFFFFull)
    return (int)hipErrorInvalidValue;
  const int lds = (int)achip::box::lds_bytes(max_src_w);
  const hipError_t e = achip::ensure_dynamic_lds<achip::box::box_kernel>(lds);
  if (e != hipSuccess)
    return (int)e;
  hipLaunchKernelGGL(achip::box::box_kernel, dim3((unsigned)n * (unsigned)max_out_h), dim3(ACHIP_BOX_BLOCK), (size_t)lds,
                     static_cast<hipStream_t>(stream), desc_dev, uni, (uint32_t)max_out_h, images, pitch);
  return (int)hipGetLastError();
}

extern "C" int box_canvas_launch(const achip_box_canvas_t *table_dev, int n, int max_out_h, int max_canvas_w, const uint8_t *tiles,
                                 uint64_t tile_pitch, uint8_t *images, uint64_t pitch, void *stream) {
  if (n <= 0)
    return (int)hipSuccess;
  if (!table_dev || !images || max_out_h <= 0 || max_out_h > ACHIP_BOX_MAX_OUT || max_canvas_w <= 0 ||
      max_canvas_w > ACHIP_BOX_MAX_SRC_W || (uint64_t)n * (uint64_t)max_out_h > 0x7FFFFFFFull)
    return (int)hipErrorInvalidValue;
  const int lds = (int)achip::box::lds_bytes(max_canvas_w);
  const hipError_t e = achip::ensure_dynamic_lds<achip::box::box_canvas_kernel>(lds);
  if (e != hipSuccess)
    return (int)e;
  hipLaunchKernelGGL(achip::box::box_canvas_kernel, dim3((unsigned)n * (unsigned)max_out_h), dim3(ACHIP_BOX_BLOCK), (size_t)lds,
                     static_cast<hipStream_t>(stream), table_dev, (uint32_t)max_out_h, tiles, tile_pitch, images, pitch);
  return (int)hipGetLastError();
}
