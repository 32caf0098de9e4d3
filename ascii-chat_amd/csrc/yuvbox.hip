/* yuvbox.hip -- the launcher of libasciichat_yuvbox.so (yuvbox_kernels.hpp); the host side is yuvbox.c. */
#include <hip/hip_runtime.h>

#include "yuvbox.h"
#include "yuvbox_kernels.hpp"

extern "C" int yuvbox_launch(const yuvbox_item_t *items_dev, const yuvbox_item_t *one, int n, int max_out_h, int max_src_w, uint8_t *images,
                             uint64_t pitch, void *stream) {
  if ((!items_dev && (!one || n != 1)) || n <= 0 || n > YUV_MAX_FRAMES || !images || max_out_h <= 0 || max_out_h > YUVBOX_MAX_OUT ||
      max_src_w <= 0 || max_src_w > YUVBOX_MAX_SRC_W || (uint64_t)n * (uint64_t)max_out_h > 0x7FFFFFFFull)
    return (int)hipErrorInvalidValue;
  yuvbox_item_t by_value = {};
  if (!items_dev)
    by_value = *one;
  /* (the stage of the widest source is 46 080 bytes: below the 48 KB a launch may ask for without saying so first) */
  hipLaunchKernelGGL(achip::yuvbox::box_kernel, dim3((unsigned)n * (unsigned)max_out_h), dim3(YUV_BLOCK), yuvbox_lds_bytes(max_src_w),
                     static_cast<hipStream_t>(stream), items_dev, by_value, (uint32_t)max_out_h, images, pitch);
  return (int)hipGetLastError();
}
