/* yuv.hip -- the launchers of libasciichat_yuv.so (yuv_kernels.hpp); the host side is yuv.c. */
#include <hip/hip_runtime.h>

#include "yuv.h"
#include "yuv_kernels.hpp"

extern "C" int yuv_launch_sample(const asciichat_yuv_source_t *sources, const achip_frame_t *frames, int n, uint32_t max_pixels,
                                 uint8_t *images, uint64_t pitch, void *stream) {
  if (!sources || !frames || n <= 0 || n > YUV_MAX_FRAMES || max_pixels == 0u || !images)
    return (int)hipErrorInvalidValue;
  const unsigned lanes = (max_pixels + 3u) / 4u, groups = (lanes + YUV_BLOCK - 1u) / YUV_BLOCK;
  hipLaunchKernelGGL(achip::yuv::sample_kernel, dim3(groups, (unsigned)n), dim3(YUV_BLOCK), 0, static_cast<hipStream_t>(stream), sources,
                     frames, images, pitch);
  return (int)hipGetLastError();
}

template <int FORMAT> static void launch_whole(const yuv_whole_args_t *a, int n, int max_w, int max_h, hipStream_t s) {
  const unsigned rows = (FORMAT == ASCIICHAT_YUV_I420 || FORMAT == ASCIICHAT_YUV_NV12) ? 2u : 1u;
  const unsigned bw = ((unsigned)max_w + 3u) / 4u, bh = ((unsigned)max_h + rows - 1u) / rows;
  const dim3 grid((bw + YUV_WHOLE_LANES_X - 1u) / YUV_WHOLE_LANES_X, (bh + YUV_WHOLE_LANES_Y - 1u) / YUV_WHOLE_LANES_Y, (unsigned)n);
  hipLaunchKernelGGL((achip::yuv::whole_kernel<FORMAT>), grid, dim3(YUV_BLOCK), 0, s, *a);
}

extern "C" int yuv_launch_whole(const yuv_whole_args_t *a, int n, int max_w, int max_h, unsigned formats, void *stream) {
  if (!a || !a->rgb || n <= 0 || n > YUV_MAX_FRAMES || max_w < 1 || max_w > YUV_MAX_SIDE || max_h < 1 || max_h > YUV_MAX_SIDE ||
      !(formats & 15u) || (formats & ~15u))
    return (int)hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int f = 0; f < 4; f++) { /* a missing instantiation is an error, never another format's kernel */
    if (!(formats >> f & 1u))
      continue;
    switch (f) {
    case ASCIICHAT_YUV_I420: launch_whole<ASCIICHAT_YUV_I420>(a, n, max_w, max_h, s); break;
    case ASCIICHAT_YUV_NV12: launch_whole<ASCIICHAT_YUV_NV12>(a, n, max_w, max_h, s); break;
    case ASCIICHAT_YUV_YUYV: launch_whole<ASCIICHAT_YUV_YUYV>(a, n, max_w, max_h, s); break;
    default: launch_whole<ASCIICHAT_YUV_UYVY>(a, n, max_w, max_h, s); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
      return (int)e;
  }
  return (int)hipSuccess;
}
