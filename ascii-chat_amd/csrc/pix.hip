/* pix.hip -- the launchers of libasciichat_pix.so (pix_kernels.hpp); the host side is pix.c. */
#include <hip/hip_runtime.h>

#include "pix.h"
#include "pix_kernels.hpp"

extern "C" int pix_launch_sample(const asciichat_pix_source_t *sources, const achip_frame_t *frames, int n, uint32_t max_pixels,
                                 uint8_t *images, uint64_t pitch, void *stream) {
  if (!sources || !frames || n <= 0 || n > PIX_MAX_FRAMES || max_pixels == 0u || !images)
    return (int)hipErrorInvalidValue;
  const unsigned lanes = (max_pixels + 3u) / 4u, groups = (lanes + PIX_BLOCK - 1u) / PIX_BLOCK;
  hipLaunchKernelGGL(achip::pix::sample_kernel, dim3(groups, (unsigned)n), dim3(PIX_BLOCK), 0, static_cast<hipStream_t>(stream), sources,
                     frames, images, pitch);
  return (int)hipGetLastError();
}

template <int BPP> static void launch_whole(const pix_whole_args_t *a, int n, int max_w, int max_h, hipStream_t s) {
  const unsigned bw = ((unsigned)max_w + PIX_WHOLE_PIXELS - 1u) / PIX_WHOLE_PIXELS;
  const dim3 grid((bw + PIX_WHOLE_LANES_X - 1u) / PIX_WHOLE_LANES_X, ((unsigned)max_h + PIX_WHOLE_LANES_Y - 1u) / PIX_WHOLE_LANES_Y, (unsigned)n);
  hipLaunchKernelGGL((achip::pix::whole_kernel<BPP>), grid, dim3(PIX_BLOCK), 0, s, *a);
}

extern "C" int pix_launch_whole(const pix_whole_args_t *a, int n, int max_w, int max_h, unsigned bpps, void *stream) {
  if (!a || !a->rgb || n <= 0 || n > PIX_MAX_FRAMES || max_w < 1 || max_w > PIX_MAX_SIDE || max_h < 1 || max_h > PIX_MAX_SIDE || !(bpps & 3u) ||
      (bpps & ~3u))
    return (int)hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int b = 0; b < 2; b++) { /* a missing instantiation is an error, never the other bpp's kernel */
    if (!(bpps >> b & 1u))
      continue;
    if (b == 0)
      launch_whole<3>(a, n, max_w, max_h, s);
    else
      launch_whole<4>(a, n, max_w, max_h, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
      return (int)e;
  }
  return (int)hipSuccess;
}

extern "C" int pix_launch_box(const pix_box_args_t *a, int n, int max_src_w, void *stream) {
  if (!a || (!a->sources && n != 1) || (a->sources && !a->frames) || n <= 0 || n > PIX_MAX_FRAMES || !a->images || a->rows_per_image == 0u ||
      a->rows_per_image > PIX_BOX_MAX_OUT || max_src_w <= 0 || max_src_w > PIX_BOX_MAX_SRC_W ||
      (uint64_t)n * (uint64_t)a->rows_per_image > 0x7FFFFFFFull)
    return (int)hipErrorInvalidValue;
  /* (the stage of the widest source is 46 080 bytes: below the 48 KB a launch may ask for without saying so first) */
  hipLaunchKernelGGL(achip::pix::box_kernel, dim3((unsigned)n * a->rows_per_image), dim3(PIX_BLOCK), pix_box_lds_bytes(max_src_w),
                     static_cast<hipStream_t>(stream), *a);
  return (int)hipGetLastError();
}
