/* yuvbox_emu_driver.cpp -- the kernel of libasciichat_yuvbox.so (ascii-chat_amd/csrc/yuvbox_kernels.hpp) under the fiber
 * emulator, from sources and descriptors as yuvbox.c takes them -- checked and staged by yuvbox.h's own text -- and launched as
 * yuvbox.hip launches it; beside it the checks and the host walk of the rule (yuvbox.h) as they stand, and the launcher yuvbox.c
 * calls when the tests link it against the mock HIP runtime.  TESTS ONLY. */
#include "yuvbox_kernels.hpp"

#include <algorithm>
#include <vector>

/* the launcher of yuvbox.hip on the emulator: also what yuvbox.c calls when the tests link it against the mock HIP runtime
 * (tests/mockhip/mock_hip.c), where device memory is host memory */
extern "C" int yuvbox_launch(const yuvbox_item_t *items, const yuvbox_item_t *one, int n, int max_out_h, int max_src_w, uint8_t *images,
                             uint64_t pitch, void *) {
  if ((!items && (!one || n != 1)) || n <= 0 || n > YUV_MAX_FRAMES || !images || max_out_h <= 0 || max_out_h > YUVBOX_MAX_OUT || max_src_w <= 0 ||
      max_src_w > YUVBOX_MAX_SRC_W || (uint64_t)n * (uint64_t)max_out_h > 0x7FFFFFFFull)
    return 1; /* hipErrorInvalidValue */
  yuvbox_item_t by_value;
  memset(&by_value, 0, sizeof(by_value));
  if (!items)
    by_value = *one;
  hipemu::launch(dim3((unsigned)n * (unsigned)max_out_h), dim3(YUV_BLOCK), yuvbox_lds_bytes(max_src_w),
                 [&] { achip::yuvbox::box_kernel(items, by_value, (uint32_t)max_out_h, images, pitch); });
  return 0;
}

/* what the host decides about a set: 0 taken, 1 refused (why receives the reason) */
extern "C" int emu_yuvbox_set_check(const asciichat_yuv_source_t *sources, const achip_frame_t *frames, int n, int max_frames, int *bad,
                                    int *unsupported, const char **why) {
  const char *w = yuvbox_set_check(sources, frames, n, max_frames, bad, unsupported);
  if (why)
    *why = w;
  return w ? 1 : 0;
}

/* create(max_frames) + set(sources, frames, n) + run(images, pitch), or with host != 0 the host walk of yuvbox.h in the
 * kernel's place.  -1: the set is refused, -2: run refuses its arguments */
extern "C" int emu_yuvbox_run(const asciichat_yuv_source_t *sources, const achip_frame_t *frames, int n, int max_frames, uint8_t *images,
                              uint64_t pitch, int host) {
  if (yuvbox_set_check(sources, frames, n, max_frames, nullptr, nullptr))
    return -1;
  std::vector<yuvbox_item_t> items((size_t)n);
  int max_out_h = 0, max_src_w = 0;
  uint64_t max_bytes = 0;
  for (int i = 0; i < n; i++) {
    items[(size_t)i] = yuvbox_item(&sources[i], frames[i].out_w, frames[i].out_h, frames[i].ops);
    max_out_h = std::max(max_out_h, (int)frames[i].out_h);
    max_src_w = std::max(max_src_w, (int)sources[i].width);
    max_bytes = std::max<uint64_t>(max_bytes, 3ull * (uint64_t)frames[i].out_w * (uint64_t)frames[i].out_h);
  }
  if (!images || ((uintptr_t)images & 15u) || (pitch & 15u) || pitch < max_bytes)
    return -2;
  if (host) {
    for (int i = 0; i < n; i++)
      yuvbox_host_image(&items[(size_t)i], images + (uint64_t)i * pitch);
    return 0;
  }
  return yuvbox_launch(items.data(), nullptr, n, max_out_h, max_src_w, images, pitch, nullptr) ? -3 : 0;
}

/* downscale(src, dst, dst_w, dst_h, flip_x, flip_y) */
extern "C" int emu_yuvbox_downscale(const asciichat_yuv_source_t *src, uint8_t *dst, int dst_w, int dst_h, int flip_x, int flip_y) {
  if (yuvbox_source_check(src))
    return -1;
  if (!dst || dst_w < 1 || dst_h < 1 || dst_w > YUVBOX_MAX_OUT || dst_h > YUVBOX_MAX_OUT)
    return -2;
  const yuvbox_item_t one = yuvbox_item(src, dst_w, dst_h, (flip_x ? ACHIP_OP_FLIP_X : 0u) | (flip_y ? ACHIP_OP_FLIP_Y : 0u));
  return yuvbox_launch(nullptr, &one, 1, dst_h, src->width, dst, 0, nullptr) ? -3 : 0;
}
