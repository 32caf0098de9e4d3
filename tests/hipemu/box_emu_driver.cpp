/* box_emu_driver.cpp -- the area-average downscale kernel (ascii-chat_amd/csrc/box_kernels.hpp) under the fiber emulator, from
 * render descriptors as box.c takes them and launched as box.hip launches it.  TESTS ONLY. */
#include "box_kernels.hpp"

#include <vector>

/* frames[i] -> images + i * pitch.  Returns 1 when the batch went in its uniform form (descriptor in the kernel arguments;
 * the array the kernel is then given is NULL), 0 for the descriptor array, or -(refusal) of the first frame box.h refuses. */
extern "C" int emu_box(const achip_frame_t *frames, int n, uint8_t *images, uint64_t pitch, int allow_uniform) {
  std::vector<achip_box_desc_t> d((size_t)n);
  int max_out_h = 0, max_src_w = 0;
  for (int i = 0; i < n; i++) {
    const int rc = achip_box_desc_from_frame(&frames[i], &d[(size_t)i]);
    if (rc != ACHIP_BOX_OK)
      return -rc;
    max_out_h = std::max(max_out_h, (int)d[(size_t)i].out_h);
    max_src_w = std::max(max_src_w, (int)d[(size_t)i].src_w);
  }
  achip_box_uniform_t uni;
  if (!achip_box_uniform(d.data(), n, &uni) || !allow_uniform)
    memset(&uni, 0, sizeof(uni));
  const achip_box_desc_t *arr = uni.enabled ? nullptr : d.data();
  hipemu::launch(dim3((unsigned)n * (unsigned)max_out_h), dim3(ACHIP_BOX_BLOCK), achip::box::lds_bytes(max_src_w), [&] {
    achip::box::box_kernel(arr, uni, (uint32_t)max_out_h, images, pitch);
  });
  return (int)uni.enabled;
}
