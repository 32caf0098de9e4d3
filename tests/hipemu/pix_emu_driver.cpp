/* pix_emu_driver.cpp -- the kernels of libasciichat_pix.so (ascii-chat_amd/csrc/pix_kernels.hpp) under the fiber emulator, from
 * sources and descriptors as pix.c takes them -- checked and resolved by pix_math.h's own text -- and launched as pix.hip
 * launches them; beside them the checks, the box bounds and the host walks of the rule (pix.h) as they stand, and the launchers
 * pix.c calls when the tests link it against the mock HIP runtime.  TESTS ONLY. */
#include "pix_kernels.hpp"

#include <algorithm>
#include <vector>

/* ---- the launchers of pix.hip on the emulator: also what pix.c calls when the tests link it against the mock HIP runtime
 * (tests/mockhip/mock_hip.c), where device memory is host memory ---- */
extern "C" int pix_launch_sample(const asciichat_pix_source_t *sources, const achip_frame_t *frames, int n, uint32_t max_pixels,
                                 uint8_t *images, uint64_t pitch, void *) {
  if (!sources || !frames || n <= 0 || n > PIX_MAX_FRAMES || max_pixels == 0u || !images)
    return 1; /* hipErrorInvalidValue */
  const unsigned lanes = (max_pixels + 3u) / 4u, groups = (lanes + PIX_BLOCK - 1u) / PIX_BLOCK;
  hipemu::launch(dim3(groups, (unsigned)n), dim3(PIX_BLOCK), 0, [&] { achip::pix::sample_kernel(sources, frames, images, pitch); });
  return 0;
}

template <int BPP> static void launch_whole(const pix_whole_args_t &a, int n, int max_w, int max_h) {
  const unsigned bw = ((unsigned)max_w + PIX_WHOLE_PIXELS - 1u) / PIX_WHOLE_PIXELS;
  hipemu::launch(dim3((bw + PIX_WHOLE_LANES_X - 1u) / PIX_WHOLE_LANES_X, ((unsigned)max_h + PIX_WHOLE_LANES_Y - 1u) / PIX_WHOLE_LANES_Y, (unsigned)n),
                 dim3(PIX_BLOCK), 0, [&] { achip::pix::whole_kernel<BPP>(a); });
}

extern "C" int pix_launch_whole(const pix_whole_args_t *a, int n, int max_w, int max_h, unsigned bpps, void *) {
  if (!a || !a->rgb || n <= 0 || n > PIX_MAX_FRAMES || max_w < 1 || max_w > PIX_MAX_SIDE || max_h < 1 || max_h > PIX_MAX_SIDE || !(bpps & 3u) ||
      (bpps & ~3u))
    return 1;
  if (bpps & 1u)
    launch_whole<3>(*a, n, max_w, max_h);
  if (bpps & 2u)
    launch_whole<4>(*a, n, max_w, max_h);
  return 0;
}

extern "C" int pix_launch_box(const pix_box_args_t *a, int n, int max_src_w, void *) {
  if (!a || (!a->sources && n != 1) || (a->sources && !a->frames) || n <= 0 || n > PIX_MAX_FRAMES || !a->images || a->rows_per_image == 0u ||
      a->rows_per_image > PIX_BOX_MAX_OUT || max_src_w <= 0 || max_src_w > PIX_BOX_MAX_SRC_W ||
      (uint64_t)n * (uint64_t)a->rows_per_image > 0x7FFFFFFFull)
    return 1;
  const pix_box_args_t by_value = *a;
  hipemu::launch(dim3((unsigned)n * a->rows_per_image), dim3(PIX_BLOCK), pix_box_lds_bytes(max_src_w), [&] { achip::pix::box_kernel(by_value); });
  return 0;
}

/* ---- pix_math.h as it stands ---- */
extern "C" int emu_pix_whole_pixels(void) { return PIX_WHOLE_PIXELS; }
extern "C" void emu_pix_bounds(uint32_t src, uint32_t out, uint32_t i, uint32_t *lo, uint32_t *hi) { pix_bounds(src, out, i, lo, hi); }
/* what the host decides: 0 taken, 1 refused (why receives the reason) */
extern "C" int emu_pix_source_check(const asciichat_pix_source_t *s, const char **why) {
  const char *w = pix_source_check(s);
  if (why)
    *why = w;
  return w ? 1 : 0;
}
extern "C" int emu_pix_set_check(const asciichat_pix_source_t *sources, const achip_frame_t *frames, int n, int max_frames, int *bad,
                                 int *unsupported, const char **why) {
  const char *w = pix_set_check(sources, frames, n, max_frames, bad, unsupported);
  if (why)
    *why = w;
  return w ? 1 : 0;
}

/* the set as the handle stages it: n resolved sources, then n descriptors */
static std::vector<uint8_t> staged(const asciichat_pix_source_t *sources, const achip_frame_t *frames, int n) {
  std::vector<uint8_t> block(pix_set_bytes(n));
  asciichat_pix_source_t *s = reinterpret_cast<asciichat_pix_source_t *>(block.data());
  for (int i = 0; i < n; i++)
    s[i] = pix_source_resolved(&sources[i]);
  if (frames)
    memcpy(block.data() + pix_set_at_frames(n), frames, (size_t)n * sizeof(achip_frame_t));
  return block;
}

/* create(max_frames) + set(sources, frames, n) + run (box == 0) or run_box (box != 0) into (images, pitch); with host != 0 the
 * host walk of pix.h in the kernel's place.  -1: the set is refused, -2: run refuses its arguments, -4: run_box does not
 * support the set */
extern "C" int emu_pix_run(const asciichat_pix_source_t *sources, const achip_frame_t *frames, int n, int max_frames, uint8_t *images,
                           uint64_t pitch, int box, int host) {
  if (!frames || pix_set_check(sources, frames, n, max_frames, nullptr, nullptr))
    return -1;
  uint32_t max_pixels = 0u;
  int max_out_h = 0, max_w = 0;
  for (int i = 0; i < n; i++) {
    max_pixels = std::max(max_pixels, (uint32_t)frames[i].out_w * (uint32_t)frames[i].out_h);
    max_out_h = std::max(max_out_h, (int)frames[i].out_h);
    max_w = std::max(max_w, (int)sources[i].width);
  }
  if (!images || ((uintptr_t)images & 15u) || (pitch & 15u) || pitch < 3ull * max_pixels)
    return -2;
  if (box && !pix_set_boxable(sources, frames, n))
    return -4;
  const std::vector<uint8_t> block = staged(sources, frames, n);
  const asciichat_pix_source_t *s = reinterpret_cast<const asciichat_pix_source_t *>(block.data());
  const achip_frame_t *f = reinterpret_cast<const achip_frame_t *>(block.data() + pix_set_at_frames(n));
  if (host) {
    for (int i = 0; i < n; i++) {
      if (box)
        pix_host_box(&s[i], f[i].out_w, f[i].out_h, f[i].ops, images + (uint64_t)i * pitch);
      else
        pix_host_sample(&s[i], &f[i], images + (uint64_t)i * pitch);
    }
    return 0;
  }
  if (!box)
    return pix_launch_sample(s, f, n, max_pixels, images, pitch, nullptr) ? -3 : 0;
  pix_box_args_t a;
  memset(&a, 0, sizeof(a));
  a.sources = s, a.frames = f;
  a.rows_per_image = (uint32_t)max_out_h;
  a.images = images, a.pitch = pitch;
  return pix_launch_box(&a, n, max_w, nullptr) ? -3 : 0;
}

/* create + set(sources, NULL, n) + run_whole(rgb, pitch), or the host walk */
extern "C" int emu_pix_run_whole(const asciichat_pix_source_t *sources, int n, int max_frames, uint8_t *rgb, uint64_t pitch, int host) {
  if (pix_set_check(sources, nullptr, n, max_frames, nullptr, nullptr))
    return -1;
  unsigned bpps = 0u;
  int max_w = 0, max_h = 0;
  uint64_t need = 0;
  for (int i = 0; i < n; i++) {
    bpps |= 1u << (sources[i].format & 1);
    max_w = std::max(max_w, (int)sources[i].width), max_h = std::max(max_h, (int)sources[i].height);
    need = std::max<uint64_t>(need, 3ull * (uint64_t)sources[i].width * (uint64_t)sources[i].height);
  }
  if (!rgb || pitch < need)
    return -2;
  const std::vector<uint8_t> block = staged(sources, nullptr, n);
  const asciichat_pix_source_t *s = reinterpret_cast<const asciichat_pix_source_t *>(block.data());
  if (host) {
    for (int i = 0; i < n; i++)
      pix_host_whole(&s[i], rgb + (uint64_t)i * pitch, 3u * (size_t)s[i].width);
    return 0;
  }
  pix_whole_args_t a;
  memset(&a, 0, sizeof(a));
  a.sources = s;
  a.rgb = rgb, a.pitch = pitch;
  return pix_launch_whole(&a, n, max_w, max_h, bpps, nullptr) ? -3 : 0;
}

/* convert(src, rgb, rgb_stride) */
extern "C" int emu_pix_convert(const asciichat_pix_source_t *src, uint8_t *rgb, int rgb_stride) {
  if (pix_source_check(src))
    return -1;
  if (!rgb || (rgb_stride != 0 && (rgb_stride < 3 * src->width || rgb_stride >= PIX_MAX_STRIDE)))
    return -2;
  pix_whole_args_t a;
  memset(&a, 0, sizeof(a));
  a.one = pix_source_resolved(src);
  a.rgb = rgb, a.rgb_stride = rgb_stride;
  return pix_launch_whole(&a, 1, src->width, src->height, 1u << (src->format & 1), nullptr) ? -3 : 0;
}

/* downscale(src, dst, dst_w, dst_h, flip_x, flip_y) */
extern "C" int emu_pix_downscale(const asciichat_pix_source_t *src, uint8_t *dst, int dst_w, int dst_h, int flip_x, int flip_y) {
  if (pix_source_check(src) || !pix_source_boxable(src))
    return -1;
  if (!dst || dst_w < 1 || dst_h < 1 || dst_w > PIX_BOX_MAX_OUT || dst_h > PIX_BOX_MAX_OUT)
    return -2;
  pix_box_args_t a;
  memset(&a, 0, sizeof(a));
  a.one = pix_source_resolved(src);
  a.one_w = dst_w, a.one_h = dst_h;
  a.one_flips = (flip_x ? ACHIP_OP_FLIP_X : 0u) | (flip_y ? ACHIP_OP_FLIP_Y : 0u);
  a.rows_per_image = (uint32_t)dst_h;
  a.images = dst;
  return pix_launch_box(&a, 1, src->width, nullptr) ? -3 : 0;
}
