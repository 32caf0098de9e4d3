/* yuv_emu_driver.cpp -- the kernels of libasciichat_yuv.so (ascii-chat_amd/csrc/yuv_kernels.hpp) under the fiber emulator, from
 * sources and descriptors as yuv.c takes them -- checked and resolved by yuv_math.h's own text -- and launched as yuv.hip
 * launches them; beside them the arithmetic and the checks of yuv_math.h as they stand.  TESTS ONLY. */
#include "yuv_kernels.hpp"

#include <vector>

extern "C" uint32_t emu_yuv_rgb(uint32_t Y, uint32_t U, uint32_t V) { return yuv_rgb(Y, U, V); }

/* every (Y, U, V): out[3 * (Y << 16 | U << 8 | V) + c] */
extern "C" void emu_yuv_rgb_all(uint8_t *out) {
  for (uint32_t i = 0; i < (1u << 24); i++) {
    const uint32_t p = yuv_rgb(i >> 16, (i >> 8) & 0xFFu, i & 0xFFu);
    out[3u * i] = (uint8_t)p, out[3u * i + 1u] = (uint8_t)(p >> 8), out[3u * i + 2u] = (uint8_t)(p >> 16);
  }
}

/* what the host decides: 0 taken, 1 refused (why receives the reason) */
extern "C" int emu_yuv_source_check(const asciichat_yuv_source_t *s, const char **why) {
  const char *w = yuv_source_check(s);
  if (why)
    *why = w;
  return w ? 1 : 0;
}
extern "C" int emu_yuv_frames_check(const asciichat_yuv_source_t *sources, const achip_frame_t *frames, int n, int max_frames, int *bad,
                                    int *unsupported, const char **why) {
  const char *w = yuv_frames_check(sources, frames, n, max_frames, bad, unsupported);
  if (why)
    *why = w;
  return w ? 1 : 0;
}

/* the host addressing: pixel (sx, sy) of a checked source */
extern "C" uint32_t emu_yuv_host_pixel(const asciichat_yuv_source_t *s, int sx, int sy) {
  const asciichat_yuv_source_t r = yuv_source_resolved(s);
  const yuv_layout_t l = yuv_layout(&r);
  return yuv_pixel(&l, sx, sy);
}

/* the set as the handle stages it: n resolved sources, then n descriptors */
static std::vector<uint8_t> staged(const asciichat_yuv_source_t *sources, const achip_frame_t *frames, int n) {
  std::vector<uint8_t> block(yuv_set_bytes(n));
  asciichat_yuv_source_t *s = reinterpret_cast<asciichat_yuv_source_t *>(block.data());
  for (int i = 0; i < n; i++)
    s[i] = yuv_source_resolved(&sources[i]);
  if (frames)
    memcpy(block.data() + yuv_set_at_frames(n), frames, (size_t)n * sizeof(achip_frame_t));
  return block;
}

/* create(max_frames) + set(sources, frames, n) + run(images, pitch).  -1: the set is refused, -2: run refuses its arguments */
extern "C" int emu_yuv_run(const asciichat_yuv_source_t *sources, const achip_frame_t *frames, int n, int max_frames, uint8_t *images,
                           uint64_t pitch) {
  if (!frames || yuv_frames_check(sources, frames, n, max_frames, nullptr, nullptr))
    return -1;
  uint32_t max_pixels = 0u;
  for (int i = 0; i < n; i++)
    max_pixels = std::max(max_pixels, (uint32_t)frames[i].out_w * (uint32_t)frames[i].out_h);
  if (!images || ((uintptr_t)images & 15u) || (pitch & 15u) || pitch < 3ull * max_pixels)
    return -2;
  const std::vector<uint8_t> block = staged(sources, frames, n);
  const asciichat_yuv_source_t *s = reinterpret_cast<const asciichat_yuv_source_t *>(block.data());
  const achip_frame_t *f = reinterpret_cast<const achip_frame_t *>(block.data() + yuv_set_at_frames(n));
  const unsigned lanes = (max_pixels + 3u) / 4u, groups = (lanes + YUV_BLOCK - 1u) / YUV_BLOCK;
  hipemu::launch(dim3(groups, (unsigned)n), dim3(YUV_BLOCK), 0, [&] { achip::yuv::sample_kernel(s, f, images, pitch); });
  return 0;
}

template <int FORMAT> static void launch_whole(const yuv_whole_args_t &a, int n, int max_w, int max_h) {
  const unsigned rows = (FORMAT == ASCIICHAT_YUV_I420 || FORMAT == ASCIICHAT_YUV_NV12) ? 2u : 1u;
  const unsigned bw = ((unsigned)max_w + 3u) / 4u, bh = ((unsigned)max_h + rows - 1u) / rows;
  hipemu::launch(dim3((bw + YUV_WHOLE_LANES_X - 1u) / YUV_WHOLE_LANES_X, (bh + YUV_WHOLE_LANES_Y - 1u) / YUV_WHOLE_LANES_Y, (unsigned)n),
                 dim3(YUV_BLOCK), 0, [&] { achip::yuv::whole_kernel<FORMAT>(a); });
}

static void launch_whole_formats(const yuv_whole_args_t &a, int n, int max_w, int max_h, unsigned formats) {
  if (formats & 1u)
    launch_whole<ASCIICHAT_YUV_I420>(a, n, max_w, max_h);
  if (formats & 2u)
    launch_whole<ASCIICHAT_YUV_NV12>(a, n, max_w, max_h);
  if (formats & 4u)
    launch_whole<ASCIICHAT_YUV_YUYV>(a, n, max_w, max_h);
  if (formats & 8u)
    launch_whole<ASCIICHAT_YUV_UYVY>(a, n, max_w, max_h);
}

/* create + set(sources, NULL, n) + run_whole(rgb, pitch) */
extern "C" int emu_yuv_run_whole(const asciichat_yuv_source_t *sources, int n, int max_frames, uint8_t *rgb, uint64_t pitch) {
  if (yuv_frames_check(sources, nullptr, n, max_frames, nullptr, nullptr))
    return -1;
  unsigned formats = 0u;
  int max_w = 0, max_h = 0;
  uint64_t need = 0;
  for (int i = 0; i < n; i++) {
    formats |= 1u << sources[i].format;
    max_w = std::max(max_w, sources[i].width), max_h = std::max(max_h, sources[i].height);
    need = std::max<uint64_t>(need, 3ull * (uint64_t)sources[i].width * (uint64_t)sources[i].height);
  }
  if (!rgb || pitch < need)
    return -2;
  const std::vector<uint8_t> block = staged(sources, nullptr, n);
  yuv_whole_args_t a;
  memset(&a, 0, sizeof(a));
  a.sources = reinterpret_cast<const asciichat_yuv_source_t *>(block.data());
  a.rgb = rgb, a.pitch = pitch;
  launch_whole_formats(a, n, max_w, max_h, formats);
  return 0;
}

/* convert(src, rgb, rgb_stride) */
extern "C" int emu_yuv_convert(const asciichat_yuv_source_t *src, uint8_t *rgb, int rgb_stride) {
  if (yuv_source_check(src))
    return -1;
  if (!rgb || (rgb_stride != 0 && (rgb_stride < 3 * src->width || rgb_stride >= YUV_MAX_STRIDE)))
    return -2;
  yuv_whole_args_t a;
  memset(&a, 0, sizeof(a));
  a.one = yuv_source_resolved(src);
  a.rgb = rgb, a.rgb_stride = rgb_stride;
  launch_whole_formats(a, 1, src->width, src->height, 1u << src->format);
  return 0;
}
