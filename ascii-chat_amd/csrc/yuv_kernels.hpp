/*
 * yuv_kernels.hpp -- YUV sources (I420, NV12, YUYV, UYVY) to RGB24 on the device; the rule and the layouts are stated in
 * include/asciichat_yuv.h, the arithmetic and the addressing are yuv_math.h's.
 *
 * sample_kernel: only the pixels a render target samples.  Grid (groups, frame): the descriptor and the source are uniform
 * per workgroup (scalar loads).  A lane owns four consecutive pixels of the image's linear order -- they may straddle an image
 * row: one division per lane, then a carry per pixel --, gathers their Y, U and V, converts, and stores 12 bytes as three
 * dwords (slots are 16-aligned by contract, 12 * lane keeps that to 4); the last lane of an image whose pixel count is no
 * multiple of four stores its bytes singly.  Lanes behind the image leave.  The stores are plain: the render that follows reads
 * the images from the L2.  No LDS, no scratch.
 *
 * whole_kernel<FORMAT>: every pixel.  Grid (64-lane columns, 4-lane rows, image): no division.  4:2:0: a lane owns a 4 x 2 pixel
 * block, so a chroma sample is read once -- two Y dwords, two chroma halfwords (I420) or one dword (NV12).  4:2:2: a lane owns
 * 4 x 1 pixels, 8 packed bytes as two dwords.  The loads are aligned where the plane's base and stride are multiples of the
 * access, else unaligned (the hardware takes them); one choice per plane.  Each image row of a block goes out as 12 bytes: three
 * dwords where that row's address is a multiple of 4, else twelve bytes -- one choice per image row --, non-temporal (written
 * once, never read back here).  Blocks at a right edge with w % 4 != 0, and the last row of an odd-height planar image, go out
 * pixel by pixel.  Nothing is read outside a plane's (rows - 1) * stride + row bytes, nothing stored outside 3 * w bytes of a
 * row.  A workgroup whose image has another format leaves: the launcher runs one instantiation per format of a set.
 *
 * Row offsets are 64-bit.  Only plain HIP and gfx950_ops.hpp: the same source runs under the CPU emulator (tests/hipemu).
 */
#pragma once

#include <gfx950_ops.hpp>

#include "yuv.h"

namespace achip {
namespace yuv {

/* the planes of a layout as global memory (pointers read out of descriptors are generic) */
__device__ inline const ACHIP_GLOBAL uint8_t *global_of(const uint8_t *p) { return (const ACHIP_GLOBAL uint8_t *)p; }

/* pixel (sx, sy) of a layout, converted: R | G << 8 | B << 16 */
__device__ inline uint32_t pixel(const yuv_layout_t &l, int32_t sx, int32_t sy) {
  return yuv_rgb(global_of(l.y_plane)[yuv_at_y(&l, sx, sy)], global_of(l.u_plane)[yuv_at_u(&l, sx, sy)],
                 global_of(l.v_plane)[yuv_at_v(&l, sx, sy)]);
}

__global__ void __launch_bounds__(YUV_BLOCK)
    sample_kernel(const asciichat_yuv_source_t *__restrict__ sources, const achip_frame_t *__restrict__ frames, uint8_t *__restrict__ images,
                  const uint64_t pitch) {
  const uint32_t fi = blockIdx.y;
  const achip_frame_t f = frames[fi];
  const asciichat_yuv_source_t s = sources[fi];
  const uint32_t out_w = (uint32_t)f.out_w, total = out_w * (uint32_t)f.out_h;
  const uint32_t p0 = 4u * (blockIdx.x * YUV_BLOCK + threadIdx.x);
  if (p0 >= total)
    return;
  const yuv_layout_t l = yuv_layout(&s);
  uint32_t y = p0 / out_w, x = p0 - y * out_w;
  uint32_t px[4];
#pragma unroll
  for (int k = 0; k < 4; k++) { /* (a pixel behind the image samples row out_h: clamped into the source like any other, never stored) */
    int32_t sx, sy;
    yuv_sample_at(&f, (int32_t)x, (int32_t)y, &sx, &sy);
    px[k] = pixel(l, sx, sy);
    if (++x == out_w)
      x = 0u, y++;
  }
  uint8_t *out = images + (uint64_t)fi * pitch + 3ull * p0;
  if (p0 + 4u <= total) {
    uint32_t *o = reinterpret_cast<uint32_t *>(out);
    o[0] = px[0] | px[1] << 24;
    o[1] = px[1] >> 8 | px[2] << 16;
    o[2] = px[2] >> 16 | px[3] << 8;
  } else {
    for (uint32_t k = 0; k < total - p0; k++) {
      out[3u * k + 0u] = (uint8_t)px[k];
      out[3u * k + 1u] = (uint8_t)(px[k] >> 8);
      out[3u * k + 2u] = (uint8_t)(px[k] >> 16);
    }
  }
}

/* the one place that says how the bytes of a whole image leave: T at an address aligned to T */
template <typename T> __device__ inline void store_rgb(uint8_t *p, T v) {
#if ACHIP_EMULATED || defined(ACHIP_NO_NT_STORE)
  *reinterpret_cast<T *>(p) = v;
#else
  __builtin_nontemporal_store(v, reinterpret_cast<T *>(p));
#endif
}

struct __attribute__((packed)) unaligned_u16 {
  uint16_t v;
};
__device__ inline uint32_t load_u32(const ACHIP_GLOBAL uint8_t *p, bool aligned) {
  return aligned ? *reinterpret_cast<const ACHIP_GLOBAL uint32_t *>(p) : reinterpret_cast<const ACHIP_GLOBAL unaligned_u32 *>(p)->v;
}
__device__ inline uint32_t load_u16(const ACHIP_GLOBAL uint8_t *p, bool aligned) {
  return aligned ? *reinterpret_cast<const ACHIP_GLOBAL uint16_t *>(p) : reinterpret_cast<const ACHIP_GLOBAL unaligned_u16 *>(p)->v;
}
__device__ inline bool multiple_of(const uint8_t *base, int32_t stride, uint32_t n) {
  return (((uint64_t)(uintptr_t)base | (uint64_t)(uint32_t)stride) & (n - 1u)) == 0u;
}

/* four pixels of one image row, 12 bytes at `out` */
__device__ inline void store_four(uint8_t *out, bool row_aligned, const uint32_t px[4]) {
  const uint32_t w0 = px[0] | px[1] << 24, w1 = px[1] >> 8 | px[2] << 16, w2 = px[2] >> 16 | px[3] << 8;
  if (row_aligned) {
    store_rgb<uint32_t>(out, w0);
    store_rgb<uint32_t>(out + 4, w1);
    store_rgb<uint32_t>(out + 8, w2);
  } else {
    const uint32_t w[3] = {w0, w1, w2};
#pragma unroll
    for (int j = 0; j < 12; j++)
      store_rgb<uint8_t>(out + j, (uint8_t)(w[j >> 2] >> (8 * (j & 3))));
  }
}

template <int FORMAT> __global__ void __launch_bounds__(YUV_BLOCK) whole_kernel(const yuv_whole_args_t a) {
  constexpr bool kPlanar = FORMAT == ASCIICHAT_YUV_I420 || FORMAT == ASCIICHAT_YUV_NV12;
  constexpr uint32_t kRows = kPlanar ? 2u : 1u;
  const uint32_t fi = blockIdx.z;
  asciichat_yuv_source_t s;
  if (a.sources)
    s = a.sources[fi];
  else
    s = a.one;
  if (s.format != FORMAT)
    return;
  const uint32_t w = (uint32_t)s.width, h = (uint32_t)s.height;
  const uint32_t bx = blockIdx.x * YUV_WHOLE_LANES_X + (threadIdx.x % YUV_WHOLE_LANES_X);
  const uint32_t by = blockIdx.y * YUV_WHOLE_LANES_Y + (threadIdx.x / YUV_WHOLE_LANES_X);
  const uint32_t x0 = 4u * bx, y0 = kRows * by;
  if (x0 >= w || y0 >= h)
    return;
  const uint64_t row_bytes = a.rgb_stride ? (uint64_t)(uint32_t)a.rgb_stride : 3ull * w;
  uint8_t *image = a.rgb + (uint64_t)fi * a.pitch;
  if (x0 + 4u > w || y0 + kRows > h) { /* a right edge, or the last row of an odd height: pixel by pixel */
    const yuv_layout_t l = yuv_layout(&s);
    for (uint32_t y = y0; y < min(h, y0 + kRows); y++)
      for (uint32_t x = x0; x < min(w, x0 + 4u); x++) {
        const uint32_t p = pixel(l, (int32_t)x, (int32_t)y);
        uint8_t *out = image + (uint64_t)y * row_bytes + 3u * x;
        store_rgb<uint8_t>(out, (uint8_t)p);
        store_rgb<uint8_t>(out + 1, (uint8_t)(p >> 8));
        store_rgb<uint8_t>(out + 2, (uint8_t)(p >> 16));
      }
    return;
  }
  const ACHIP_GLOBAL uint8_t *p0 = global_of(s.plane[0]);
  uint32_t px[kRows][4];
  if (kPlanar) {
    const bool y_aligned = multiple_of(s.plane[0], s.stride[0], 4u);
    uint32_t yw[2], u[2], v[2];
    yw[0] = load_u32(p0 + (int64_t)y0 * s.stride[0] + x0, y_aligned);
    yw[1] = load_u32(p0 + (int64_t)(y0 + 1u) * s.stride[0] + x0, y_aligned);
    if (FORMAT == ASCIICHAT_YUV_I420) {
      const uint32_t uu = load_u16(global_of(s.plane[1]) + (int64_t)by * s.stride[1] + 2u * bx, multiple_of(s.plane[1], s.stride[1], 2u));
      const uint32_t vv = load_u16(global_of(s.plane[2]) + (int64_t)by * s.stride[2] + 2u * bx, multiple_of(s.plane[2], s.stride[2], 2u));
      u[0] = uu & 0xFFu, u[1] = uu >> 8, v[0] = vv & 0xFFu, v[1] = vv >> 8;
    } else {
      const uint32_t c = load_u32(global_of(s.plane[1]) + (int64_t)by * s.stride[1] + 4u * bx, multiple_of(s.plane[1], s.stride[1], 4u));
      u[0] = c & 0xFFu, v[0] = (c >> 8) & 0xFFu, u[1] = (c >> 16) & 0xFFu, v[1] = c >> 24;
    }
#pragma unroll
    for (uint32_t r = 0; r < kRows; r++)
#pragma unroll
      for (int k = 0; k < 4; k++)
        px[r][k] = yuv_rgb((yw[r] >> (8 * k)) & 0xFFu, u[k >> 1], v[k >> 1]);
  } else {
    const bool aligned = multiple_of(s.plane[0], s.stride[0], 4u);
    const ACHIP_GLOBAL uint8_t *row = p0 + (int64_t)y0 * s.stride[0] + 8u * bx;
    const uint32_t d[2] = {load_u32(row, aligned), load_u32(row + 4, aligned)};
#pragma unroll
    for (int j = 0; j < 2; j++) { /* UYVY: U Y0 V Y1; YUYV: Y0 U Y1 V */
      const uint32_t b0 = d[j] & 0xFFu, b1 = (d[j] >> 8) & 0xFFu, b2 = (d[j] >> 16) & 0xFFu, b3 = d[j] >> 24;
      if (FORMAT == ASCIICHAT_YUV_UYVY) {
        px[0][2 * j] = yuv_rgb(b1, b0, b2);
        px[0][2 * j + 1] = yuv_rgb(b3, b0, b2);
      } else {
        px[0][2 * j] = yuv_rgb(b0, b1, b3);
        px[0][2 * j + 1] = yuv_rgb(b2, b1, b3);
      }
    }
  }
#pragma unroll
  for (uint32_t r = 0; r < kRows; r++) {
    uint8_t *row = image + (uint64_t)(y0 + r) * row_bytes;
    store_four(row + 12u * bx, ((uint64_t)(uintptr_t)row & 3u) == 0u, px[r]);
  }
}

} // namespace yuv
} // namespace achip
