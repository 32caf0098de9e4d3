/*
 * yuvbox_kernels.hpp -- YUV sources (I420, NV12, YUYV, UYVY) box-averaged to the size a render target samples, straight from
 * their planes: image i is the box average of the whole conversion of source i.  The rule is stated in
 * include/asciichat_yuvbox.h; the arithmetic (yuv_rgb) and the addressing are yuv_math.h's, the box bounds yuvbox.h's.  Every
 * pixel is converted and clamped, then summed: nothing is averaged in YUV.
 *
 * box_kernel: box_kernels.hpp's decomposition, one 256-thread workgroup per (image, stored output row), the item -- the resolved
 * source, the image's size, the flips -- uniform per workgroup (scalar loads), the format a uniform branch.  It was kept over
 * lanes that sum their own box in registers because a box is 24 columns wide at 1080p -> 80 x 24: a lane walking its own box
 * would load with a 24-byte lane pitch, where a lane per four columns loads whole lines of a row, and the sources are what the
 * pass moves.
 *   Phase 1 sums the rows [y0, y1) of the row's box per pixel column: a lane owns fixed groups of four columns
 *   (g = lane, lane + 256, ...) and keeps twelve 32-bit sums (R, G, B of four pixels) in registers.
 *     4:2:0: the rows are walked a chroma row at a time -- a head row when y0 is odd (its chroma row is shared with the box
 *     above), whole pairs, a tail row when y1 is odd (shared with the box below, or the last row of an odd height) --; a pair
 *     loads its chroma once (I420 two halfwords, NV12 one dword) and two Y dwords, and the chroma terms of yuv_rgb are common
 *     to the eight pixels (the compiler keeps them: one inlined expression, equal operands).
 *     4:2:2: 8 packed bytes of a row as two dwords.
 *   The loads are aligned where the plane's base and stride are multiples of the access, else unaligned (the hardware takes
 *   them); one choice per plane.  The sums go to the LDS stage (3 * width words, 45 KB at 3840 pixels) as three 16-byte
 *   stores per group; every column has one owner, so nothing is atomic.  The columns behind the last whole group (width % 4)
 *   are summed pixel by pixel, one lane each.  Nothing is read outside a plane's (rows - 1) * stride + row bytes.
 *   Phase 2, after one barrier, is box_kernel's: 3 * out_w lanes each add their box's columns at pitch 3, divide and store one
 *   byte.  Exactly 3 * out_w * out_h bytes of an image are stored.
 *
 * The phase-1 functions take a column range [c0, c1), c0 a multiple of four: only the groups and edge columns that touch it are
 * summed, and the stage starts at column c0 (3 * (x - c0) + c is the word of column x).  They also take the lanes that share the
 * work (Lanes: this lane's index among `count`) and their stage, and rows [y0, y1) that may be none (the stage then holds
 * zeros).  box_kernel passes the whole width, the whole workgroup and the whole box; the tile kernel of yuvboxgrid_kernels.hpp a
 * segment of a row's boxes, and where that leaves lanes idle, a slice of the box's rows per part of the workgroup.
 *
 * Row offsets are 64-bit, sums are 32-bit (an all-white 3840 x 2160 frame averaged to 1 x 1 sums to 2 115 072 000; with n / 2
 * added still below 2^32): no 16-bit partial sums, nothing to flush.  No atomics, no inline assembly, no scratch.
 * Only plain HIP and gfx950_ops.hpp: the same source runs under the CPU emulator (tests/hipemu).
 */
#pragma once

#include <gfx950_ops.hpp>

#include "yuvbox.h"

namespace achip {
namespace yuvbox {

constexpr uint32_t kBlock = YUV_BLOCK;

/* the planes of a source as global memory (pointers read out of items are generic) */
__device__ inline const ACHIP_GLOBAL uint8_t *global_of(const uint8_t *p) { return (const ACHIP_GLOBAL uint8_t *)p; }

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

/* one converted pixel (R | G << 8 | B << 16) into the three sums of its column */
__device__ inline void add_pixel(uint32_t *acc, uint32_t p) {
  acc[0] += p & 0xFFu;
  acc[1] += (p >> 8) & 0xFFu;
  acc[2] += p >> 16;
}

/* four pixels of one row, their Y in the bytes of yw, the chroma of the two pairs in u[] and v[] */
__device__ inline void add_four(uint32_t (&acc)[12], uint32_t yw, const uint32_t (&u)[2], const uint32_t (&v)[2]) {
#pragma unroll
  for (int k = 0; k < 4; k++)
    add_pixel(acc + 3 * k, yuv_rgb((yw >> (8 * k)) & 0xFFu, u[k >> 1], v[k >> 1]));
}

/* the lanes that share a range of columns and rows, and where their sums go (16-aligned LDS) */
struct Lanes {
  uint32_t lane, count; /* count >= 3: the edge columns take a lane each */
  uint32_t *stage;
};
__device__ inline Lanes whole_workgroup() { return Lanes{threadIdx.x, kBlock, reinterpret_cast<uint32_t *>(ACHIP_SMEM)}; }

/* a group's sums to the stage: columns 4 * g .. 4 * g + 3 of a stage that starts at group g = 0, three words each */
__device__ inline void stage_group(uint32_t *stage, uint32_t g, const uint32_t (&acc)[12]) {
  uint4 *slot = reinterpret_cast<uint4 *>(stage) + 3u * g;
  slot[0] = make_uint4(acc[0], acc[1], acc[2], acc[3]);
  slot[1] = make_uint4(acc[4], acc[5], acc[6], acc[7]);
  slot[2] = make_uint4(acc[8], acc[9], acc[10], acc[11]);
}

/* the columns behind the last whole group (groups = width / 4) that lie below c1, one lane each, pixel by pixel */
__device__ inline void edge_columns(const asciichat_yuv_source_t &s, uint32_t groups, uint32_t y0, uint32_t y1, uint32_t c0, uint32_t c1,
                                    const Lanes &w) {
  const uint32_t x = 4u * groups + w.lane;
  if (x >= (uint32_t)s.width || x >= c1)
    return;
  const yuv_layout_t l = yuv_layout(&s);
  uint32_t acc[3] = {0u, 0u, 0u};
  for (uint32_t r = y0; r < y1; r++)
    add_pixel(acc, yuv_rgb(global_of(l.y_plane)[yuv_at_y(&l, (int32_t)x, (int32_t)r)], global_of(l.u_plane)[yuv_at_u(&l, (int32_t)x, (int32_t)r)],
                           global_of(l.v_plane)[yuv_at_v(&l, (int32_t)x, (int32_t)r)]));
  uint32_t *sums = w.stage;
  sums[3u * (x - c0)] = acc[0], sums[3u * (x - c0) + 1u] = acc[1], sums[3u * (x - c0) + 2u] = acc[2]; /* (c0 <= 4 * groups) */
}

/* the whole groups that touch columns [c0, c1): [c0 / 4, *last) */
__device__ inline uint32_t first_group(uint32_t groups, uint32_t c0, uint32_t c1, uint32_t *last) {
  const uint32_t end = (c1 + 3u) / 4u;
  *last = end < groups ? end : groups;
  return c0 / 4u;
}

/* 4:2:0: sums[3 * (x - c0) + c] = the sum over rows [y0, y1) of channel c of the converted pixel (x, row), for the columns of
 * the groups that touch [c0, c1) (c0 a multiple of four, c0 < c1 <= width) */
template <int FORMAT> __device__ inline void planar_sums(const asciichat_yuv_source_t &s, uint32_t y0, uint32_t y1, uint32_t c0, uint32_t c1,
                                                      const Lanes &w) {
  const uint32_t groups = (uint32_t)s.width / 4u;
  uint32_t last;
  const uint32_t first = first_group(groups, c0, c1, &last);
  const ACHIP_GLOBAL uint8_t *yp = global_of(s.plane[0]);
  const ACHIP_GLOBAL uint8_t *up = global_of(s.plane[1]);
  const ACHIP_GLOBAL uint8_t *vp = global_of(s.plane[FORMAT == ASCIICHAT_YUV_I420 ? 2 : 1]);
  const int64_t ys = s.stride[0], us = s.stride[1], vs = s.stride[FORMAT == ASCIICHAT_YUV_I420 ? 2 : 1];
  const bool y_aligned = multiple_of(s.plane[0], s.stride[0], 4u);
  const bool u_aligned = multiple_of(s.plane[1], s.stride[1], FORMAT == ASCIICHAT_YUV_I420 ? 2u : 4u);
  const bool v_aligned = FORMAT == ASCIICHAT_YUV_I420 ? multiple_of(s.plane[2], s.stride[2], 2u) : u_aligned;
  for (uint32_t g = first + w.lane; g < last; g += w.count) {
    uint32_t acc[12];
#pragma unroll
    for (int k = 0; k < 12; k++)
      acc[k] = 0u;
    /* the chroma of columns 4 * g .. 4 * g + 3 in chroma row cr */
    auto chroma = [&](uint32_t cr, uint32_t (&u)[2], uint32_t (&v)[2]) {
      if (FORMAT == ASCIICHAT_YUV_I420) {
        const uint32_t uu = load_u16(up + (int64_t)cr * us + 2u * g, u_aligned), vv = load_u16(vp + (int64_t)cr * vs + 2u * g, v_aligned);
        u[0] = uu & 0xFFu, u[1] = uu >> 8, v[0] = vv & 0xFFu, v[1] = vv >> 8;
      } else {
        const uint32_t c = load_u32(up + (int64_t)cr * us + 4u * g, u_aligned);
        u[0] = c & 0xFFu, v[0] = (c >> 8) & 0xFFu, u[1] = (c >> 16) & 0xFFu, v[1] = c >> 24;
      }
    };
    auto one_row = [&](uint32_t r) { /* a row whose chroma row is shared with a neighbouring box, or the last of an odd height */
      uint32_t u[2], v[2];
      chroma(r >> 1, u, v);
      add_four(acc, load_u32(yp + (int64_t)r * ys + 4u * g, y_aligned), u, v);
    };
    uint32_t r = y0;
    if ((r & 1u) && r < y1)
      one_row(r++);
#pragma unroll 2
    for (; r + 2u <= y1; r += 2u) {
      uint32_t u[2], v[2];
      chroma(r >> 1, u, v);
      const uint32_t ya = load_u32(yp + (int64_t)r * ys + 4u * g, y_aligned), yb = load_u32(yp + (int64_t)(r + 1u) * ys + 4u * g, y_aligned);
      add_four(acc, ya, u, v);
      add_four(acc, yb, u, v);
    }
    if (r < y1)
      one_row(r);
    stage_group(w.stage, g - first, acc);
  }
  edge_columns(s, groups, y0, y1, c0, c1, w);
}

/* 4:2:2: the same sums from rows of packed pairs -- UYVY: U Y0 V Y1; YUYV: Y0 U Y1 V */
template <int FORMAT> __device__ inline void packed_sums(const asciichat_yuv_source_t &s, uint32_t y0, uint32_t y1, uint32_t c0, uint32_t c1,
                                                      const Lanes &w) {
  const uint32_t groups = (uint32_t)s.width / 4u;
  uint32_t last;
  const uint32_t first = first_group(groups, c0, c1, &last);
  const ACHIP_GLOBAL uint8_t *p0 = global_of(s.plane[0]);
  const int64_t stride = s.stride[0];
  const bool aligned = multiple_of(s.plane[0], s.stride[0], 4u);
  for (uint32_t g = first + w.lane; g < last; g += w.count) {
    uint32_t acc[12];
#pragma unroll
    for (int k = 0; k < 12; k++)
      acc[k] = 0u;
#pragma unroll 4
    for (uint32_t r = y0; r < y1; r++) {
      const ACHIP_GLOBAL uint8_t *row = p0 + (int64_t)r * stride + 8u * g;
      const uint32_t d[2] = {load_u32(row, aligned), load_u32(row + 4, aligned)};
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const uint32_t b0 = d[j] & 0xFFu, b1 = (d[j] >> 8) & 0xFFu, b2 = (d[j] >> 16) & 0xFFu, b3 = d[j] >> 24;
        if (FORMAT == ASCIICHAT_YUV_UYVY) {
          add_pixel(acc + 6 * j, yuv_rgb(b1, b0, b2));
          add_pixel(acc + 6 * j + 3, yuv_rgb(b3, b0, b2));
        } else {
          add_pixel(acc + 6 * j, yuv_rgb(b0, b1, b3));
          add_pixel(acc + 6 * j + 3, yuv_rgb(b2, b1, b3));
        }
      }
    }
    stage_group(w.stage, g - first, acc);
  }
  edge_columns(s, groups, y0, y1, c0, c1, w); /* (an even width: two columns, or none) */
}

/* the sums of columns [c0, c1) of rows [y0, y1) of a source into the stage, by its format */
__device__ inline void column_sums(const asciichat_yuv_source_t &s, uint32_t y0, uint32_t y1, uint32_t c0, uint32_t c1, const Lanes &w) {
  switch (s.format) { /* a format outside the four stores nothing defined: the host refuses it */
  case ASCIICHAT_YUV_I420: planar_sums<ASCIICHAT_YUV_I420>(s, y0, y1, c0, c1, w); break;
  case ASCIICHAT_YUV_NV12: planar_sums<ASCIICHAT_YUV_NV12>(s, y0, y1, c0, c1, w); break;
  case ASCIICHAT_YUV_YUYV: packed_sums<ASCIICHAT_YUV_YUYV>(s, y0, y1, c0, c1, w); break;
  default: packed_sums<ASCIICHAT_YUV_UYVY>(s, y0, y1, c0, c1, w); break;
  }
}

/* workgroup b: image b / rows_per_image, stored row b % rows_per_image (rows beyond the image's out_h: nothing to do).
 * items == NULL: the one image of `one` */
__global__ void __launch_bounds__(YUV_BLOCK)
    box_kernel(const yuvbox_item_t *__restrict__ items, const yuvbox_item_t one, const uint32_t rows_per_image, uint8_t *__restrict__ images,
               const uint64_t pitch) {
  const uint32_t image = blockIdx.x / rows_per_image, y = blockIdx.x - image * rows_per_image;
  yuvbox_item_t it;
  if (items)
    it = items[image];
  else
    it = one;
  const uint32_t src_w = (uint32_t)it.src.width, src_h = (uint32_t)it.src.height, out_w = (uint32_t)it.out_w, out_h = (uint32_t)it.out_h;
  if (y >= out_h)
    return;
  uint32_t y0, y1;
  yuvbox_bounds(src_h, out_h, (it.flips & ACHIP_OP_FLIP_Y) ? out_h - 1u - y : y, &y0, &y1);
  column_sums(it.src, y0, y1, 0u, src_w, whole_workgroup());
  __syncthreads();
  const uint32_t *sums = reinterpret_cast<const uint32_t *>(ACHIP_SMEM);
  uint8_t *out = images + (uint64_t)image * pitch + (uint64_t)y * (3u * out_w);
  for (uint32_t j = threadIdx.x; j < 3u * out_w; j += kBlock) {
    const uint32_t x = j / 3u, c = j - 3u * x;
    uint32_t x0, x1;
    yuvbox_bounds(src_w, out_w, (it.flips & ACHIP_OP_FLIP_X) ? out_w - 1u - x : x, &x0, &x1);
    uint32_t s = 0u;
    for (uint32_t k = x0; k < x1; k++)
      s += sums[3u * k + c];
    const uint32_t n = (x1 - x0) * (y1 - y0);
    out[j] = (uint8_t)((s + n / 2u) / n);
  }
}

} // namespace yuvbox
} // namespace achip
