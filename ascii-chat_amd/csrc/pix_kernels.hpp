/*
 * pix_kernels.hpp -- packed RGB sources (RGB24, RGBA, BGR24, BGRA) to RGB24 on the device; the rule and the layouts are stated in
 * include/asciichat_pix.h, the addressing, the permutation and the box bounds are pix_math.h's.  A format is a uniform fact of
 * a workgroup everywhere below: its bytes per pixel pick the loads, its channel order is a UNIFORM BRANCH (not a template
 * parameter: the swap is three bit operations per pixel, and a mixed tick stays one launch per bpp).
 *
 * sample_kernel: only the pixels a render target samples.  Grid (groups, frame): the descriptor and the source are uniform per
 * workgroup (scalar loads).  A lane owns four consecutive pixels of the image's linear order -- they may straddle an image row:
 * one division per lane, then a carry per pixel --, gathers them, permutes, and stores 12 bytes as three dwords (slots are
 * 16-aligned by contract, 12 * lane keeps that to 4); the last lane of an image whose pixel count is no multiple of four stores
 * its bytes singly.  A 4-byte format loads one dword per pixel, aligned where base and stride are multiples of 4, else as four
 * unaligned bytes in one access (the hardware takes them); a 3-byte format loads three bytes.  Lanes behind the image leave.
 * The stores are plain: the render that follows reads the images from the L2.  No LDS.
 *
 * whole_kernel<BPP>: every pixel, the streaming path.  Grid (64-lane columns, 4-lane rows, image): no division.  A lane owns a
 * run of PIX_WHOLE_PIXELS consecutive pixels of one row (pix.h: 4 or 16).  A run wholly inside the row whose bytes are a
 * multiple of 16 is loaded as 16-byte words where base and stride are multiples of 16; every other run group by group (four
 * pixels: BPP dwords), aligned where base and stride are multiples of 4, else unaligned -- one choice per source.  The
 * permutation happens in registers (RGB24 in, RGB24 out: the words pass as they are).  Each group goes out as 12 bytes: a run of
 * 16 pixels as three 16-byte stores where the destination is a multiple of 16, else three dwords a group where the image row's
 * address is a multiple of 4, else twelve bytes -- one choice per image row --, non-temporal (written once, never read back
 * here).  The pixels behind the last whole group of a row (w % 4) go pixel by pixel.  Nothing is read outside a source's
 * (height - 1) * stride + BPP * width bytes, nothing stored outside 3 * w bytes of a row.  A workgroup whose source has the
 * other bpp leaves: the launcher runs one instantiation per bpp of a set.
 *
 * box_kernel: yuvbox_kernels.hpp's decomposition, one 256-thread workgroup per (image, stored output row), the source and the
 * image's size and flips uniform per workgroup.
 *   Phase 1 sums the rows [y0, y1) of the row's box per pixel column: a lane owns fixed groups of four columns
 *   (g = lane, lane + 256, ...) and keeps twelve 32-bit sums in registers, in memory order; per row it loads 16 bytes (4-byte
 *   formats: one 16-byte word where base and stride are multiples of 16, else four dwords) or 12 (3-byte formats: three
 *   dwords), aligned to 4 or not as above.  A blue-first group swaps its first and third sums once, behind the rows.  The sums
 *   go to the LDS stage (3 * width words, 45 KB at 3840 pixels) as three 16-byte stores per group; every column has one owner,
 *   so nothing is atomic.  The columns behind the last whole group (width % 4) are summed pixel by pixel, one lane each.
 *   Phase 2, after one barrier, is box_kernels.hpp's text (restated: it is the body of that kernel, not a function of its
 *   header): 3 * out_w lanes each add their box's columns at pitch 3, divide and store one byte.  Exactly 3 * out_w * out_h
 *   bytes of an image are stored.
 *   Phase 1 (column_sums) also takes a column range [c0, c1), c0 a multiple of four -- only the groups and edge columns that
 *   touch it are summed, and the stage starts at column c0 --, the lanes that share the work and their stage (Lanes), and rows
 *   that may be none: pixgrid_kernels.hpp's averaged tile kernel calls it with a segment of a row's boxes and a slice of the
 *   box's rows.  box_kernel passes the whole width, the whole workgroup and the whole box.
 *
 * Row offsets are 64-bit, sums are 32-bit (an all-white 3840 x 2160 frame averaged to 1 x 1 sums to 2 115 072 000; with n / 2
 * added still below 2^32): no 16-bit partial sums, nothing to flush.  No atomics, no inline assembly, no scratch, and only
 * vector stores.  Only plain HIP and gfx950_ops.hpp: the same source runs under the CPU emulator (tests/hipemu).
 */
#pragma once

#include <gfx950_ops.hpp>

#include "pix.h"

namespace achip {
namespace pix {

constexpr uint32_t kBlock = PIX_BLOCK;

/* the pixels of a source as global memory (pointers read out of descriptors are generic) */
__device__ inline const ACHIP_GLOBAL uint8_t *global_of(const uint8_t *p) { return (const ACHIP_GLOBAL uint8_t *)p; }

__device__ inline uint32_t load_u32(const ACHIP_GLOBAL uint8_t *p, bool aligned) {
  return aligned ? *reinterpret_cast<const ACHIP_GLOBAL uint32_t *>(p) : reinterpret_cast<const ACHIP_GLOBAL unaligned_u32 *>(p)->v;
}
struct alignas(16) aligned_u32x4 {
  uint32_t x, y, z, w;
};
/* 16 bytes at a multiple of 16: one dwordx4 load */
__device__ inline void load_u32x4(const ACHIP_GLOBAL uint8_t *p, uint32_t *d) {
  const ACHIP_GLOBAL aligned_u32x4 *v = reinterpret_cast<const ACHIP_GLOBAL aligned_u32x4 *>(p);
  d[0] = v->x, d[1] = v->y, d[2] = v->z, d[3] = v->w;
}
__device__ inline bool multiple_of(const uint8_t *base, int32_t stride, uint32_t n) {
  return (((uint64_t)(uintptr_t)base | (uint64_t)(uint32_t)stride) & (n - 1u)) == 0u;
}

/* pixel (sx, sy) of a resolved source, R | G << 8 | B << 16; bpp4, swapped and aligned4 are the source's, uniform */
__device__ inline uint32_t pixel(const asciichat_pix_source_t &s, bool bpp4, bool swapped, bool aligned4, int32_t sx, int32_t sy) {
  const ACHIP_GLOBAL uint8_t *p = global_of(s.pixels) + pix_at(s.stride, bpp4 ? 4 : 3, sx, sy);
  if (bpp4)
    return pix_word_rgb(load_u32(p, aligned4), swapped);
  return pix_bytes_rgb(p[0], p[1], p[2], swapped);
}

__global__ void __launch_bounds__(PIX_BLOCK)
    sample_kernel(const asciichat_pix_source_t *__restrict__ sources, const achip_frame_t *__restrict__ frames, uint8_t *__restrict__ images,
                  const uint64_t pitch) {
  const uint32_t fi = blockIdx.y;
  const achip_frame_t f = frames[fi];
  const asciichat_pix_source_t s = sources[fi];
  const uint32_t out_w = (uint32_t)f.out_w, total = out_w * (uint32_t)f.out_h;
  const uint32_t p0 = 4u * (blockIdx.x * kBlock + threadIdx.x);
  if (p0 >= total)
    return;
  const bool bpp4 = pix_bpp(s.format) == 4, swapped = pix_swapped(s.format) != 0, aligned4 = multiple_of(s.pixels, s.stride, 4u);
  uint32_t y = p0 / out_w, x = p0 - y * out_w;
  uint32_t px[4];
#pragma unroll
  for (int k = 0; k < 4; k++) { /* (a pixel behind the image samples row out_h: clamped into the source like any other, never stored) */
    int32_t sx, sy;
    pix_sample_at(&f, (int32_t)x, (int32_t)y, &sx, &sy);
    px[k] = pixel(s, bpp4, swapped, aligned4, sx, sy);
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

/* four pixels of a group (the BPP dwords at d) as the three words of their RGB24 bytes */
template <int BPP> __device__ inline void permute_group(const uint32_t *d, bool swapped, uint32_t *o) {
  uint32_t px[4];
  if (BPP == 4) {
#pragma unroll
    for (int k = 0; k < 4; k++)
      px[k] = pix_word_rgb(d[k], swapped);
  } else {
    if (!swapped) { /* RGB24 in, RGB24 out */
      o[0] = d[0], o[1] = d[1], o[2] = d[2];
      return;
    }
    px[0] = pix_word_rgb(d[0], 1);
    px[1] = pix_word_rgb(d[0] >> 24 | d[1] << 8, 1);
    px[2] = pix_word_rgb(d[1] >> 16 | d[2] << 16, 1);
    px[3] = pix_word_rgb(d[2] >> 8, 1);
  }
  o[0] = px[0] | px[1] << 24;
  o[1] = px[1] >> 8 | px[2] << 16;
  o[2] = px[2] >> 16 | px[3] << 8;
}

template <int BPP> __global__ void __launch_bounds__(PIX_BLOCK) whole_kernel(const pix_whole_args_t a) {
  constexpr uint32_t kRun = PIX_WHOLE_PIXELS, kGroups = kRun / 4u, kWords = kGroups * BPP; /* a group of four pixels is BPP dwords */
  static_assert(kRun == 4u || kRun == 16u, "a lane's run is 4 or 16 pixels");
  const uint32_t fi = blockIdx.z;
  asciichat_pix_source_t s;
  if (a.sources)
    s = a.sources[fi];
  else
    s = a.one;
  if (pix_bpp(s.format) != BPP)
    return;
  const bool swapped = pix_swapped(s.format) != 0;
  const uint32_t w = (uint32_t)s.width, h = (uint32_t)s.height;
  const uint32_t bx = blockIdx.x * PIX_WHOLE_LANES_X + (threadIdx.x % PIX_WHOLE_LANES_X);
  const uint32_t y = blockIdx.y * PIX_WHOLE_LANES_Y + (threadIdx.x / PIX_WHOLE_LANES_X);
  const uint32_t x0 = kRun * bx;
  if (x0 >= w || y >= h)
    return;
  const uint64_t row_bytes = a.rgb_stride ? (uint64_t)(uint32_t)a.rgb_stride : 3ull * w;
  uint8_t *out_row = a.rgb + (uint64_t)fi * a.pitch + (uint64_t)y * row_bytes;
  uint8_t *out = out_row + 3u * x0;
  const ACHIP_GLOBAL uint8_t *in_row = global_of(s.pixels) + (int64_t)y * s.stride;
  const ACHIP_GLOBAL uint8_t *in = in_row + (uint32_t)BPP * x0;
  const bool in4 = multiple_of(s.pixels, s.stride, 4u), in16 = multiple_of(s.pixels, s.stride, 16u);
  const uint32_t full = min(kGroups, (w - x0) / 4u); /* the whole groups of this run */
  uint32_t d[kWords], o[3u * kGroups];
  if (kWords % 4u == 0u && full == kGroups && in16) { /* (BPP * kRun bytes a lane: the run starts at a multiple of 16 too) */
#pragma unroll
    for (uint32_t j = 0; j < kWords / 4u; j++)
      load_u32x4(in + 16u * j, d + 4u * j);
  } else {
#pragma unroll
    for (uint32_t g = 0; g < kGroups; g++)
      if (g < full) {
#pragma unroll
        for (uint32_t j = 0; j < (uint32_t)BPP; j++)
          d[g * BPP + j] = load_u32(in + 4u * (g * BPP + j), in4);
      }
  }
#pragma unroll
  for (uint32_t g = 0; g < kGroups; g++)
    if (g < full)
      permute_group<BPP>(d + g * BPP, swapped, o + 3u * g);
  if (kGroups == 4u && full == kGroups && ((uint64_t)(uintptr_t)out & 15u) == 0u) {
#pragma unroll
    for (uint32_t j = 0; j < 3u * kGroups / 4u; j++)
      store_u4_nt(out + 16u * j, make_uint4(o[4u * j], o[4u * j + 1u], o[4u * j + 2u], o[4u * j + 3u]));
  } else if (((uint64_t)(uintptr_t)out_row & 3u) == 0u) { /* (12 bytes a group keep the row's alignment to 4) */
#pragma unroll
    for (uint32_t g = 0; g < kGroups; g++)
      if (g < full) {
        store_rgb<uint32_t>(out + 12u * g, o[3u * g]);
        store_rgb<uint32_t>(out + 12u * g + 4u, o[3u * g + 1u]);
        store_rgb<uint32_t>(out + 12u * g + 8u, o[3u * g + 2u]);
      }
  } else {
#pragma unroll
    for (uint32_t g = 0; g < kGroups; g++)
      if (g < full) {
#pragma unroll
        for (uint32_t j = 0; j < 12u; j++)
          store_rgb<uint8_t>(out + 12u * g + j, (uint8_t)(o[3u * g + (j >> 2)] >> (8u * (j & 3u))));
      }
  }
  if (full < kGroups) /* the row ends inside this run: its last w % 4 pixels, one by one */
    for (uint32_t x = x0 + 4u * full; x < w; x++) {
      const ACHIP_GLOBAL uint8_t *p = in_row + (uint32_t)BPP * x;
      const uint32_t v = pix_bytes_rgb(p[0], p[1], p[2], swapped);
      uint8_t *q = out_row + 3u * x;
      store_rgb<uint8_t>(q, (uint8_t)v);
      store_rgb<uint8_t>(q + 1, (uint8_t)(v >> 8));
      store_rgb<uint8_t>(q + 2, (uint8_t)(v >> 16));
    }
}

/* the lanes that share a range of columns and rows, and where their sums go (16-aligned LDS) */
struct Lanes {
  uint32_t lane, count; /* count >= 3: the columns behind the last whole group take a lane each */
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

/* stage[3 * (x - c0) + c] = the sum over rows [y0, y1) of channel c of the RGB24 value of pixel (x, row), for the columns x of
 * the groups that touch [c0, c1) (c0 a multiple of four, c0 < c1 <= width), shared among the lanes of `l`; rows that are none
 * stage zeros.  box_kernel passes the whole width, the whole workgroup and the whole box (the overload below); the averaged tile
 * kernel of pixgrid_kernels.hpp a segment of a row's boxes, and where that leaves lanes idle, a slice of the box's rows per part
 * of the workgroup. */
template <int BPP>
__device__ inline void column_sums(const asciichat_pix_source_t &s, uint32_t y0, uint32_t y1, uint32_t c0, uint32_t c1, const Lanes &l) {
  uint32_t *stage = l.stage;
  const uint32_t w = (uint32_t)s.width, groups = w / 4u;
  const uint32_t first = c0 / 4u, end = (c1 + 3u) / 4u, last = end < groups ? end : groups; /* the whole groups that touch [c0, c1) */
  const ACHIP_GLOBAL uint8_t *base = global_of(s.pixels);
  const int64_t stride = s.stride;
  const bool swapped = pix_swapped(s.format) != 0;
  const bool in4 = multiple_of(s.pixels, s.stride, 4u), in16 = multiple_of(s.pixels, s.stride, 16u);
  for (uint32_t g = first + l.lane; g < last; g += l.count) {
    uint32_t acc[12]; /* in memory order: a blue-first group is turned round once, below */
#pragma unroll
    for (int k = 0; k < 12; k++)
      acc[k] = 0u;
    const ACHIP_GLOBAL uint8_t *col = base + 4u * (uint32_t)BPP * g;
#pragma unroll 4
    for (uint32_t r = y0; r < y1; r++) {
      const ACHIP_GLOBAL uint8_t *p = col + (int64_t)r * stride;
      uint32_t d[4];
      if (BPP == 4 && in16) {
        load_u32x4(p, d);
      } else {
#pragma unroll
        for (int j = 0; j < BPP; j++)
          d[j] = load_u32(p + 4 * j, in4);
      }
      if (BPP == 4) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
          acc[3 * k] += d[k] & 0xFFu;
          acc[3 * k + 1] += (d[k] >> 8) & 0xFFu;
          acc[3 * k + 2] += (d[k] >> 16) & 0xFFu;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 12; j++)
          acc[j] += (d[j >> 2] >> (8 * (j & 3))) & 0xFFu;
      }
    }
    if (swapped) {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t t = acc[3 * k];
        acc[3 * k] = acc[3 * k + 2];
        acc[3 * k + 2] = t;
      }
    }
    stage_group(stage, g - first, acc);
  }
  const uint32_t x = 4u * groups + l.lane; /* the columns behind the last whole group that lie below c1, one lane each */
  if (x < w && x < c1) {
    uint32_t acc[3] = {0u, 0u, 0u};
    for (uint32_t r = y0; r < y1; r++) {
      const ACHIP_GLOBAL uint8_t *p = base + pix_at(stride, BPP, (int32_t)x, (int32_t)r);
      const uint32_t v = pix_bytes_rgb(p[0], p[1], p[2], swapped);
      acc[0] += v & 0xFFu, acc[1] += (v >> 8) & 0xFFu, acc[2] += v >> 16;
    }
    stage[3u * (x - c0)] = acc[0], stage[3u * (x - c0) + 1u] = acc[1], stage[3u * (x - c0) + 2u] = acc[2]; /* (c0 <= 4 * groups) */
  }
}

/* every column of the source, by the whole workgroup: stage[3 * x + c] */
template <int BPP> __device__ inline void column_sums(const asciichat_pix_source_t &s, uint32_t y0, uint32_t y1) {
  column_sums<BPP>(s, y0, y1, 0u, (uint32_t)s.width, whole_workgroup());
}

/* workgroup b: image b / rows_per_image, stored row b % rows_per_image (rows beyond the image's out_h: nothing to do) */
__global__ void __launch_bounds__(PIX_BLOCK) box_kernel(const pix_box_args_t a) {
  const uint32_t image = blockIdx.x / a.rows_per_image, y = blockIdx.x - image * a.rows_per_image;
  asciichat_pix_source_t s;
  uint32_t out_w, out_h, flips;
  if (a.sources) {
    s = a.sources[image];
    out_w = (uint32_t)a.frames[image].out_w, out_h = (uint32_t)a.frames[image].out_h, flips = a.frames[image].ops;
  } else {
    s = a.one;
    out_w = (uint32_t)a.one_w, out_h = (uint32_t)a.one_h, flips = a.one_flips;
  }
  if (y >= out_h)
    return;
  const uint32_t src_w = (uint32_t)s.width, src_h = (uint32_t)s.height;
  uint32_t y0, y1;
  pix_bounds(src_h, out_h, (flips & ACHIP_OP_FLIP_Y) ? out_h - 1u - y : y, &y0, &y1);
  if (pix_bpp(s.format) == 4)
    column_sums<4>(s, y0, y1);
  else
    column_sums<3>(s, y0, y1);
  __syncthreads();
  const uint32_t *sums = reinterpret_cast<const uint32_t *>(ACHIP_SMEM);
  uint8_t *out = a.images + (uint64_t)image * a.pitch + (uint64_t)y * (3u * out_w);
  for (uint32_t j = threadIdx.x; j < 3u * out_w; j += kBlock) {
    const uint32_t x = j / 3u, c = j - 3u * x;
    uint32_t x0, x1;
    pix_bounds(src_w, out_w, (flips & ACHIP_OP_FLIP_X) ? out_w - 1u - x : x, &x0, &x1);
    uint32_t sum = 0u;
    for (uint32_t k = x0; k < x1; k++)
      sum += sums[3u * k + c];
    const uint32_t n = (x1 - x0) * (y1 - y0);
    out[j] = (uint8_t)((sum + n / 2u) / n);
  }
}

} // namespace pix
} // namespace achip
