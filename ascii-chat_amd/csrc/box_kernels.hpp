/*
 * box_kernels.hpp -- the opt-in area-average (box filter) downscale in front of the renderers: source frame i becomes the
 * out_w x out_h RGB24 image a render target would have point-sampled, every pixel the rounded mean of its box instead.
 * NOT the reference's resize (which samples one pixel, image.c:293-325): the renderers run over the averaged image give
 * byte for byte what the reference's renderers give over that image, nothing is claimed about the source frame.
 *
 * The rule (integer, exact; achip_box_bounds on the host states the same):
 *   column box of x:  x0 = floor(x * src_w / out_w),  x1 = max(x0 + 1, floor((x + 1) * src_w / out_w));  rows alike
 *   A[y][x][c] = (S + n / 2) / n,  S the sum of channel c over the box,  n = (x1 - x0) * (y1 - y0)
 *   stored pixel (x, y) = A[flip_y ? out_h - 1 - y : y][flip_x ? out_w - 1 - x : x]
 *
 * One 256-thread workgroup per (frame, output row).  Phase 1 sums the rows of the row's box per BYTE column: a lane owns
 * fixed 16-byte groups of the source rows (g = lane, lane + 256, ...), loads them as uint4 -- a wave reads 1 KB of a row at a
 * time -- eight rows in flight per lane (32 KB per workgroup, several workgroups per CU), and adds them into packed 16-bit
 * sums: even bytes in one register, odd bytes in another, per dword.  A 16-bit sum holds 256 rows of 255, so the packed
 * sums are flushed into the LDS stage (3 * src_w words, 45 KB at 3840 pixels) every 256 rows: the first flush stores, later
 * ones add -- every column has one owner, so nothing is atomic.  The bytes of a row beyond its last whole group are summed
 * one byte per lane.  A source whose base or stride is not a multiple of 16 takes the same loop with 4-byte groups and
 * unaligned dword loads.  Nothing is read outside [src, src + (src_h - 1) * stride + 3 * src_w).
 * Phase 2, after one barrier: 3 * out_w lanes each add their box's columns at pitch 3, divide and store one byte.
 *
 * Row offsets are 64-bit (2159 rows of 11520 bytes pass 2^24: no 24-bit multiply anywhere), sums are 32-bit (an all-255
 * 3840 x 2160 frame averaged to 1 x 1 sums to 2 115 072 000; with n / 2 added still below 2^32).
 * Only plain HIP: the same source runs under the CPU emulator (tests/hipemu).
 *
 * Grid composites (box_canvas_kernel): a composite frame is averaged in two exact steps, each rounded -- every placed source
 * k to its tile T_k (tile_w x tile_h, no flips) by box_kernel into a scratch slab, then the canvas_w x canvas_h canvas, whose
 * pixel (X, Y) is T_k[Y - org_y][X - org_x] under the cell lookup of sample_composite (render_kernels.hpp) and black
 * elsewhere, to out_w x out_h by the same rule (black pixels count in n; flips mirror the result).  The canvas is never
 * stored: one 256-thread workgroup per (composite frame, stored output row) sums the canvas rows of the row's box per byte
 * column straight from the tiles.  A lane owns byte columns j = lane, lane + 256, ... < 3 * canvas_w, resolves the column's
 * cell column once, and walks the rows [y0, y1) one cell row at a time (the cell changes only at multiples of cell_h):
 * within a cell the column's bytes are 3 * tile_w apart in one tile.  Sums go to the same LDS stage (12 * canvas_w bytes,
 * one owner per column, nothing atomic); phase 2 is box_kernel's.  No division by a cell size of 0: such a canvas is black.
 */
#pragma once

#include <gfx950_ops.hpp>

#include "achip_types.h"
#include "box.h"

namespace achip {
namespace box {

constexpr uint32_t kBlock = ACHIP_BOX_BLOCK;
constexpr uint32_t kRowsInFlight = 8; /* loads a lane issues before it adds the first */
constexpr uint32_t kFlushRows = 256;  /* 256 * 255 = 65280 fits a 16-bit sum */
constexpr size_t lds_bytes(int max_src_w) { return ((size_t)12 * (size_t)max_src_w + 15u) & ~(size_t)15u; }

/* the box of output index i on one axis */
__device__ inline void bounds(uint32_t src, uint32_t out, uint32_t i, uint32_t &lo, uint32_t &hi) {
  lo = i * src / out;
  hi = max(lo + 1u, (i + 1u) * src / out);
}

template <int W> struct Group {
  uint32_t w[W];
};
template <int W> __device__ inline Group<W> load_group(const ACHIP_GLOBAL uint8_t *p);
struct alignas(16) aligned_u32x4 {
  uint32_t x, y, z, w;
};
template <> __device__ inline Group<4> load_group<4>(const ACHIP_GLOBAL uint8_t *p) { /* 16-byte aligned: one dwordx4 load */
  const ACHIP_GLOBAL aligned_u32x4 *v = reinterpret_cast<const ACHIP_GLOBAL aligned_u32x4 *>(p);
  return Group<4>{{v->x, v->y, v->z, v->w}};
}
template <> __device__ inline Group<1> load_group<1>(const ACHIP_GLOBAL uint8_t *p) { /* any address */
  return Group<1>{{reinterpret_cast<const ACHIP_GLOBAL unaligned_u32 *>(p)->v}};
}

/* sums[b] = sum over the n_rows rows at `rows` (stride bytes apart) of byte b, for b < row_bytes; W dwords per group */
template <int W> __device__ inline void column_sums(const ACHIP_GLOBAL uint8_t *rows, int64_t stride, uint32_t n_rows, uint32_t row_bytes) {
  uint32_t *sums = reinterpret_cast<uint32_t *>(ACHIP_SMEM);
  constexpr uint32_t kGroup = 4u * W;
  const uint32_t groups = row_bytes / kGroup;
  for (uint32_t g = threadIdx.x; g < groups; g += kBlock) {
    const ACHIP_GLOBAL uint8_t *col = rows + g * kGroup;
    for (uint32_t r0 = 0; r0 < n_rows; r0 += kFlushRows) {
      const uint32_t r1 = min(n_rows, r0 + kFlushRows);
      uint32_t even[W], odd[W]; /* bytes 0 and 2, 1 and 3 of each dword, 16 bits each */
#pragma unroll
      for (int j = 0; j < W; j++)
        even[j] = odd[j] = 0u;
      uint32_t r = r0;
      for (; r + kRowsInFlight <= r1; r += kRowsInFlight) {
        Group<W> v[kRowsInFlight];
#pragma unroll
        for (uint32_t k = 0; k < kRowsInFlight; k++)
          v[k] = load_group<W>(col + (int64_t)(r + k) * stride);
#pragma unroll
        for (uint32_t k = 0; k < kRowsInFlight; k++)
#pragma unroll
          for (int j = 0; j < W; j++) {
            even[j] += v[k].w[j] & 0x00FF00FFu;
            odd[j] += (v[k].w[j] >> 8) & 0x00FF00FFu;
          }
      }
      for (; r < r1; r++) {
        const Group<W> v = load_group<W>(col + (int64_t)r * stride);
#pragma unroll
        for (int j = 0; j < W; j++) {
          even[j] += v.w[j] & 0x00FF00FFu;
          odd[j] += (v.w[j] >> 8) & 0x00FF00FFu;
        }
      }
#pragma unroll
      for (int j = 0; j < W; j++) {
        uint4 *slot = reinterpret_cast<uint4 *>(sums + g * kGroup + 4u * (uint32_t)j);
        uint4 s = make_uint4(even[j] & 0xFFFFu, odd[j] & 0xFFFFu, even[j] >> 16, odd[j] >> 16);
        if (r0 != 0u) {
          const uint4 t = *slot;
          s = make_uint4(s.x + t.x, s.y + t.y, s.z + t.z, s.w + t.w);
        }
        *slot = s;
      }
    }
  }
  for (uint32_t b = groups * kGroup + threadIdx.x; b < row_bytes; b += kBlock) { /* fewer than 16 bytes */
    uint32_t s = 0u;
    for (uint32_t r = 0; r < n_rows; r++)
      s += rows[(int64_t)r * stride + b];
    sums[b] = s;
  }
}

/* workgroup b: frame b / rows_per_frame, stored row b % rows_per_frame (rows beyond the frame's out_h: nothing to do) */
__global__ void __launch_bounds__(ACHIP_BOX_BLOCK)
    box_kernel(const achip_box_desc_t *__restrict__ desc, const achip_box_uniform_t uni, const uint32_t rows_per_frame,
               uint8_t *__restrict__ images, const uint64_t pitch) {
  const uint32_t frame = blockIdx.x / rows_per_frame, y = blockIdx.x - frame * rows_per_frame;
  achip_box_desc_t d;
  if (uni.enabled) {
    d = uni.d;
    d.src += (int64_t)frame * uni.src_pitch;
  } else {
    d = desc[frame];
  }
  const uint32_t src_w = (uint32_t)d.src_w, src_h = (uint32_t)d.src_h, out_w = (uint32_t)d.out_w, out_h = (uint32_t)d.out_h;
  if (y >= out_h)
    return;
  uint32_t y0, y1;
  bounds(src_h, out_h, (d.flips & ACHIP_OP_FLIP_Y) ? out_h - 1u - y : y, y0, y1);
  const ACHIP_GLOBAL uint8_t *rows = (const ACHIP_GLOBAL uint8_t *)d.src + (int64_t)y0 * d.src_stride;
  if ((((uint64_t)(uintptr_t)d.src | (uint64_t)d.src_stride) & 15u) == 0u)
    column_sums<4>(rows, d.src_stride, y1 - y0, 3u * src_w);
  else
    column_sums<1>(rows, d.src_stride, y1 - y0, 3u * src_w);
  __syncthreads();
  const uint32_t *sums = reinterpret_cast<const uint32_t *>(ACHIP_SMEM);
  uint8_t *out = images + (uint64_t)frame * pitch + (uint64_t)y * (3u * out_w);
  for (uint32_t j = threadIdx.x; j < 3u * out_w; j += kBlock) {
    const uint32_t x = j / 3u, c = j - 3u * x;
    uint32_t x0, x1;
    bounds(src_w, out_w, (d.flips & ACHIP_OP_FLIP_X) ? out_w - 1u - x : x, x0, x1);
    uint32_t s = 0u;
    for (uint32_t k = x0; k < x1; k++)
      s += sums[3u * k + c];
    const uint32_t n = (x1 - x0) * (y1 - y0);
    out[j] = (uint8_t)((s + n / 2u) / n);
  }
}

/* workgroup b: composite frame b / rows_per_frame of the table, stored row b % rows_per_frame */
__global__ void __launch_bounds__(ACHIP_BOX_BLOCK)
    box_canvas_kernel(const achip_box_canvas_t *__restrict__ table, const uint32_t rows_per_frame, const uint8_t *__restrict__ tiles,
                      const uint64_t tile_pitch, uint8_t *__restrict__ images, const uint64_t pitch) {
  const uint32_t k = blockIdx.x / rows_per_frame, y = blockIdx.x - k * rows_per_frame;
  const achip_box_canvas_t *__restrict__ t = table + k;
  const uint32_t canvas_w = (uint32_t)t->canvas_w, canvas_h = (uint32_t)t->canvas_h, out_w = (uint32_t)t->out_w,
                 out_h = (uint32_t)t->out_h, flips = t->flips;
  if (y >= out_h)
    return;
  uint32_t y0, y1;
  bounds(canvas_h, out_h, (flips & ACHIP_OP_FLIP_Y) ? out_h - 1u - y : y, y0, y1);
  uint32_t *sums = reinterpret_cast<uint32_t *>(ACHIP_SMEM);
  const bool grid = t->cell_w > 0 && t->cell_h > 0;
  const uint32_t cell_w = (uint32_t)t->cell_w, cell_h = (uint32_t)t->cell_h, cols = (uint32_t)t->cols, rows = (uint32_t)t->rows,
                 n_src = (uint32_t)t->n_src;
  for (uint32_t j = threadIdx.x; j < 3u * canvas_w; j += kBlock) {
    const uint32_t X = j / 3u;
    uint32_t s = 0u;
    const uint32_t col = grid ? X / cell_w : cols; /* (never a division by 0) */
    if (col < cols) {
      uint32_t row = y0 / cell_h;
      for (uint32_t Y = y0; Y < y1 && row < rows; row++) {
        const uint32_t Yend = min(y1, (row + 1u) * cell_h); /* the rows of [Y, y1) in this cell row */
        const uint64_t idx = (uint64_t)row * cols + col;
        if (idx >= n_src)
          break; /* so is every later cell row */
        const achip_box_cell_t *__restrict__ cell = &t->cell[idx];
        const int32_t slot = cell->slot, lx = (int32_t)X - cell->org_x;
        if (slot >= 0 && lx >= 0 && lx < cell->tile_w) {
          const int32_t ya = max((int32_t)Y, cell->org_y), yb = min((int32_t)Yend, cell->org_y + cell->tile_h);
          const uint32_t step = 3u * (uint32_t)cell->tile_w;
          const ACHIP_GLOBAL uint8_t *p = (const ACHIP_GLOBAL uint8_t *)tiles + (uint64_t)slot * tile_pitch +
                                          (uint64_t)(uint32_t)(ya - cell->org_y) * step + (j - 3u * (uint32_t)cell->org_x);
          for (int32_t yy = ya; yy < yb; yy++, p += step)
            s += *p;
        }
        Y = Yend;
      }
    }
    sums[j] = s;
  }
  __syncthreads();
  uint8_t *out = images + (uint64_t)(uint32_t)t->frame * pitch + (uint64_t)y * (3u * out_w);
  for (uint32_t j = threadIdx.x; j < 3u * out_w; j += kBlock) {
    const uint32_t x = j / 3u, c = j - 3u * x;
    uint32_t x0, x1;
    bounds(canvas_w, out_w, (flips & ACHIP_OP_FLIP_X) ? out_w - 1u - x : x, x0, x1);
    uint32_t s = 0u;
    for (uint32_t i = x0; i < x1; i++)
      s += sums[3u * i + c];
    const uint32_t n = (x1 - x0) * (y1 - y0);
    out[j] = (uint8_t)((s + n / 2u) / n);
  }
}

} // namespace box
} // namespace achip
