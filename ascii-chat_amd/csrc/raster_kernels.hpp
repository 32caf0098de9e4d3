/*
 * raster_kernels.hpp -- rendered ANSI frames to RGBA pixels (include/asciichat_raster.h has the grammar and the compositing
 * rule; tests/raster_ref.py restates both against the reference's terminal.c).  Four launches per batch:
 *
 *   starts   one workgroup per frame: a newline count-and-scan gives the byte at which each of the first `rows` text rows and
 *            the text behind them begins.
 *   parse    one WAVE per text row (plus one per frame for the text behind the grid, which yields flags only).  The row is
 *            staged through LDS RASTER_CHUNK bytes at a time, one dword per lane; per 64 bytes a ballot marks the printable
 *            ASCII bytes.  A run of those in the ground state is written as cells by its lanes at once; every other byte
 *            steps a wave-uniform state machine (ESC, CSI parameters with the SGR rules applied to a shadow pen that a final
 *            'm' commits, UTF-8 continuation), so a token may straddle any chunk boundary.  The pen crosses rows: a cell
 *            written before the row's first fg- (bg-) setting parameter carries RASTER_INHERIT_FG (_BG), and the row records
 *            its exit pen per channel.  Cells never written become blank.
 *   resolve  per 32 cell rows: the entry pen of a row is the exit pen of the nearest earlier row that set the channel, else
 *            the default; marked cells take it.  The frame's status is the OR of its rows' flags.
 *   draw     the hot path, pure write.  One workgroup per (frame, cell row) walks tiles of 64 x 16 bytes of the image rows; a
 *            lane owns the 4 pixels of one 16-byte ALIGNED group of the output (a row may begin 0..3 pixels into its first
 *            group, by the image's address) and stores it as one vector; the groups at a row's ends, when partial, go out as
 *            dwords.  The tile's cells, their right and lower neighbours, with their glyphs' rectangles, sit in LDS, and so
 *            does the coverage atlas when it is at most RASTER_ATLAS_LDS bytes.  A pixel shows its last writer in row-major
 *            cell order: down-right, down, down-left, right, own glyph, own background.
 *
 * (f a + b (255 - a)) / 255 is exact as (v * 0x8081) >> 23 for v <= 65535; v <= 65025 here.
 * Only plain HIP and gfx950_ops.hpp: the same source runs under the CPU emulator (tests/hipemu).
 */
#pragma once

#include <gfx950_ops.hpp>

#include "raster.h"

namespace achip {
namespace raster {

constexpr uint32_t kBlock = RASTER_BLOCK;

/* ---- starts ----------------------------------------------------------------------------------------------------------- */

__device__ inline uint32_t frame_len(const uint32_t *__restrict__ len, uint32_t f, uint64_t stride) {
  const uint32_t n = len[f];
  return (n == ACHIP_LEN_OVERFLOW || (uint64_t)n > stride) ? 0u : n;
}

/* bit j: byte j of the dword is '\n' (exact per byte) */
__device__ inline uint32_t newline_bits(uint32_t w) {
  const uint32_t x = w ^ 0x0A0A0A0Au;
  const uint32_t t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
  return ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u);
}

/* starts[f][0] = 0; starts[f][k + 1] = the byte behind the k-th newline for k < rows, len + 1 where there is none */
__global__ void __launch_bounds__(RASTER_BLOCK)
    starts_kernel(const raster_params_t p, const uint8_t *__restrict__ frames, const uint64_t stride, const uint32_t *__restrict__ len,
                  uint32_t *__restrict__ starts) {
  const uint32_t f = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n = frame_len(len, f, stride), R = (uint32_t)p.rows;
  const uint8_t *__restrict__ src = frames + (uint64_t)f * stride;
  uint32_t *__restrict__ st = starts + (uint64_t)f * (R + 2u);
  uint32_t *wsum = reinterpret_cast<uint32_t *>(ACHIP_SMEM);
  const bool aligned = ((uint64_t)(uintptr_t)src & 15u) == 0u;
  if (tid == 0u)
    st[0] = 0u;
  uint32_t base = 0u; /* newlines before this pass */
  for (uint32_t pos0 = 0u; pos0 < n && base < R; pos0 += kBlock * 16u) {
    const uint32_t my = pos0 + tid * 16u;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (aligned && my + 16u <= n) {
      const uint4 v = *reinterpret_cast<const uint4 *>(src + my);
      w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
      for (uint32_t j = 0u; j < 16u; j++)
        if (my + j < n)
          w[j >> 2] |= (uint32_t)src[my + j] << (8u * (j & 3u));
    }
    uint32_t mask = newline_bits(w[0]) | newline_bits(w[1]) << 4 | newline_bits(w[2]) << 8 | newline_bits(w[3]) << 12;
    const uint32_t cnt = (uint32_t)__popcll((uint64_t)mask);
    const uint32_t incl = wave_inclusive_scan(cnt);
    if (lane == 63u)
      wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
    for (uint32_t k = 0u; k < kBlock / 64u; k++) {
      const uint32_t s = wsum[k];
      before += k < wave ? s : 0u;
      total += s;
    }
    uint32_t k = base + before + incl - cnt;
    while (mask) {
      const uint32_t j = (uint32_t)__ffs((int)mask) - 1u;
      mask &= mask - 1u;
      if (k < R)
        st[k + 1u] = my + j + 1u;
      k++;
    }
    __syncthreads();
    base += total;
  }
  for (uint32_t k = min(base, R) + 1u + tid; k <= R + 1u; k += kBlock)
    st[k] = n + 1u;
}

/* ---- parse ------------------------------------------------------------------------------------------------------------- */

enum : uint32_t { S_GROUND = 0, S_ESC, S_CSI_PARAM, S_CSI_INTERM, S_UTF8 };
enum : uint32_t { M_TOP = 0, M_SELECT, M_R, M_G, M_B, M_INDEX };

struct Pen {
  uint32_t fg, bg;
  bool fg_in, bg_in; /* still the row's entry pen: inherited */
};

struct RowParser {
  /* what the row is */
  const raster_params_t *p;
  const uint32_t *cps; /* LDS: the atlas' codepoints */
  raster_cell_t *row;  /* the row's cells; unused in the tail */
  uint32_t cols;
  bool tail;
  uint32_t lane;
  /* where it stands */
  uint32_t col, hi, flags, last_cp;
  bool has_last;
  Pen pen;
  uint32_t state;
  /* a control sequence in progress */
  uint32_t cur, npar, first_val, mode, acc_r, acc_g;
  bool cur_empty, nondigit, interm, target_fg, shadow_unknown;
  Pen shadow;
  /* a UTF-8 sequence in progress */
  uint32_t u_len, u_rem, u_cp;

  __device__ uint32_t lookup(uint32_t cp) const {
    if (cp == 0u || cp == 0x20u)
      return RASTER_NO_GLYPH;
    if (p->matrix_map && cp >= 32u && cp <= 126u)
      cp = 0xE900u + (cp - 32u) % 27u;
    uint32_t lo = 0u, hi_ = (uint32_t)p->n_glyphs;
    while (lo < hi_) {
      const uint32_t mid = (lo + hi_) >> 1;
      const uint32_t c = cps[mid];
      if (c == cp)
        return mid;
      if (c < cp)
        lo = mid + 1u;
      else
        hi_ = mid;
    }
    return RASTER_NO_GLYPH;
  }
  __device__ void store(uint32_t c, uint32_t slot) const {
    raster_cell_t v;
    v.slot = slot | (pen.fg_in ? RASTER_INHERIT_FG : 0u) | (pen.bg_in ? RASTER_INHERIT_BG : 0u);
    v.fg = pen.fg;
    v.bg = pen.bg;
    row[c] = v;
  }
  /* `count` times the codepoint cp from the current column (uniform): the lanes share the cells */
  __device__ void put(uint32_t cp, uint32_t count) {
    last_cp = cp;
    has_last = true;
    if (tail) {
      flags |= ASCIICHAT_RASTER_OVERFLOW_ROWS;
      return;
    }
    const uint32_t room = cols - col, take = min(count, room);
    if (count > room)
      flags |= ASCIICHAT_RASTER_OVERFLOW_COLS;
    if (take) {
      const uint32_t slot = lookup(cp);
      for (uint32_t c = col + lane; c < col + take; c += 64u)
        store(c, slot);
    }
    col += take;
    hi = max(hi, col);
  }
  __device__ void set_colour(Pen &q, bool fg, uint32_t rgb) const {
    if (fg)
      q.fg = rgb, q.fg_in = false;
    else
      q.bg = rgb, q.bg_in = false;
  }
  /* one SGR parameter, left to right, onto the shadow pen */
  __device__ void sgr(uint32_t v) {
    switch (mode) {
    case M_TOP:
      if (v == 0u) {
        set_colour(shadow, true, p->default_fg);
        set_colour(shadow, false, p->default_bg);
      } else if (v == 38u || v == 48u) {
        target_fg = v == 38u;
        mode = M_SELECT;
      } else if ((v >= 30u && v <= 37u) || (v >= 90u && v <= 97u)) {
        set_colour(shadow, true, p->lut[v < 90u ? v - 30u : v - 90u + 8u]);
      } else if ((v >= 40u && v <= 47u) || (v >= 100u && v <= 107u)) {
        set_colour(shadow, false, p->lut[256u + (v < 100u ? v - 40u : v - 100u + 8u)]);
      } else if (v == 39u) {
        set_colour(shadow, true, p->default_fg);
      } else if (v == 49u) {
        set_colour(shadow, false, p->default_bg);
      } else {
        shadow_unknown = true;
      }
      break;
    case M_SELECT:
      mode = v == 2u ? M_R : v == 5u ? M_INDEX : M_TOP;
      if (mode == M_TOP)
        shadow_unknown = true;
      break;
    case M_R:
      acc_r = v;
      mode = M_G;
      break;
    case M_G:
      acc_g = v;
      mode = M_B;
      break;
    case M_B:
      if (acc_r <= 255u && acc_g <= 255u && v <= 255u)
        set_colour(shadow, target_fg, acc_r << 16 | acc_g << 8 | v);
      else
        shadow_unknown = true;
      mode = M_TOP;
      break;
    default: /* M_INDEX */
      if (v <= 255u)
        set_colour(shadow, target_fg, p->lut[(target_fg ? 0u : 256u) + v]);
      else
        shadow_unknown = true;
      mode = M_TOP;
      break;
    }
  }
  __device__ void end_param() {
    const uint32_t v = cur_empty ? 0u : cur;
    if (npar == 0u)
      first_val = v;
    npar++;
    sgr(v);
    cur = 0u;
    cur_empty = true;
  }
  __device__ void final_byte(uint32_t b) {
    end_param();
    state = S_GROUND;
    if (b == 0x6Du && !interm && !nondigit) { /* SGR */
      pen = shadow;
      if (shadow_unknown || mode != M_TOP)
        flags |= ASCIICHAT_RASTER_UNKNOWN;
    } else if (b == 0x62u && !interm && !nondigit && npar == 1u) { /* REP */
      if (has_last)
        put(last_cp, first_val ? first_val : 1u);
      else
        flags |= ASCIICHAT_RASTER_UNKNOWN;
    } else {
      flags |= ASCIICHAT_RASTER_UNKNOWN;
    }
  }
  /* one byte that is not part of a ground-state printable run; false: the byte ended something and counts again */
  __device__ bool step(uint32_t b) {
    switch (state) {
    case S_GROUND:
      if (b >= 0x20u && b <= 0x7Eu) {
        put(b, 1u);
      } else if (b == 0x0Au) { /* (only the tail holds newlines) */
        col = 0u;
        has_last = false;
      } else if (b == 0x0Du) {
        col = 0u;
      } else if (b == 0x1Bu) {
        state = S_ESC;
      } else if (b < 0x80u) {
        flags |= ASCIICHAT_RASTER_UNKNOWN;
      } else {
        u_len = (b >= 0xC2u && b <= 0xDFu) ? 1u : (b >= 0xE0u && b <= 0xEFu) ? 2u : (b >= 0xF0u && b <= 0xF4u) ? 3u : 0u;
        if (u_len == 0u) {
          flags |= ASCIICHAT_RASTER_BAD_UTF8;
          put(0xFFFDu, 1u);
        } else {
          u_rem = u_len;
          u_cp = b & (u_len == 1u ? 0x1Fu : u_len == 2u ? 0x0Fu : 0x07u);
          state = S_UTF8;
        }
      }
      return true;
    case S_ESC:
      if (b == 0x5Bu) {
        state = S_CSI_PARAM;
        cur = 0u, npar = 0u, first_val = 0u, mode = M_TOP;
        cur_empty = true, nondigit = false, interm = false, shadow_unknown = false;
        shadow = pen;
        return true;
      }
      flags |= ASCIICHAT_RASTER_UNKNOWN;
      state = S_GROUND;
      return false;
    case S_CSI_PARAM:
      if (b >= 0x30u && b <= 0x39u) {
        cur = min(cur * 10u + (b - 0x30u), 65535u);
        cur_empty = false;
        return true;
      }
      if (b == 0x3Bu) {
        end_param();
        return true;
      }
      if (b >= 0x3Au && b <= 0x3Fu) {
        nondigit = true;
        return true;
      }
      [[fallthrough]]; /* an intermediate, a final or neither */
    case S_CSI_INTERM:
      if (b >= 0x20u && b <= 0x2Fu) {
        state = S_CSI_INTERM;
        interm = true;
        return true;
      }
      if (b >= 0x40u && b <= 0x7Eu) {
        final_byte(b);
        return true;
      }
      flags |= ASCIICHAT_RASTER_UNKNOWN;
      state = S_GROUND;
      return false;
    default: /* S_UTF8 */
      state = S_GROUND;
      if (b >= 0x80u && b <= 0xBFu) {
        u_cp = u_cp << 6 | (b & 0x3Fu);
        if (--u_rem) {
          state = S_UTF8;
          return true;
        }
        const uint32_t least = u_len == 1u ? 0x80u : u_len == 2u ? 0x800u : 0x10000u;
        if (u_cp < least || (u_cp >= 0xD800u && u_cp <= 0xDFFFu) || u_cp > 0x10FFFFu) {
          flags |= ASCIICHAT_RASTER_BAD_UTF8;
          u_cp = 0xFFFDu;
        }
        put(u_cp, 1u);
        return true;
      }
      flags |= ASCIICHAT_RASTER_BAD_UTF8;
      put(0xFFFDu, 1u);
      return false;
    }
  }
  /* the row is over: what was in progress never completes */
  __device__ void finish() {
    if (state == S_UTF8) {
      flags |= ASCIICHAT_RASTER_BAD_UTF8;
      put(0xFFFDu, 1u);
    } else if (state != S_GROUND) {
      flags |= ASCIICHAT_RASTER_UNKNOWN;
    }
    state = S_GROUND;
  }
};

/* workgroup b: frame b / blocks_per_frame, wave w of it the text row (b % blocks_per_frame) * 4 + w; row `rows` is the text
 * behind the grid.  LDS: the atlas' codepoints, then a chunk per wave. */
__global__ void __launch_bounds__(RASTER_BLOCK)
    parse_kernel(const raster_params_t p, const uint8_t *__restrict__ frames, const uint64_t stride, const uint32_t *__restrict__ len,
                 const uint32_t *__restrict__ starts, raster_rowrec_t *__restrict__ recs, raster_cell_t *__restrict__ cells) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t rows = (uint32_t)p.rows, cols = (uint32_t)p.cols;
  const uint32_t units = rows + 1u, bpf = (units + RASTER_ROWS_PER_BLOCK - 1u) / RASTER_ROWS_PER_BLOCK;
  const uint32_t f = blockIdx.x / bpf, u = (blockIdx.x - f * bpf) * RASTER_ROWS_PER_BLOCK + wave;
  uint32_t *cps = reinterpret_cast<uint32_t *>(ACHIP_SMEM);
  uint8_t *chunk = ACHIP_SMEM + 4u * ASCIICHAT_RASTER_MAX_GLYPHS + wave * RASTER_CHUNK;
  for (uint32_t i = tid; i < (uint32_t)p.n_glyphs; i += kBlock)
    cps[i] = p.codepoints[i];
  __syncthreads();
  if (u >= units)
    return;
  const uint32_t raw = len[f], n = frame_len(len, f, stride);
  const uint8_t *__restrict__ src = frames + (uint64_t)f * stride;
  const uint32_t *__restrict__ st = starts + (uint64_t)f * (rows + 2u);
  const bool tail = u == rows;
  const uint32_t begin = min(st[u], n), end = tail ? n : min(st[u + 1u] - 1u, n);

  RowParser ps;
  ps.p = &p;
  ps.cps = cps;
  ps.row = tail ? nullptr : cells + ((uint64_t)f * rows + u) * cols;
  ps.cols = cols;
  ps.tail = tail;
  ps.lane = lane;
  ps.col = ps.hi = ps.flags = ps.last_cp = 0u;
  ps.has_last = false;
  ps.pen = Pen{0u, 0u, true, true};
  ps.shadow = ps.pen;
  ps.state = S_GROUND;
  ps.cur = ps.npar = ps.first_val = ps.acc_r = ps.acc_g = 0u;
  ps.mode = M_TOP;
  ps.cur_empty = true;
  ps.nondigit = ps.interm = ps.target_fg = ps.shadow_unknown = false;
  ps.u_len = ps.u_rem = ps.u_cp = 0u;

  for (uint32_t c0 = begin; c0 < end; c0 += RASTER_CHUNK) {
    const uint32_t cn = min((uint32_t)RASTER_CHUNK, end - c0);
    wave_lockstep(); /* the chunk before has been read */
    if (4u * lane < cn) {
      uint32_t w = 0u;
      if (4u * lane + 4u <= cn) {
        w = reinterpret_cast<const unaligned_u32 *>(src + c0 + 4u * lane)->v;
      } else {
        for (uint32_t j = 0u; 4u * lane + j < cn; j++)
          w |= (uint32_t)src[c0 + 4u * lane + j] << (8u * j);
      }
      reinterpret_cast<uint32_t *>(chunk)[lane] = w;
    }
    lds_store_fence();
    for (uint32_t g0 = 0u; g0 < cn; g0 += 64u) {
      const uint32_t gn = min(64u, cn - g0);
      const uint32_t v = lane < gn ? (uint32_t)chunk[g0 + lane] : 0u;
      const uint64_t plain = wave_ballot(v >= 0x20u && v <= 0x7Eu);
      uint32_t q = 0u;
      while (q < gn) {
        const uint64_t from = plain >> q;
        if (ps.state == S_GROUND && (from & 1ull)) {
          /* a run of printable ASCII: one cell per lane */
          const uint64_t stop = ~from;
          const uint32_t run = min(gn - q, stop ? (uint32_t)__ffsll((unsigned long long)stop) - 1u : 64u);
          ps.last_cp = wave_read_lane(v, (int)(q + run - 1u));
          ps.has_last = true;
          if (tail) {
            ps.flags |= ASCIICHAT_RASTER_OVERFLOW_ROWS;
          } else {
            const uint32_t room = cols - ps.col, take = min(run, room);
            if (run > room)
              ps.flags |= ASCIICHAT_RASTER_OVERFLOW_COLS;
            if (lane >= q && lane < q + take)
              ps.store(ps.col + (lane - q), ps.lookup(v));
            ps.col += take;
            ps.hi = max(ps.hi, ps.col);
          }
          q += run;
        } else if (ps.step(wave_read_lane(v, (int)q))) {
          q++;
        }
      }
    }
  }
  ps.finish();
  if (!tail)
    for (uint32_t c = ps.hi + lane; c < cols; c += 64u) {
      raster_cell_t blank;
      blank.slot = RASTER_NO_GLYPH;
      blank.fg = p.default_fg;
      blank.bg = p.default_bg;
      ps.row[c] = blank;
    }
  if (lane == 0u) {
    raster_rowrec_t r;
    r.fg = ps.pen.fg_in ? RASTER_PEN_UNTOUCHED : ps.pen.fg;
    r.bg = ps.pen.bg_in ? RASTER_PEN_UNTOUCHED : ps.pen.bg;
    r.flags = ps.flags | ((tail && (raw == ACHIP_LEN_OVERFLOW || (uint64_t)raw > stride)) ? ASCIICHAT_RASTER_NO_FRAME : 0u);
    r._pad = 0u;
    recs[(uint64_t)f * units + u] = r;
  }
}

/* ---- resolve ----------------------------------------------------------------------------------------------------------- */

/* workgroup b: frame b / groups, cell rows [(b % groups) * 32, + 32) */
__global__ void __launch_bounds__(RASTER_BLOCK)
    resolve_kernel(const raster_params_t p, const raster_rowrec_t *__restrict__ recs, raster_cell_t *__restrict__ cells,
                   uint32_t *__restrict__ status) {
  const uint32_t tid = threadIdx.x, rows = (uint32_t)p.rows, cols = (uint32_t)p.cols;
  const uint32_t groups = (rows + RASTER_FIX_ROWS - 1u) / RASTER_FIX_ROWS;
  const uint32_t f = blockIdx.x / groups, r0 = (blockIdx.x - f * groups) * RASTER_FIX_ROWS;
  const uint32_t nr = min((uint32_t)RASTER_FIX_ROWS, rows - r0);
  const raster_rowrec_t *__restrict__ rec = recs + (uint64_t)f * (rows + 1u);
  uint32_t *entry = reinterpret_cast<uint32_t *>(ACHIP_SMEM); /* [2][32], then the flags of 256 threads */
  uint32_t *red = entry + 2u * RASTER_FIX_ROWS;
  if (tid < 2u * nr) {
    const uint32_t t = tid >> 1, bg = tid & 1u;
    uint32_t v = bg ? p.default_bg : p.default_fg;
    for (uint32_t k = r0 + t; k-- > 0u;) {
      const uint32_t e = bg ? rec[k].bg : rec[k].fg;
      if (e != RASTER_PEN_UNTOUCHED) {
        v = e;
        break;
      }
    }
    entry[bg * RASTER_FIX_ROWS + t] = v;
  }
  uint32_t fl = 0u;
  for (uint32_t k = tid; k <= rows; k += kBlock)
    fl |= rec[k].flags;
  red[tid] = fl;
  __syncthreads();
  if (r0 == 0u && tid == 0u) {
    for (uint32_t k = 1u; k < kBlock; k++)
      fl |= red[k];
    status[f] = fl;
  }
  raster_cell_t *__restrict__ c = cells + ((uint64_t)f * rows + r0) * cols;
  for (uint32_t i = tid; i < nr * cols; i += kBlock) {
    const uint32_t slot = c[i].slot;
    if (slot & (RASTER_INHERIT_FG | RASTER_INHERIT_BG)) {
      const uint32_t t = i / cols;
      if (slot & RASTER_INHERIT_FG)
        c[i].fg = entry[t];
      if (slot & RASTER_INHERIT_BG)
        c[i].bg = entry[RASTER_FIX_ROWS + t];
      c[i].slot = slot & 0xFFFFu;
    }
  }
}

/* ---- draw -------------------------------------------------------------------------------------------------------------- */

constexpr uint32_t kTileCells = RASTER_TILE_GROUPS * 4u + 8u; /* per cell row of a tile, neighbours included */
constexpr uint32_t kCellLds = 2u * kTileCells * 20u;

__device__ inline uint32_t blend(uint32_t f, uint32_t b, uint32_t a) {
  const uint32_t na = 255u - a;
  const uint32_t r = (((f >> 16) & 255u) * a + ((b >> 16) & 255u) * na) * 0x8081u >> 23;
  const uint32_t g = (((f >> 8) & 255u) * a + ((b >> 8) & 255u) * na) * 0x8081u >> 23;
  const uint32_t bl = ((f & 255u) * a + (b & 255u) * na) * 0x8081u >> 23;
  return r | g << 8 | bl << 16 | 0xFF000000u;
}
__device__ inline uint32_t opaque_rgb(uint32_t c) { return ((c >> 16) & 255u) | (c & 0xFF00u) | (c & 255u) << 16 | 0xFF000000u; }

/* workgroup (x, y): frame x / rows, cell row x % rows, tiles y, y + gridDim.y, ... of its image rows */
__global__ void __launch_bounds__(RASTER_BLOCK)
    draw_kernel(const raster_params_t p, const raster_cell_t *__restrict__ cells, uint8_t *__restrict__ pixels, const uint64_t image_pitch,
                const uint32_t tiles) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t rows = (uint32_t)p.rows, cols = (uint32_t)p.cols, cw = (uint32_t)p.cell_w, ch = (uint32_t)p.cell_h;
  const uint32_t f = blockIdx.x / rows, r = blockIdx.x - f * rows, W = cols * cw;
  uint32_t *l_box = reinterpret_cast<uint32_t *>(ACHIP_SMEM);
  uint32_t *l_fg = l_box + 2u * kTileCells, *l_bg = l_fg + 2u * kTileCells, *l_pitch = l_bg + 2u * kTileCells,
           *l_off = l_pitch + 2u * kTileCells;
  const uint8_t *l_atlas = ACHIP_SMEM + kCellLds;
  const bool in_lds = p.atlas_in_lds != 0u;
  if (in_lds) { /* (the device copy of the coverage is 16-byte aligned and padded to 16) */
    uint4 *dst = reinterpret_cast<uint4 *>(ACHIP_SMEM + kCellLds);
    const uint4 *__restrict__ srcv = reinterpret_cast<const uint4 *>(p.coverage);
    for (uint32_t i = tid; i < (p.coverage_bytes + 15u) / 16u; i += kBlock)
      dst[i] = srcv[i];
  }
  const raster_cell_t *__restrict__ frame_cells = cells + (uint64_t)f * rows * cols;
  uint8_t *__restrict__ image = pixels + (uint64_t)f * image_pitch;
  for (uint32_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
    /* the pixels any row of this tile may hold: [256 tile - 3, 256 tile + 256) of [0, W) */
    const uint32_t px_lo = tile ? tile * 256u - 3u : 0u, px_hi = min(W - 1u, tile * 256u + 255u);
    if (px_lo > px_hi)
      break;
    const uint32_t c_lo = px_lo / cw, c_hi = px_hi / cw, ncell = c_hi - c_lo + 3u; /* LDS index 0 is cell c_lo - 1 */
    __syncthreads(); /* the tile before has been drawn */
    for (uint32_t i = tid; i < 2u * ncell; i += kBlock) {
      const uint32_t below = i >= ncell ? 1u : 0u, k = i - below * ncell;
      const int32_t cc = (int32_t)(c_lo + k) - 1;
      const uint32_t at = below * kTileCells + k;
      uint32_t box = 0u, fg = 0u, bg = 0u, pitch = 0u, off = 0u;
      if (cc >= 0 && cc < (int32_t)cols && r + below < rows) {
        const raster_cell_t c = frame_cells[(uint64_t)(r + below) * cols + (uint32_t)cc];
        fg = c.fg, bg = c.bg;
        const uint32_t slot = c.slot & 0xFFFFu;
        if (slot != RASTER_NO_GLYPH) {
          const raster_glyph_t g = p.glyphs[slot];
          box = g.box, pitch = g.pitch, off = g.offset;
        }
      }
      l_box[at] = box, l_fg[at] = fg, l_bg[at] = bg, l_pitch[at] = pitch, l_off[at] = off;
    }
    __syncthreads();
    for (uint32_t y = wave; y < ch; y += kBlock / 64u) {
      const uint64_t row_off = (uint64_t)(r * ch + y) * (4u * (uint64_t)W);
      uint8_t *__restrict__ out = image + row_off;
      const uint32_t shift = (uint32_t)(((uint64_t)(uintptr_t)out >> 2) & 3u); /* pixels of the row's first group before it */
      const int32_t xs = (int32_t)(4u * (tile * RASTER_TILE_GROUPS + lane)) - (int32_t)shift;
      if (xs >= (int32_t)W || xs + 4 <= 0)
        continue;
      const uint32_t x_first = xs < 0 ? 0u : (uint32_t)xs;
      uint32_t c = x_first / cw, lx = x_first - c * cw;
      uint32_t px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int32_t x = xs + j;
        if (x < 0 || x >= (int32_t)W)
          continue;
        const uint32_t li = c - c_lo + 1u; /* the own cell's LDS index */
        /* the candidates, last writer first: {LDS index, dx, dy} relative to that cell's origin */
        uint32_t val = opaque_rgb(l_bg[li]);
#pragma unroll
        for (int k = 0; k < 5; k++) {
          const uint32_t below = k < 3 ? 1u : 0u;
          const int32_t dc = k == 0 ? 1 : k == 1 ? 0 : k == 2 ? -1 : k == 3 ? 1 : 0;
          const uint32_t at = below * kTileCells + (uint32_t)((int32_t)li + dc);
          const uint32_t box = l_box[at];
          const uint32_t bx = (uint32_t)((int32_t)lx - dc * (int32_t)cw + 32), by = y + 64u - below * ch;
          const uint32_t x0 = box & 255u, y0 = (box >> 8) & 255u, x1 = (box >> 16) & 255u, y1 = box >> 24;
          if (bx >= x0 && bx < x1 && by >= y0 && by < y1) {
            const uint32_t idx = l_off[at] + (by - y0) * l_pitch[at] + (bx - x0);
            const uint32_t a = in_lds ? l_atlas[idx] : p.coverage[idx];
            val = blend(l_fg[at], l_bg[at], a);
            break;
          }
        }
        px[j] = val;
        if (++lx == cw) {
          lx = 0u;
          c++;
        }
      }
      if (xs >= 0 && xs + 4 <= (int32_t)W) {
        store_u4_nt(out + 4u * (uint32_t)xs, make_uint4(px[0], px[1], px[2], px[3]));
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int32_t x = xs + j;
          if (x >= 0 && x < (int32_t)W)
            reinterpret_cast<uint32_t *>(out)[x] = px[j];
        }
      }
    }
  }
}

} // namespace raster
} // namespace achip
