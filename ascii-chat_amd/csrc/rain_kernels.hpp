/*
 * rain_kernels.hpp -- the --matrix digital rain of the display path (digital_rain_apply, lib/video/anim/digital_rain.c) as
 * a string-to-string pass over a slab: frame i of the input (src + i * src_stride, src_len[i] bytes, up to its first NUL)
 * becomes frame i of the output (dst + i * dst_stride, its length in dst_len[i]), every character preceded by an SGR in the
 * rain colour and every truecolor SGR rewritten, both scaled by the rain brightness of the character's cell.
 *
 * One 256-thread workgroup per frame.  The frame is walked in chunks of 4 KB, thread t owning bytes 16t .. 16t+15 of a
 * chunk and every token that STARTS there.  Where a token starts depends on everything in front of it (inside a CSI,
 * inside a UTF-8 character), so each thread first composes the transition maps of its 16 bytes over the tokenizer's six
 * states (token start, 1-3 UTF-8 bytes left, after ESC, inside CSI); a workgroup scan of the maps gives every thread its
 * entry state.  A second scan gives every thread the (row, column, events in the cell so far) at its first token, a third
 * the output offset of its first token; then every thread writes its tokens.  The state carried from chunk to chunk is one
 * tokenizer state, one cell position and one output offset.  Each chunk (and 64 bytes beyond it) is first copied to LDS with
 * coalesced loads: the four walks over a thread's bytes read LDS, only tokens that reach further read global memory.
 *
 * Brightness B(column, row) costs two binary32 sines, taken as (float)sin((double)x): it is computed once per cell into
 * an LDS table of columns x (rows + 1) entries where that fits (ACHIP_RAIN_TABLE_MAX), on demand beyond it.  The blend with
 * the previous frame's brightness is sequential per cell -- an event that is the k-th of its cell applies it k times to the
 * stored value, stopping early once a step changes nothing -- and the cell's LAST event (its character, or the newline /
 * frame end behind colour events with no character) stores the result.  Every store happens after every read of the chunk
 * (a barrier between them), and a cell's events never span two frames of one launch (one context per launch and frame).
 *
 * A frame whose output may not fit its slot (20 * len + 1 > dst_stride) first copies its state to the backup half of the
 * state block and copies it back when it did not fit: such a frame leaves the state as it found it.  The backup half starts
 * behind the grid as ALLOCATED (desc.backup cells): a grid written smaller than that leaves the cells beyond it alone, as
 * the reference does.  A descriptor that leaves the field 0 has its backup directly behind the grid as written.
 *
 * Floating point follows the reference's source order in binary32 without contraction; division is correctly rounded
 * (hipcc's default for HIP).  Only plain HIP: the same source runs under the CPU emulator (tests/hipemu).
 */
#pragma once

#include <gfx950_ops.hpp>
#include <math.h>

#include "achip_types.h"
#include "rain.h"

#if defined(__clang__)
#define ACHIP_RAIN_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define ACHIP_RAIN_NO_CONTRACT
#endif

namespace achip {
namespace rain {

enum : uint32_t { T_CHAR = 0, T_NL = 1, T_ESC = 2, T_CSI = 3, T_COLOR = 4 };
constexpr uint32_t kBlock = ACHIP_RAIN_BLOCK, kSeg = ACHIP_RAIN_SEG, kChunk = kBlock * kSeg;
constexpr uint32_t kIdentity = 0u | (1u << 3) | (2u << 6) | (3u << 9) | (4u << 12) | (5u << 15);
constexpr uint32_t kStageBytes = kChunk + 64; /* the chunk's bytes and what tokens starting in it look at beyond it */
constexpr int kScanOff = 0;                   /* kBlock x 16 bytes of scan buffer */
constexpr int kStageOff = kBlock * 16;        /* the chunk's bytes */
constexpr int kTableOff = kStageOff + (int)kStageBytes; /* brightness table (floats) */
constexpr size_t lds_bytes(int table_entries) { return (size_t)kTableOff + 4u * (size_t)table_entries; }

/* the frame's bytes: from the LDS copy of the current chunk where it covers them, else from global memory; 0 past the end */
struct Src {
  const uint8_t *p;
  uint32_t len, lo;
  __device__ inline uint32_t at(uint32_t i) const {
    const uint32_t o = i - lo;
    if (o < kStageBytes)
      return ACHIP_SMEM[kStageOff + o];
    return i < len ? (uint32_t)p[i] : 0u;
  }
};

/* utf8_decode (lib/util/utf8.c:18-44): 1-4 bytes with continuation bytes checked, an invalid sequence is 1 byte */
__device__ inline uint32_t utf8_len(const Src &s, uint32_t i, uint32_t b0) {
  if (b0 < 0x80u)
    return 1u;
  const bool c1 = (s.at(i + 1) & 0xC0u) == 0x80u;
  if ((b0 & 0xE0u) == 0xC0u)
    return c1 ? 2u : 1u;
  const bool c2 = c1 && (s.at(i + 2) & 0xC0u) == 0x80u;
  if ((b0 & 0xF0u) == 0xE0u)
    return c2 ? 3u : 1u;
  if ((b0 & 0xF8u) == 0xF0u)
    return c2 && (s.at(i + 3) & 0xC0u) == 0x80u ? 4u : 1u;
  return 1u;
}

struct Tok {
  uint32_t type, nbytes, fg;
  int32_t r, g, b;
};

/* the token that starts at byte i (i < the frame's end) */
__device__ inline Tok token_at(const Src &s, uint32_t i) {
  Tok t{T_CHAR, 1u, 1u, 0, 0, 0};
  const uint32_t b0 = s.at(i);
  if (b0 == 0x1Bu) {
    if (s.at(i + 1) != '[') {
      t.type = T_ESC;
      return t;
    }
    const uint32_t j = i + 2;
    const uint32_t c0 = s.at(j);
    if ((c0 == '3' || c0 == '4') && s.at(j + 1) == '8' && s.at(j + 2) == ';' && s.at(j + 3) == '2' && s.at(j + 4) == ';') {
      uint32_t p = j + 5;
      /* one digit run (may be empty: 0) and the byte that must follow it */
      auto run = [&](int32_t &out, uint32_t sep) {
        uint32_t v = 0, d;
        while ((d = s.at(p)) >= '0' && d <= '9') {
          v = v * 10u + (d - '0'); /* (beyond 9 digits the reference's int overflows: outside the contract) */
          p++;
        }
        out = (int32_t)v;
        return s.at(p++) == sep;
      };
      if (run(t.r, ';') && run(t.g, ';') && run(t.b, 'm')) {
        t.type = T_COLOR;
        t.nbytes = p - i;
        t.fg = c0 == '3';
        return t;
      }
    }
    uint32_t k = j, c;
    while ((c = s.at(k)) != 0u && !(c >= 0x40u && c <= 0x7Eu))
      k++;
    t.type = T_CSI;
    t.nbytes = (c != 0u ? k + 1 : k) - i;
    return t;
  }
  if (b0 == '\n') {
    t.type = T_NL;
    return t;
  }
  t.nbytes = utf8_len(s, i, b0);
  return t;
}

/* ---- the tokenizer's states as maps: 6 entries of 3 bits ---- */
__device__ inline uint32_t map_get(uint32_t m, uint32_t s) { return (m >> (3u * s)) & 7u; }
__device__ inline uint32_t map_then(uint32_t a, uint32_t b) { /* a, then b */
  uint32_t r = 0;
  for (uint32_t s = 0; s < 6u; s++)
    r |= map_get(b, map_get(a, s)) << (3u * s);
  return r;
}
/* the state after byte i (value b), from each state */
__device__ inline uint32_t byte_map(const Src &src, uint32_t i, uint32_t b) {
  const uint32_t start = b == 0x1Bu ? 4u : b == '\n' ? 0u : utf8_len(src, i, b) - 1u;
  const uint32_t fin = (b >= 0x40u && b <= 0x7Eu) ? 0u : 5u;
  return start | (0u << 3) | (1u << 6) | (2u << 9) | ((b == '[' ? 5u : start) << 12) | (fin << 15);
}

/* ---- workgroup scans (Hillis-Steele over LDS; portable, emulated as written) ---- */
template <class T, class Op> __device__ inline T block_scan_incl(T v, Op op, uint32_t tid) {
  T *buf = reinterpret_cast<T *>(ACHIP_SMEM + kScanOff);
  buf[tid] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kBlock; d <<= 1) {
    const T o = tid >= d ? buf[tid - d] : v;
    __syncthreads();
    if (tid >= d)
      v = op(o, v);
    buf[tid] = v;
    __syncthreads();
  }
  return v;
}
/* exclusive prefix (identity for thread 0) and the total; leaves the buffer free for the next scan */
template <class T> struct Scan {
  T excl, total;
};
template <class T, class Op> __device__ inline Scan<T> block_scan(T v, Op op, T identity, uint32_t tid) {
  block_scan_incl(v, op, tid);
  const T *buf = reinterpret_cast<const T *>(ACHIP_SMEM + kScanOff);
  const Scan<T> r{tid ? buf[tid - 1] : identity, buf[kBlock - 1]};
  __syncthreads();
  return r;
}

struct MapNul {
  uint32_t map, nul;
};
struct Cell { /* a run of tokens as a function of (row, col, k): see apply() */
  uint32_t nl, c, reset, kk;
};
__device__ inline Cell cell_then(Cell a, Cell b) {
  return Cell{a.nl + b.nl, b.nl ? b.c : a.c + b.c, a.reset | b.reset, b.reset ? b.kk : a.kk + b.kk};
}
struct Pos {
  int32_t row, col;
  uint32_t k; /* events of the current cell so far */
};
__device__ inline Pos apply(Pos p, Cell a) {
  return Pos{p.row + (int32_t)a.nl, a.nl ? (int32_t)a.c : p.col + (int32_t)a.c, a.reset ? a.kk : p.k + a.kk};
}

/* ---- brightness ---- */
struct Rain {
  float *state;
  const float *cols;
  float t, fall_speed, raindrop_length, decay;
  int32_t ncol, nrow;
  bool first, use_table;
};

ACHIP_RAIN_NO_CONTRACT
__device__ inline float column_time(const Rain &R, int32_t c) {
  return R.cols[2 * c] + R.t * R.fall_speed * R.cols[2 * c + 1];
}
ACHIP_RAIN_NO_CONTRACT
__device__ inline float brightness_at(float column_time, int32_t row, float raindrop_length) {
  const float x = (column_time - (float)row) / raindrop_length;
  const float s2 = (float)sin((double)(1.41421354f * x));
  const float s5 = (float)sin((double)(2.23606801f * x));
  const float w = x + 0.3f * s2 + 0.2f * s5;
  return 1.0f - (w - floorf(w));
}
__device__ inline float brightness(const Rain &R, int32_t c, int32_t r) {
  if (c >= R.ncol)
    return 0.0f;
  if (R.use_table && r <= R.nrow)
    return reinterpret_cast<const float *>(ACHIP_SMEM + kTableOff)[r * R.ncol + c];
  return brightness_at(column_time(R, c), r, R.raindrop_length);
}
__device__ inline uint32_t fbits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
/* the k-th event of cell (c, r): its blended brightness (what the cell stores after it) and whether it is a cursor */
ACHIP_RAIN_NO_CONTRACT
__device__ inline float event_brightness(const Rain &R, int32_t c, int32_t r, uint32_t k, bool &cursor) {
  const float raw = brightness(R, c, r);
  cursor = raw > brightness(R, c, r + 1);
  if (R.first || r >= R.nrow || c >= R.ncol)
    return raw;
  float b = R.state[(size_t)r * (size_t)R.ncol + (size_t)c];
  for (uint32_t q = 0; q < k; q++) {
    const float nb = b + (raw - b) * R.decay;
    if (fbits(nb) == fbits(b))
      break; /* the same step again changes nothing either */
    b = nb;
  }
  return b;
}
__device__ inline void store_state(const Rain &R, int32_t c, int32_t r, uint32_t k) {
  if (r >= R.nrow || c >= R.ncol)
    return;
  bool cursor;
  const float b = event_brightness(R, c, r, k, cursor);
  R.state[(size_t)r * (size_t)R.ncol + (size_t)c] = b;
}
ACHIP_RAIN_NO_CONTRACT
__device__ inline uint32_t modulate(int32_t v, float b, bool cursor) {
  if (cursor)
    b *= 2.0f;
  if (!(b >= 0.0f)) /* (negative or NaN: NaN converts to INT_MIN on the reference's x86, then clamps to 0) */
    b = 0.0f;
  if (b > 1.0f)
    b = 1.0f;
  const float f = (float)v * b;
  int32_t x = (f >= -2147483648.0f && f < 2147483648.0f) ? (int32_t)f : (int32_t)0x80000000u;
  return x < 0 ? 0u : x > 255 ? 255u : (uint32_t)x;
}
__device__ inline uint32_t digits(uint32_t v) { return 1u + (v >= 10u) + (v >= 100u); }
/* ESC [ 3|4 8 ; 2 ; R ; G ; B m, the channels packed as r | g << 8 | b << 16 */
__device__ inline uint32_t sgr_len(uint32_t c) { return 10u + digits(c & 0xFFu) + digits((c >> 8) & 0xFFu) + digits(c >> 16); }

struct Out {
  uint8_t *p;
  uint64_t cap;
  __device__ inline void put(uint64_t o, uint32_t b) const {
    if (o < cap)
      p[o] = (uint8_t)b;
  }
  __device__ inline uint64_t num(uint64_t o, uint32_t v) const {
    if (v >= 100u)
      put(o++, '0' + v / 100u);
    if (v >= 10u)
      put(o++, '0' + (v / 10u) % 10u);
    put(o++, '0' + v % 10u);
    return o;
  }
  __device__ inline uint64_t sgr(uint64_t o, bool fg, uint32_t c) const {
    put(o, 0x1B);
    put(o + 1, '[');
    put(o + 2, fg ? '3' : '4');
    put(o + 3, '8');
    put(o + 4, ';');
    put(o + 5, '2');
    put(o + 6, ';');
    o = num(o + 7, c & 0xFFu);
    put(o++, ';');
    o = num(o, (c >> 8) & 0xFFu);
    put(o++, ';');
    o = num(o, c >> 16);
    put(o++, 'm');
    return o;
  }
};

/* the first token start in [lo, hi) for a thread entering in tokenizer state s (hi when none) */
__device__ inline uint32_t first_start(const Src &S, uint32_t lo, uint32_t hi, uint32_t s) {
  uint32_t i = lo;
  while (i < hi && s != 0u) {
    const uint32_t b = S.at(i);
    if (s == 5u) {
      s = (b >= 0x40u && b <= 0x7Eu) ? 0u : 5u;
      i++;
    } else if (s == 4u) {
      if (b == '[') {
        s = 5u;
        i++;
      } else {
        s = 0u; /* a lone ESC in front: this byte starts a token */
      }
    } else {
      s--;
      i++;
    }
  }
  return s == 0u ? i : hi;
}

/* the colour an event writes: its own (a colour SGR) or the rain's (a character), scaled */
__device__ inline uint32_t event_color(const Tok &t, uint32_t color, float b, bool cursor) {
  const bool own = t.type == T_COLOR;
  return modulate(own ? t.r : (int32_t)(color & 0xFFu), b, cursor) | modulate(own ? t.g : (int32_t)((color >> 8) & 0xFFu), b, cursor) << 8 |
         modulate(own ? t.b : (int32_t)(color >> 16), b, cursor) << 16;
}

__global__ void __launch_bounds__(256)
    rain_kernel(const achip_rain_desc_t *__restrict__ desc, int table_cap, const uint8_t *__restrict__ src_base,
                uint64_t src_stride, const uint32_t *__restrict__ src_len, uint8_t *__restrict__ dst_base, uint64_t dst_stride,
                uint32_t *__restrict__ dst_len) {
  const uint32_t tid = threadIdx.x;
  const uint32_t f = blockIdx.x;
  const achip_rain_desc_t d = desc[f];
  uint32_t len = src_len[f];
  if (len >= 0xFFFFFFF0u) { /* an upstream error code travels on; the state is not touched */
    if (tid == 0)
      dst_len[f] = len;
    return;
  }
  if ((uint64_t)len > src_stride)
    len = (uint32_t)src_stride;
  Src S{src_base + (uint64_t)f * src_stride, len, 0xFFFFFFFFu - kStageBytes};
  const Out O{dst_base + (uint64_t)f * dst_stride, dst_stride};
  Rain R{d.state, d.cols, d.t, d.fall_speed, d.raindrop_length, d.decay, d.num_columns, d.num_rows, (d.color >> 24) != 0u, false};
  const uint32_t color = d.color & 0xFFFFFFu;
  const size_t cells = (size_t)R.ncol * (size_t)R.nrow;
  const bool may_overflow = 20ull * len + 1ull > dst_stride;
  /* never inside the live cells: a descriptor that leaves the field 0 gets the backup directly behind the grid as written */
  const size_t backup = (size_t)d.backup > cells ? (size_t)d.backup : cells;
  if (may_overflow)
    for (size_t q = tid; q < cells; q += kBlock)
      R.state[backup + q] = R.state[q];
  const uint64_t entries = (uint64_t)R.ncol * (uint64_t)(R.nrow + 1);
  R.use_table = entries <= (uint64_t)table_cap;
  if (R.use_table) {
    float *table = reinterpret_cast<float *>(ACHIP_SMEM + kTableOff);
    for (uint32_t q = tid; q < (uint32_t)entries; q += kBlock) {
      const int32_t r = (int32_t)(q / (uint32_t)R.ncol), c = (int32_t)(q % (uint32_t)R.ncol);
      table[q] = brightness_at(column_time(R, c), r, R.raindrop_length);
    }
  }
  __syncthreads();

  uint32_t carry_state = 0;
  Pos carry_pos{0, 0, 0};
  uint64_t carry_out = 0;
  for (uint32_t lo = 0; lo < len; lo += kChunk) {
    for (uint32_t q = tid; q < kStageBytes; q += kBlock) /* coalesced: every later read of the chunk is an LDS read */
      ACHIP_SMEM[kStageOff + q] = lo + q < len ? S.p[lo + q] : (uint8_t)0;
    S.lo = lo;
    __syncthreads();
    const uint32_t seg_lo = lo + tid * kSeg;
    const uint32_t seg_hi = seg_lo + kSeg < len ? seg_lo + kSeg : len;
    /* 1. transition map of this thread's bytes, and the chunk's first NUL */
    MapNul mine{kIdentity, 0xFFFFFFFFu};
    for (uint32_t i = seg_lo; i < seg_hi; i++) {
      const uint32_t b = S.at(i);
      if (b == 0u && mine.nul == 0xFFFFFFFFu)
        mine.nul = i;
      mine.map = map_then(mine.map, byte_map(S, i, b));
    }
    const Scan<MapNul> ms = block_scan(
        mine, [](MapNul a, MapNul b) { return MapNul{map_then(a.map, b.map), a.nul < b.nul ? a.nul : b.nul}; },
        MapNul{kIdentity, 0xFFFFFFFFu}, tid);
    const MapNul ex = ms.excl, tot = ms.total;
    const uint32_t end = tot.nul < len ? tot.nul : len; /* the frame ends at its first NUL */
    const uint32_t s0 = map_get(ex.map, carry_state);
    const uint32_t first = first_start(S, seg_lo, seg_hi, s0);

    /* 2. cell positions */
    Cell cm{0, 0, 0, 0};
    for (uint32_t i = first; i < seg_hi && i < end;) {
      const Tok t = token_at(S, i);
      if (t.type == T_NL)
        cm = Cell{cm.nl + 1, 0, 1, 0};
      else if (t.type == T_CHAR)
        cm = Cell{cm.nl, cm.c + 1, 1, 0};
      else if (t.type == T_COLOR)
        cm.kk++;
      i += t.nbytes;
    }
    const Scan<Cell> cs = block_scan(cm, [](Cell a, Cell b) { return cell_then(a, b); }, Cell{0, 0, 0, 0}, tid);
    const Cell cex = cs.excl, ctot = cs.total;
    const Pos p0 = apply(carry_pos, cex);

    /* 3. output lengths */
    uint32_t olen = 0;
    {
      Pos p = p0;
      for (uint32_t i = first; i < seg_hi && i < end;) {
        const Tok t = token_at(S, i);
        if (t.type == T_NL) {
          olen += 1;
          p = Pos{p.row + 1, 0, 0};
        } else if (t.type == T_ESC || t.type == T_CSI) {
          olen += t.nbytes;
        } else {
          bool cursor;
          p.k++;
          const float b = event_brightness(R, p.col, p.row, p.k, cursor);
          const uint32_t c = event_color(t, color, b, cursor);
          olen += sgr_len(c) + (t.type == T_CHAR ? t.nbytes : 0u);
          if (t.type == T_CHAR)
            p = Pos{p.row, p.col + 1, 0};
        }
        i += t.nbytes;
      }
    }
    const Scan<uint32_t> os = block_scan(olen, [](uint32_t a, uint32_t b) { return a + b; }, 0u, tid);
    const uint32_t oex = os.excl, otot = os.total;

    /* 4. the bytes (every state read of this chunk happens here or above) */
    {
      Pos p = p0;
      uint64_t o = carry_out + oex;
      for (uint32_t i = first; i < seg_hi && i < end;) {
        const Tok t = token_at(S, i);
        if (t.type == T_NL) {
          O.put(o++, '\n');
          p = Pos{p.row + 1, 0, 0};
        } else if (t.type == T_ESC || t.type == T_CSI) {
          for (uint32_t q = 0; q < t.nbytes; q++)
            O.put(o++, S.at(i + q));
        } else {
          bool cursor;
          p.k++;
          const float b = event_brightness(R, p.col, p.row, p.k, cursor);
          const uint32_t c = event_color(t, color, b, cursor);
          o = O.sgr(o, t.fg != 0u, c);
          if (t.type == T_CHAR) {
            for (uint32_t q = 0; q < t.nbytes; q++)
              O.put(o++, S.at(i + q));
            p = Pos{p.row, p.col + 1, 0};
          }
        }
        i += t.nbytes;
      }
    }
    __syncthreads();

    /* 5. state: each cell's last event stores what it computed */
    {
      Pos p = p0;
      for (uint32_t i = first; i < seg_hi && i < end;) {
        const Tok t = token_at(S, i);
        if (t.type == T_NL) {
          if (p.k > 0u) /* colour events with no character behind them before the newline */
            store_state(R, p.col, p.row, p.k);
          p = Pos{p.row + 1, 0, 0};
        } else if (t.type == T_COLOR) {
          p.k++;
        } else if (t.type == T_CHAR) {
          p.k++;
          store_state(R, p.col, p.row, p.k);
          p = Pos{p.row, p.col + 1, 0};
        }
        i += t.nbytes;
      }
    }
    carry_state = map_get(tot.map, carry_state);
    carry_pos = apply(carry_pos, ctot);
    carry_out += otot;
    __syncthreads();
    if (end < len)
      break;
  }
  if (tid == 0 && carry_pos.k > 0u) /* colour events at the very end */
    store_state(R, carry_pos.col, carry_pos.row, carry_pos.k);
  const bool overflow = carry_out + 1u > dst_stride;
  if (overflow && may_overflow) {
    __syncthreads();
    for (size_t q = tid; q < cells; q += kBlock)
      R.state[q] = R.state[backup + q];
  }
  if (tid == 0) {
    if (!overflow)
      O.put(carry_out, 0u);
    dst_len[f] = overflow ? ACHIP_LEN_OVERFLOW : (uint32_t)carry_out;
  }
}

} // namespace rain
} // namespace achip
