/*
 * zpack_kernels.hpp -- the wire stage with the frames compressed on the device: every rendered frame becomes a valid zstd
 * frame made only of raw, RLE and Huffman-literals blocks with zero sequences ("zhuf"), and is sent in that form
 * when the reference's own rule says so (lib/network/packet/packet.c:444-469: more than 1024 bytes and below 0.8 of the
 * original), else as it is.  Every client decodes such a frame with ZSTD_decompress (lib/network/compression.c:58-70).
 *
 * Four launches on one stream, one 256-thread workgroup per (frame, piece of 128 KB) in the two that touch the bytes:
 *   measure  16-byte loads of the piece: the CRC-32C register of the original bytes (crc_math.hpp's scheme) and a histogram
 *            per Huffman stream in the same read; code lengths (two-queue merge, limited to 11 bits: zpack_code_lengths below
 *            states the algorithm, tests/zhuf_ref.py restates it), canonical codes, and from sum(count * length) the exact size
 *            of every stream -- so the block type and its size are known before a bit is written.  Record -> scratch.
 *   plan     one workgroup: the frame rule, the sent lengths, off[i] = sum of round16(sent_len[j]) (pack_frames' layout, no
 *            first-come claim), the frame checksums.
 *   encode   wave w writes Huffman stream w: a lane owns a run of 16-byte groups of the piece, a wave scan of the runs' bit
 *            lengths gives every lane its distance from the stream's END (streams are written last symbol first), codes are
 *            ORed into an LDS image of the block (ds_or_b32); the image lies at the destination's phase (byte k of the
 *            image at LDS offset (address of byte k) mod 16), is checksummed there and drained in aligned 16-byte stores,
 *            its ragged ends in byte stores -- a neighbouring block's bytes are never touched.  Frames sent as they are
 *            are copied in whole groups, as crc_kernels.hpp's COPY form does.
 *   close    one thread per frame: the 24-byte header {width, height, original_size, compressed_size, checksum, flags} and
 *            the CRC of header || payload as sent, combined from the blocks' registers.
 * The slab is read twice (measure, encode).  Nothing is stored at or behind dst + capacity.
 *
 * measure and encode are templates over the form (Form<Wide> below): the narrow one codes symbols 0 .. 128 with the tree in
 * the direct form, the wide one all 256 with the tree in the FSE-compressed form where a piece holds a byte above 0x80; plan
 * and close take the words of a piece's record as a template argument.  Without template arguments a kernel is the narrow one.
 */
#pragma once

#include <gfx950_ops.hpp>

#include "crc_math.hpp"
#include "zpack.h"

namespace achip {
namespace zpack {

constexpr int kBlock = ACHIP_ZPACK_BLOCK;
constexpr uint32_t kPiece = ACHIP_ZPACK_PIECE;
constexpr uint32_t kMaxBits = ACHIP_ZPACK_MAX_BITS;
constexpr uint32_t kFull = 1u << kMaxBits;

/* The two forms of the pass.  Narrow: symbols 0 .. 128, the tree in the direct form, a piece with a byte above 0x80 is never
 * coded.  Wide: all 256 symbols, the tree of a piece whose largest symbol is above 128 in the FSE-compressed form
 * (zpack_fse_tree below); a piece without such a byte comes out as in the narrow form, byte for byte. */
template <bool Wide>
struct Form {
  static constexpr int syms = Wide ? 256 : 129;   /* symbols a table holds */
  static constexpr int leaves = Wide ? 256 : 132; /* ... rounded to whole 16-byte groups of words */
  static constexpr int nodes = Wide ? 512 : 260;  /* 2 * syms - 1 tree nodes, rounded likewise */
  static constexpr int rec_words = Wide ? ACHIP_ZPACK_WIDE_REC_WORDS : ACHIP_ZPACK_REC_WORDS;
};

/* LDS of the measure kernel: the checksum's tables and scratch (CrcLds), then the histograms and the code builder's arrays */
template <bool Wide>
struct MLdsT {
  static constexpr int o_hist = CrcLds::bytes;                         /* uint32 [4][256]: per stream */
  static constexpr int o_tot = o_hist + 4096;                          /* uint32 [256]: per symbol */
  static constexpr int o_sorted = o_tot + 1024;                        /* uint32 [leaves]: symbols by (count, value) */
  static constexpr int o_wt = o_sorted + 4 * Form<Wide>::leaves;       /* uint32 [nodes]: node weights, then depths */
  static constexpr int o_par = o_wt + 4 * Form<Wide>::nodes;           /* uint32 [nodes] */
  static constexpr int o_len = o_par + 4 * Form<Wide>::nodes;          /* uint32 [leaves]: code length per symbol */
  static constexpr int o_misc = o_len + 4 * Form<Wide>::leaves;        /* uint32 [64] */
  static constexpr int o_fse = o_misc + 256;                           /* uint32 [192]: the wide form's tree builder (FSE_* below) */
  static constexpr int bytes = o_fse + (Wide ? 4 * 192 : 0);
};
using MLds = MLdsT<false>;
static_assert(MLds::o_wt - MLds::o_sorted == 528 && MLds::o_par - MLds::o_wt == 1040 && MLds::o_misc - MLds::o_len == 528, "the narrow layout");
enum { M_TOP = 0, M_COUNT = 4, M_BAD = 8, M_MAXBITS = 12, M_START = 16 /* [12] */, M_SIZE = 32 /* [4] */, M_KIND = 40, M_TREE = 41 };
/* the tree builder's arrays, words from MLdsT::o_fse */
enum { FSE_N = 0 /* [12] */, FSE_CUMUL = 16 /* [12] */, FSE_CELL = 32 /* [64] */, FSE_STATE = 96 /* [64] */, FSE_DNB = 160 /* [12] */, FSE_DFS = 176 /* [12] */ };
static_assert(CrcLds::bytes % 16 == 0, "16-byte aligned arrays behind the checksum's");

/* LDS of the encode kernel: the checksum's, the piece's code table, the image of the block */
template <bool Wide>
struct ELdsT {
  static constexpr int o_code = CrcLds::bytes; /* uint32 [leaves] */
  static constexpr int o_img = o_code + 4 * Form<Wide>::leaves;
  /* frame header + block header + the block (never above the piece) at any phase, rounded to groups */
  static constexpr size_t bytes(uint32_t max_piece) { return (size_t)o_img + (((size_t)max_piece + 9u + 3u + 15u + 15u) & ~(size_t)15u); }
};
using ELds = ELdsT<false>;
static_assert(ELds::o_img % 16 == 0 && ELdsT<true>::o_img % 16 == 0, "the image's groups are aligned");
static_assert(ELds::bytes(kPiece) <= 160u * 1024u && ELdsT<true>::bytes(kPiece) <= 160u * 1024u, "a whole piece's image fits the LDS of a CU");
static_assert(MLdsT<true>::bytes <= 160 * 1024, "the wide measure kernel's arrays fit too");

__device__ inline uint32_t stream_of(uint32_t pos, uint32_t seg) { return (pos >= seg ? 1u : 0u) + (pos >= 2u * seg ? 1u : 0u) + (pos >= 3u * seg ? 1u : 0u); }

/* Code lengths of m >= 2 symbols, ONE thread.  wt[0..m): the counts in ascending order (ties: symbol value ascending).
 *   1. two-queue Huffman merge: leaves in that order, internal nodes in creation order, the smaller weight first, a leaf
 *      before an internal node of equal weight; a leaf's depth is its length.
 *   2. depths above 11 are cut to 11, K = sum of 2^(11 - length) in units of 2^-11.
 *   3. demote while K > 2048: the longest code below 11 bits (of those the least frequent: the first in order) gets one bit more.
 *   4. promote while K < 2048: the most frequent symbol (the last in order) whose step 2^(11 - length) fits 2048 - K loses a bit.
 * On return wt[0..m) holds the lengths.  (A longest code's step always fits, so 4 ends with K == 2048.) */
__device__ inline void zpack_code_lengths(uint32_t *wt, uint32_t *par, uint32_t m) {
  uint32_t li = 0, ii = m;
  for (uint32_t k = m; k < 2u * m - 1u; k++) {
    uint32_t sum = 0;
    for (int r = 0; r < 2; r++) {
      const bool leaf = li < m && (ii >= k || wt[li] <= wt[ii]);
      const uint32_t idx = leaf ? li++ : ii++;
      par[idx] = k;
      sum += wt[idx];
    }
    wt[k] = sum;
  }
  wt[2u * m - 2u] = 0u;
  uint32_t deepest = 0;
  for (int k = (int)(2u * m - 3u); k >= 0; k--) {
    wt[k] = wt[par[k]] + 1u;
    if ((uint32_t)k < m)
      deepest = max(deepest, wt[k]);
  }
  if (deepest <= kMaxBits)
    return;
  uint32_t kraft = 0;
  for (uint32_t j = 0; j < m; j++) {
    wt[j] = min(wt[j], kMaxBits);
    kraft += kFull >> wt[j];
  }
  while (kraft > kFull) {
    int best = -1;
    for (uint32_t j = 0; j < m; j++)
      if (wt[j] < kMaxBits && (best < 0 || wt[j] > wt[best]))
        best = (int)j;
    wt[best] += 1u;
    kraft -= kFull >> wt[best];
  }
  while (kraft < kFull) {
    for (int j = (int)m - 1; j >= 0; j--)
      if ((kFull >> wt[j]) <= kFull - kraft) {
        kraft += kFull >> wt[j];
        wt[j] -= 1u;
        break;
      }
  }
}

/* The tree of a wide piece whose largest symbol `top` is above 128, in zstd's FSE-compressed form, ONE thread: the weights
 * of symbols 0 .. top - 1 (maxbits + 1 - length, 0: absent) as an FSE stream of Accuracy_Log 6.
 *   1. c[w]: how many of the weights are w; n[w] = max(1, 64 c[w] / top) for a present w; while the sum is above 64 the largest
 *      n (ties: the smallest w) loses one, then the largest takes what is missing to 64.  No "less than 1" probability.
 *   2. the table description (FSE_writeNCount's bits), padded to a byte.
 *   3. the coding table: symbols spread with step 43 over 64 cells, stateTable, deltaNbBits / deltaFindState per value.
 *   4. the weights from the last to the first through two states, the states, the end mark.
 * out: 32 words that receive header byte || description || bitstream (nothing is stored behind them).  Returns their byte
 * count, or 0 where the form does not apply: one weight value only, or more than 127 bytes behind the header byte.  Every
 * array lives in LDS (fse: FSE_* above) -- private ones would be scratch memory. */
__device__ inline uint32_t zpack_fse_tree(const uint32_t *clen, uint32_t top, uint32_t maxbits, uint32_t *fse, uint32_t *out) {
  uint32_t *nn = fse + FSE_N, *cumul = fse + FSE_CUMUL, *cell = fse + FSE_CELL, *state = fse + FSE_STATE;
  uint32_t *dnb = fse + FSE_DNB;
  int32_t *dfs = reinterpret_cast<int32_t *>(fse + FSE_DFS);
  auto weight = [&](uint32_t s) { const uint32_t l = clen[s]; return l ? maxbits + 1u - l : 0u; };
  for (uint32_t w = 0; w < 12u; w++)
    nn[w] = 0u;
  for (uint32_t s = 0; s < top; s++)
    nn[weight(s)] += 1u;
  uint32_t present = 0, sum = 0;
  for (uint32_t w = 0; w < 12u; w++)
    if (nn[w] != 0u) {
      present += 1u;
      nn[w] = max(1u, 64u * nn[w] / top);
      sum += nn[w];
    }
  if (present < 2u)
    return 0u;
  auto largest = [&]() {
    uint32_t b = 0;
    for (uint32_t w = 1; w < 12u; w++)
      b = nn[w] > nn[b] ? w : b;
    return b;
  };
  for (; sum > 64u; sum--)
    nn[largest()] -= 1u;
  if (sum < 64u)
    nn[largest()] += 64u - sum;

  /* an LSB-first bit stream into `out` through a 64-bit accumulator; byte 0 is the header byte, filled in at the end */
  uint64_t acc = 0;
  uint32_t held = 8u, word = 0u;
  auto put = [&](uint32_t v, uint32_t nb) { /* nb <= 7 */
    acc |= (uint64_t)v << held;
    held += nb;
    if (held >= 32u) {
      if (word < 32u)
        out[word] = (uint32_t)acc;
      acc >>= 32;
      held -= 32u;
      word += 1u;
    }
  };
  put(1u, 4u); /* Accuracy_Log - 5 */
  {
    uint32_t remaining = 65u, threshold = 64u, nb = 7u, w = 0u;
    while (remaining > 1u) {
      const uint32_t mx = 2u * threshold - 1u - remaining, c = nn[w];
      uint32_t v = c + 1u;
      remaining -= c;
      if (v >= threshold)
        v += mx;
      put(v, v < mx ? nb - 1u : nb);
      while (remaining < threshold) {
        nb -= 1u;
        threshold >>= 1;
      }
      w += 1u;
      if (c == 0u) { /* the zeros behind this one, three per flag */
        uint32_t r = 0;
        while (nn[w] == 0u) {
          w += 1u;
          r += 1u;
        }
        for (; r >= 3u; r -= 3u)
          put(3u, 2u);
        put(r, 2u);
      }
    }
    put(0u, (0u - held) & 7u);
  }
  {
    uint32_t pos = 0, total = 0;
    for (uint32_t w = 0; w < 12u; w++) {
      cumul[w] = total;
      const uint32_t c = nn[w];
      for (uint32_t k = 0; k < c; k++) {
        cell[pos] = w;
        pos = (pos + 43u) & 63u;
      }
      if (c == 1u) {
        dnb[w] = (6u << 16) - 64u;
        dfs[w] = (int32_t)total - 1;
      } else if (c > 1u) {
        const uint32_t b = 6u - (31u - (uint32_t)__clz((int)(c - 1u)));
        dnb[w] = (b << 16) - (c << b);
        dfs[w] = (int32_t)total - (int32_t)c;
      }
      total += c;
    }
    for (uint32_t u = 0; u < 64u; u++)
      state[cumul[cell[u]]++] = 64u + u;
  }
  auto init = [&](uint32_t w) {
    const uint32_t nb = (dnb[w] + 32768u) >> 16;
    return state[(int32_t)(((nb << 16) - dnb[w]) >> nb) + dfs[w]];
  };
  auto step = [&](uint32_t st, uint32_t w) {
    const uint32_t nb = (st + dnb[w]) >> 16;
    put(st & ((1u << nb) - 1u), nb);
    return state[(int32_t)(st >> nb) + dfs[w]];
  };
  uint32_t s1, s2, at;
  if (top & 1u) {
    s1 = init(weight(top - 1u));
    s2 = init(weight(top - 2u));
    s1 = step(s1, weight(top - 3u));
    at = top - 3u;
  } else {
    s2 = init(weight(top - 1u));
    s1 = init(weight(top - 2u));
    at = top - 2u;
  }
  for (; at > 0u; at -= 2u) { /* an even count is left: symbol 0 goes through s1 */
    s2 = step(s2, weight(at - 1u));
    s1 = step(s1, weight(at - 2u));
  }
  put(s2 & 63u, 6u);
  put(s1 & 63u, 6u);
  put(1u, 1u);
  put(0u, (0u - held) & 7u);
  const uint32_t bytes = 4u * word + held / 8u;
  if (held != 0u && word < 32u)
    out[word] = (uint32_t)acc;
  if (bytes > 128u)
    return 0u;
  out[0] |= bytes - 1u;
  return bytes;
}

/* workgroup b: frame b / pieces, piece b % pieces.  tab: the image of crc_frame_tables_init_kernel<256>. */
template <bool Wide = false>
__global__ void __launch_bounds__(ACHIP_ZPACK_BLOCK)
    zpack_measure_kernel(const uint8_t *__restrict__ base, uint64_t stride, const uint32_t *__restrict__ len, int n_frames,
                         uint32_t pieces, uint32_t *__restrict__ scratch, const uint4 *__restrict__ tab) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  const uint32_t i = blockIdx.x / pieces, p = blockIdx.x - i * pieces;
  if (i >= (uint32_t)n_frames)
    return;
  using F = Form<Wide>;
  using ML = MLdsT<Wide>;
  uint32_t *rec = scratch + ((size_t)i * pieces + p) * F::rec_words;
  uint32_t L = len[i];
  const uint64_t lo = (uint64_t)p * kPiece;
  if (L >= 0xFFFFFFF0u || (p > 0u && lo >= L)) {
    if (tid == 0) {
      rec[ZR_KIND] = 3u;
      rec[ZR_N] = 0u;
      rec[ZR_BODY] = 0u;
    }
    return;
  }
  const uint32_t n = (uint32_t)min((uint64_t)L - lo, (uint64_t)kPiece);
  const uint8_t *src = base + (size_t)i * stride + lo;
  uint32_t *slice = lds_ptr<uint32_t>(CrcLds::o_slice), *mulh = lds_ptr<uint32_t>(CrcLds::o_mulh), *tree = lds_ptr<uint32_t>(CrcLds::o_tree);
  uint32_t *hist = lds_ptr<uint32_t>(ML::o_hist), *tot = lds_ptr<uint32_t>(ML::o_tot), *sorted = lds_ptr<uint32_t>(ML::o_sorted);
  uint32_t *wt = lds_ptr<uint32_t>(ML::o_wt), *par = lds_ptr<uint32_t>(ML::o_par), *clen = lds_ptr<uint32_t>(ML::o_len);
  uint32_t *misc = lds_ptr<uint32_t>(ML::o_misc);
  const uint32_t lane_k = CRC_LANE_TAB.k[lane], lane_xk = CRC_LANE_TAB.xk[lane];
  for (int k = tid; k < ACHIP_FRAME_CRC_TAB_BYTES / 16; k += kBlock)
    lds_ptr<uint4>(CrcLds::o_slice)[k] = tab[k];
  for (int k = tid; k < 1024; k += kBlock)
    hist[k] = 0u;
  if (tid < F::leaves)
    clen[tid] = 0u;
  const int full = (int)(n >> 4);
  const int rounds = (full + kBlock - 1) / kBlock;
  const int lead = rounds * kBlock - full;
  const uint32_t ntail = n & 15u, seg = (n + 3u) >> 2;
  const uint32_t tail_byte = (uint32_t)tid < ntail ? src[(size_t)full * 16u + (uint32_t)tid] : 0u;
  __syncthreads();
  if ((uint32_t)tid < ntail)
    atomicAdd(&hist[stream_of((uint32_t)full * 16u + (uint32_t)tid, seg) * 256u + tail_byte], 1u);

  uint32_t s = 0;
  for (int j0 = 0; j0 < rounds; j0 += 4) {
    uint4 d[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int g = (j0 + u) * kBlock + tid - lead;
      d[u] = (j0 + u < rounds && g >= 0) ? *reinterpret_cast<const uint4 *>(src + (size_t)g * 16u) : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int g = (j0 + u) * kBlock + tid - lead;
      if (j0 + u < rounds) {
        uint4 c = d[u];
        if (g == 0 && p == 0u)
          c.x = ~c.x; /* the initial value 0xFFFFFFFF, folded into the frame's first four bytes */
        s = crc_mul_table(mulh, s) ^ crc_raw16(slice, c);
        if (g >= 0) {
          const uint32_t w[4] = {d[u].x, d[u].y, d[u].z, d[u].w};
          const uint32_t pos0 = (uint32_t)g * 16u;
          const uint32_t s0 = stream_of(pos0, seg), s1 = stream_of(pos0 + 15u, seg);
#pragma unroll
          for (int b = 0; b < 16; b++) {
            const uint32_t st = s0 == s1 ? s0 : stream_of(pos0 + (uint32_t)b, seg);
            atomicAdd(&hist[st * 256u + ((w[b >> 2] >> (8 * (b & 3))) & 0xFFu)], 1u);
          }
        }
      }
    }
  }
  const uint32_t whole = crc_reduce_waves<kBlock>(tree, s, tid, lane_k, lane_xk); /* (one barrier: the histograms are whole behind it) */
  if (wave == 0) {
    const uint32_t reg = full > 0 ? whole : (p == 0u ? 0xFFFFFFFFu : 0u);
    const CrcClose c = crc_close_wave(slice, lds_ptr<const uint32_t>(CrcLds::o_powtab), reg, ntail, tail_byte, false, 0u, 0u, lane, lane_xk);
    if (lane == 0)
      rec[ZR_CRC] = c.st;
  }

  /* ---- what the piece holds: symbol tid over the four streams ---- */
  const uint32_t mine = hist[tid] + hist[256 + tid] + hist[512 + tid] + hist[768 + tid];
  tot[tid] = mine;
  const uint64_t mask = wave_ballot(mine != 0u);
  if (lane == 0) {
    misc[M_TOP + wave] = mask ? (uint32_t)(64 * wave + 63 - __clzll((long long)mask)) : 0xFFFFFFFFu;
    misc[M_COUNT + wave] = (uint32_t)__popcll(mask);
    misc[M_BAD + wave] = wave == 3 ? (mask != 0ull) : wave == 2 ? ((mask & ~1ull) != 0ull) : 0u; /* a byte above 0x80 */
  }
  __syncthreads();
  const uint32_t m = misc[M_COUNT] + misc[M_COUNT + 1] + misc[M_COUNT + 2] + misc[M_COUNT + 3];
  const bool bad = !Wide && (misc[M_BAD + 2] | misc[M_BAD + 3]) != 0u; /* (the wide form has no such byte) */
  uint32_t top = 0;
  for (int w = 0; w < 4; w++)
    if (misc[M_TOP + w] != 0xFFFFFFFFu)
      top = misc[M_TOP + w];
  uint32_t kind = 0u, body = n;
  if (m == 1u) {
    kind = 1u;
    body = 1u;
  } else if (m >= 2u && !bad && n >= ACHIP_ZPACK_MIN_HUF) {
    /* by (count, value) ascending: every present symbol counts the ones in front of it */
    if (tid < F::syms && mine != 0u) {
      uint32_t rank = 0;
      for (int u = 0; u < F::syms; u++) {
        const uint32_t c = tot[u];
        rank += (c != 0u && (c < mine || (c == mine && u < tid))) ? 1u : 0u;
      }
      sorted[rank] = (uint32_t)tid;
      wt[rank] = mine;
    }
    __syncthreads();
    if (tid == 0) {
      zpack_code_lengths(wt, par, m);
      uint32_t count[kMaxBits + 2];
      for (uint32_t d = 0; d < kMaxBits + 2; d++)
        count[d] = 0u;
      uint32_t maxbits = 0;
      for (uint32_t j = 0; j < m; j++) {
        clen[sorted[j]] = wt[j];
        count[wt[j]] += 1u;
        maxbits = max(maxbits, wt[j]);
      }
      uint32_t code = 0;
      for (uint32_t d = maxbits; d >= 1u; d--) { /* longest codes first; (code + count) >> 1 on the way up */
        misc[M_START + d] = code;
        code = (code + count[d]) >> 1;
      }
      misc[M_MAXBITS] = maxbits;
      if constexpr (Wide) /* the tree's bytes in the literals section; 0: the FSE form does not take this tree */
        misc[M_TREE] = top <= 128u ? 1u + (top + 1u) / 2u
                                   : zpack_fse_tree(clen, top, maxbits, lds_ptr<uint32_t>(ML::o_fse), rec + ZWR_TREE);
    }
    __syncthreads();
    const uint32_t maxbits = misc[M_MAXBITS];
    if (tid < F::syms) {
      const uint32_t l = clen[tid];
      uint32_t entry = 0u;
      if (l != 0u) {
        uint32_t code = misc[M_START + l];
        for (int u = 0; u < tid; u++)
          code += clen[u] == l ? 1u : 0u;
        entry = code | (l << 16);
      }
      rec[ZR_TABLE + tid] = entry;
    }
    /* wave w: the bits of stream w */
    uint32_t bits = hist[256 * wave + lane] * clen[lane] + hist[256 * wave + 64 + lane] * clen[64 + lane];
    if constexpr (Wide)
      bits += hist[256 * wave + 128 + lane] * clen[128 + lane] + hist[256 * wave + 192 + lane] * clen[192 + lane];
    else if (lane == 0)
      bits += hist[256 * wave + 128] * clen[128];
    bits = wave_read_lane(wave_inclusive_scan(bits), 63);
    if (lane == 0)
      misc[M_SIZE + wave] = bits / 8u + 1u; /* + the end mark, padded to a byte */
    __syncthreads();
    if (tid == 0) {
      uint32_t tree = 1u + (top + 1u) / 2u;
      if constexpr (Wide)
        tree = misc[M_TREE];
      const uint32_t csize = tree + 6u + misc[M_SIZE] + misc[M_SIZE + 1] + misc[M_SIZE + 2] + misc[M_SIZE + 3];
      const uint32_t fmt = (n < 1024u && csize < 1024u) ? 1u : (n < 16384u && csize < 16384u) ? 2u : 3u;
      const uint32_t blk = 2u + fmt + csize + 1u;
      rec[ZR_CSIZE] = csize;
      rec[ZR_FMT] = fmt;
      rec[ZR_MAXBITS] = maxbits;
      for (int w = 0; w < 4; w++)
        rec[ZR_STREAM + w] = misc[M_SIZE + w];
      if constexpr (Wide)
        rec[ZWR_TREELEN] = tree;
      misc[M_KIND] = (blk < n && (!Wide || tree != 0u)) ? blk : 0u;
    }
    __syncthreads();
    if (misc[M_KIND] != 0u) {
      kind = 2u;
      body = misc[M_KIND];
    }
  }
  if (tid == 0) {
    rec[ZR_KIND] = kind;
    rec[ZR_N] = n;
    rec[ZR_BODY] = body;
    rec[ZR_TOP] = top;
    rec[ZR_RLE] = top;
  }
}

/* ONE workgroup: the frame rule, the layout, the frame checksums.  Piece: bytes of a frame per block (the sequence form cuts finer). */
template <int RecWords = ACHIP_ZPACK_REC_WORDS, uint32_t Piece = ACHIP_ZPACK_PIECE>
__global__ void __launch_bounds__(ACHIP_ZPACK_BLOCK)
    zpack_plan_kernel(const uint32_t *__restrict__ len, int n_frames, uint32_t pieces, uint32_t *__restrict__ scratch, uint64_t capacity,
                      uint64_t *__restrict__ off_out, uint32_t *__restrict__ len_out, uint32_t *__restrict__ crc_out) {
  const int tid = (int)threadIdx.x;
  uint32_t *frm = scratch + (size_t)n_frames * pieces * RecWords;
  unsigned long long *sums = lds_ptr<unsigned long long>(0);
  const int per = (n_frames + kBlock - 1) / kBlock;
  const int lo = min(n_frames, tid * per), hi = min(n_frames, lo + per);
  unsigned long long groups = 0;
  for (int i = lo; i < hi; i++) {
    const uint32_t raw_len = len[i];
    const bool bad = raw_len >= 0xFFFFFFF0u;
    const uint32_t L = bad ? 0u : raw_len;
    const uint32_t np = bad ? 0u : max(1u, (uint32_t)(((uint64_t)L + Piece - 1u) / Piece));
    uint64_t zlen = 9u;
    uint32_t st = 0xFFFFFFFFu;
    for (uint32_t p = 0; p < np; p++) {
      uint32_t *rec = scratch + ((size_t)i * pieces + p) * RecWords;
      rec[ZR_AT] = p == 0u ? 0u : (uint32_t)zlen;
      zlen += 3u + rec[ZR_BODY];
      st = p == 0u ? rec[ZR_CRC] : crc_mulmod(st, crc_x8_pow_len(rec[ZR_N])) ^ rec[ZR_CRC];
    }
    /* the sender's rule (compress_data + COMPRESSION_RATIO_THRESHOLD 0.8 + COMPRESSION_MIN_SIZE 1024), in integers */
    const uint32_t kind = bad ? 2u : (L <= 1024u || 5u * zlen >= 4u * (uint64_t)L) ? 0u : 1u;
    const uint32_t sent = bad ? 0u : kind ? (uint32_t)zlen : L;
    uint32_t *f = frm + (size_t)i * ACHIP_ZPACK_FRM_WORDS;
    f[ZF_KIND] = kind;
    f[ZF_SENT] = sent;
    f[ZF_STATE] = st;
    f[ZF_PIECES] = np;
    f[ZF_LEN] = L;
    crc_out[i] = bad ? 0u : ~st;
    if (len_out)
      len_out[i] = bad ? raw_len : sent; /* error codes travel as they are */
    groups += ((uint64_t)sent + 15u) >> 4;
  }
  sums[tid] = groups;
  __syncthreads();
  unsigned long long below = 0, all = 0;
  for (int t = 0; t < kBlock; t++) {
    const unsigned long long v = sums[t];
    below += t < tid ? v : 0ull;
    all += v;
  }
  uint64_t off = 16ull * below;
  for (int i = lo; i < hi; i++) {
    uint32_t *f = frm + (size_t)i * ACHIP_ZPACK_FRM_WORDS;
    const uint64_t room = 16ull * (((uint64_t)f[ZF_SENT] + 15u) >> 4);
    f[ZF_OFF_LO] = (uint32_t)off;
    f[ZF_OFF_HI] = (uint32_t)(off >> 32);
    f[ZF_FITS] = off + room <= capacity ? 1u : 0u; /* whole groups travel: the last one must fit too */
    if (off_out)
      off_out[i] = off;
    off += room;
  }
  if (off_out && tid == 0)
    off_out[n_frames] = 16ull * all;
}

/* the CRC register (from 0) over LDS bytes [0, nbytes) of `img`, valid in wave 0's lanes; every thread calls (one barrier) */
__device__ inline uint32_t lds_crc_raw(const uint8_t *img, uint32_t nbytes, int tid, uint32_t lane_k, uint32_t lane_xk) {
  const uint32_t *slice = lds_ptr<const uint32_t>(CrcLds::o_slice), *mulh = lds_ptr<const uint32_t>(CrcLds::o_mulh);
  const int full = (int)(nbytes >> 4);
  const int rounds = (full + kBlock - 1) / kBlock;
  const int lead = rounds * kBlock - full;
  const uint32_t ntail = nbytes & 15u;
  const uint32_t tail_byte = (uint32_t)tid < ntail ? img[(size_t)full * 16u + (uint32_t)tid] : 0u;
  uint32_t s = 0;
  for (int j = 0; j < rounds; j++) {
    const int g = j * kBlock + tid - lead;
    const uint4 d = g >= 0 ? reinterpret_cast<const uint4 *>(img)[g] : make_uint4(0u, 0u, 0u, 0u);
    s = crc_mul_table(mulh, s) ^ crc_raw16(slice, d);
  }
  const uint32_t whole = crc_reduce_waves<kBlock>(lds_ptr<uint32_t>(CrcLds::o_tree), s, tid, lane_k, lane_xk);
  uint32_t st = 0u;
  if (wave_uniform(tid >> 6) == 0)
    st = crc_close_wave(slice, lds_ptr<const uint32_t>(CrcLds::o_powtab), full > 0 ? whole : 0u, ntail, tail_byte, false, 0u, 0u, tid & 63, lane_xk).st;
  return st;
}

/* one Huffman stream by one wave: symbols [s0, s1) of the piece -> bits at LDS byte address `at` (the image is zero) */
__device__ inline void encode_stream(const uint8_t *__restrict__ src, uint32_t s0, uint32_t s1, const uint32_t *code, uint32_t at, int lane) {
  const uint32_t b0 = s0 & ~15u;
  const uint32_t chunk = 16u * ((s1 - b0 + 16u * 64u - 1u) / (16u * 64u));
  const uint32_t a = min(s1, max(s0, b0 + (uint32_t)lane * chunk)), b = min(s1, b0 + ((uint32_t)lane + 1u) * chunk);
  uint32_t bits = 0;
  for (uint32_t g = a & ~15u; g < b; g += 16u) {
    const uint4 d = *reinterpret_cast<const uint4 *>(src + g);
    const uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (uint32_t k = 0; k < 16u; k++)
      if (g + k >= a && g + k < b)
        bits += code[(w[k >> 2] >> (8u * (k & 3u))) & 0xFFu] >> 16;
  }
  const uint32_t incl = wave_inclusive_scan(bits);
  const uint32_t total = wave_read_lane(incl, 63);
  /* the stream's last symbol lies at bit 0: this lane's run starts (with its last symbol) behind everything that follows it */
  uint32_t pos = 8u * at + (total - incl);
  uint32_t word = pos >> 5;
  uint64_t acc = 0;
  if (b > a) {
    for (uint32_t g = (b - 1u) & ~15u;; g -= 16u) {
      const uint4 d = *reinterpret_cast<const uint4 *>(src + g);
      const uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
      for (int k = 15; k >= 0; k--)
        if (g + (uint32_t)k >= a && g + (uint32_t)k < b) {
          const uint32_t e = code[(w[k >> 2] >> (8 * (k & 3))) & 0xFFu];
          if ((pos >> 5) != word) { /* (a code is at most 11 bits: one word further at most) */
            ds_or_u32(lds_base_addr() + 4u * word, (uint32_t)acc);
            acc >>= 32;
            word += 1u;
          }
          acc |= (uint64_t)(e & 0xFFFFu) << (pos - 32u * word);
          pos += e >> 16;
        }
      if (g <= (a & ~15u))
        break;
    }
    ds_or_u32(lds_base_addr() + 4u * word, (uint32_t)acc);
    if ((uint32_t)(acc >> 32) != 0u)
      ds_or_u32(lds_base_addr() + 4u * word + 4u, (uint32_t)(acc >> 32));
  }
  if (lane == 0) { /* the end mark */
    const uint32_t end = 8u * at + total;
    ds_or_u32(lds_base_addr() + 4u * (end >> 5), 1u << (end & 31u));
  }
}

/* workgroup b: frame b / pieces, piece b % pieces */
template <bool Wide = false>
__global__ void __launch_bounds__(ACHIP_ZPACK_BLOCK)
    zpack_encode_kernel(const uint8_t *__restrict__ base, uint64_t stride, int n_frames, uint32_t pieces, uint32_t *__restrict__ scratch,
                        uint8_t *__restrict__ dst, const uint4 *__restrict__ tab) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  const uint32_t i = blockIdx.x / pieces, p = blockIdx.x - i * pieces;
  if (i >= (uint32_t)n_frames)
    return;
  using F = Form<Wide>;
  using EL = ELdsT<Wide>;
  const uint32_t *f = scratch + (size_t)n_frames * pieces * F::rec_words + (size_t)i * ACHIP_ZPACK_FRM_WORDS;
  uint32_t *rec = scratch + ((size_t)i * pieces + p) * F::rec_words;
  const uint32_t fkind = f[ZF_KIND], np = f[ZF_PIECES];
  if (fkind == 2u || p >= np)
    return;
  const uint32_t n = rec[ZR_N];
  const bool fits = f[ZF_FITS] != 0u;
  const uint64_t off = (uint64_t)f[ZF_OFF_LO] | ((uint64_t)f[ZF_OFF_HI] << 32);
  const uint8_t *src = base + (size_t)i * stride + (size_t)p * kPiece;
  if (fkind == 0u) { /* as it is: whole 16-byte groups, the frame's last one included (padding the layout allows) */
    if (fits) {
      uint4 *out = reinterpret_cast<uint4 *>(dst + off + (size_t)p * kPiece);
      for (uint32_t g = (uint32_t)tid; g < (n + 15u) >> 4; g += kBlock)
        out[g] = *reinterpret_cast<const uint4 *>(src + (size_t)g * 16u);
    }
    return;
  }
  const uint32_t bkind = rec[ZR_KIND], body = rec[ZR_BODY], at = rec[ZR_AT];
  const uint32_t pre = p == 0u ? 9u : 0u, sh = at & 15u; /* piece 0 starts the frame: at == 0 */
  const uint32_t blen = pre + 3u + body, span = sh + blen;
  uint8_t *img = lds_ptr<uint8_t>(EL::o_img);
  uint32_t *code = lds_ptr<uint32_t>(EL::o_code);
  const uint32_t lane_k = CRC_LANE_TAB.k[lane], lane_xk = CRC_LANE_TAB.xk[lane];
  for (int k = tid; k < ACHIP_FRAME_CRC_TAB_BYTES / 16; k += kBlock)
    lds_ptr<uint4>(CrcLds::o_slice)[k] = tab[k];
  for (uint32_t g = (uint32_t)tid; g < (span + 15u) >> 4; g += kBlock)
    reinterpret_cast<uint4 *>(img)[g] = make_uint4(0u, 0u, 0u, 0u);
  if (tid < F::leaves)
    code[tid] = (bkind == 2u && tid < F::syms) ? rec[ZR_TABLE + tid] : 0u;
  __syncthreads();
  const uint32_t hb = sh + pre + 3u; /* where the block's body starts in the image */
  if (tid == 0) {
    if (p == 0u) { /* magic, Frame_Header_Descriptor (Single_Segment, 4-byte Frame_Content_Size), the frame's length */
      const uint32_t L = f[ZF_LEN];
      img[0] = 0x28u, img[1] = 0xB5u, img[2] = 0x2Fu, img[3] = 0xFDu, img[4] = 0xA0u;
      img[5] = (uint8_t)L, img[6] = (uint8_t)(L >> 8), img[7] = (uint8_t)(L >> 16), img[8] = (uint8_t)(L >> 24);
    }
    const uint32_t hv = (p == np - 1u ? 1u : 0u) | (bkind << 1) | ((bkind == 1u ? n : body) << 3);
    img[hb - 3u] = (uint8_t)hv, img[hb - 2u] = (uint8_t)(hv >> 8), img[hb - 1u] = (uint8_t)(hv >> 16);
  }
  if (bkind == 0u) {
    for (uint32_t k = (uint32_t)tid; k < n; k += kBlock)
      img[hb + k] = src[k];
  } else if (bkind == 1u) {
    if (tid == 0)
      img[hb] = (uint8_t)rec[ZR_RLE];
  } else {
    const uint32_t fmt = rec[ZR_FMT], csize = rec[ZR_CSIZE], top = rec[ZR_TOP], maxbits = rec[ZR_MAXBITS];
    const uint32_t hl = 2u + fmt, tree = Wide ? rec[ZWR_TREELEN] : 1u + (top + 1u) / 2u;
    const uint32_t z0 = rec[ZR_STREAM], z1 = rec[ZR_STREAM + 1], z2 = rec[ZR_STREAM + 2];
    if (tid == 0) {
      const uint64_t hv = 2ull | ((uint64_t)fmt << 2) | ((uint64_t)n << 4) | ((uint64_t)csize << (4u + (fmt == 1u ? 10u : fmt == 2u ? 14u : 18u)));
      for (uint32_t k = 0; k < hl; k++)
        img[hb + k] = (uint8_t)(hv >> (8u * k));
      if (!Wide || top <= 128u)
        img[hb + hl] = (uint8_t)(127u + top);
      uint8_t *jt = img + hb + hl + tree;
      jt[0] = (uint8_t)z0, jt[1] = (uint8_t)(z0 >> 8), jt[2] = (uint8_t)z1, jt[3] = (uint8_t)(z1 >> 8), jt[4] = (uint8_t)z2, jt[5] = (uint8_t)(z2 >> 8);
    }
    if (Wide && top > 128u) { /* the FSE form: as measure left it */
      if ((uint32_t)tid < tree)
        img[hb + hl + (uint32_t)tid] = reinterpret_cast<const uint8_t *>(rec + ZWR_TREE)[tid];
    } else if ((uint32_t)tid < (top + 1u) / 2u) { /* weights of symbols 0 .. top - 1, high nibble first */
      const uint32_t sa = 2u * (uint32_t)tid, sb = sa + 1u;
      const uint32_t la = code[sa] >> 16, lb = sb < top ? code[sb] >> 16 : 0u;
      const uint32_t wa = la ? maxbits + 1u - la : 0u, wb = lb ? maxbits + 1u - lb : 0u;
      img[hb + hl + 1u + (uint32_t)tid] = (uint8_t)((wa << 4) | wb);
    }
    __syncthreads(); /* byte stores and the ORs below may share a word */
    const uint32_t seg = (n + 3u) >> 2;
    const uint32_t zb = hb + hl + tree + 6u + (wave > 0 ? z0 : 0u) + (wave > 1 ? z1 : 0u) + (wave > 2 ? z2 : 0u);
    encode_stream(src, (uint32_t)wave * seg, min(n, ((uint32_t)wave + 1u) * seg), code, (uint32_t)EL::o_img + zb, lane);
    lds_store_fence();
  }
  __syncthreads();
  const uint32_t st = lds_crc_raw(img, span, tid, lane_k, lane_xk); /* (the sh bytes in front are zero: they leave a zero register alone) */
  if (tid == 0) {
    rec[ZR_BCRC] = st;
    rec[ZR_BLEN] = blen;
  }
  if (!fits)
    return;
  uint8_t *out = dst + off + at - sh; /* 16-byte aligned: off is, and at - sh */
  for (uint32_t g = (uint32_t)tid; g < (span + 15u) >> 4; g += kBlock) {
    const uint32_t lo = 16u * g, hi = lo + 16u;
    if (lo >= sh && hi <= span) {
      *reinterpret_cast<uint4 *>(out + lo) = reinterpret_cast<const uint4 *>(img)[g];
    } else {
      for (uint32_t k = max(lo, sh); k < min(hi, span); k++)
        out[k] = img[k];
    }
  }
}

/* one thread per frame: the header and the CRC of header || payload as sent */
template <int RecWords = ACHIP_ZPACK_REC_WORDS>
__global__ void __launch_bounds__(ACHIP_ZPACK_BLOCK)
    zpack_close_kernel(const uint32_t *__restrict__ len, int n_frames, uint32_t pieces, const uint32_t *__restrict__ scratch,
                       const uint32_t *__restrict__ dims, uint8_t *__restrict__ hdr_out, uint32_t *__restrict__ pkt_crc_out) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (i >= n_frames)
    return;
  const uint32_t *f = scratch + (size_t)n_frames * pieces * RecWords + (size_t)i * ACHIP_ZPACK_FRM_WORDS;
  const uint32_t kind = f[ZF_KIND];
  const bool bad = kind == 2u;
  const uint32_t L = bad ? 0u : len[i];
  const uint32_t w = dims && !bad ? dims[2 * i] : 0u, h = dims && !bad ? dims[2 * i + 1] : 0u;
  const uint32_t crc = bad ? 0u : ~f[ZF_STATE];
  const uint32_t field[6] = {w, h, L, kind == 1u ? f[ZF_SENT] : 0u, crc, kind == 1u ? 2u /* FRAME_FLAG_IS_COMPRESSED */ : 0u};
  uint32_t *hp = reinterpret_cast<uint32_t *>(hdr_out + (size_t)i * 24u);
  for (int k = 0; k < 6; k++)
    hp[k] = bswap32(field[k]); /* HOST_TO_NET_U32 */
  if (!pkt_crc_out)
    return;
  uint32_t st = 0xFFFFFFFFu;
  for (int k = 0; k < 24; k++)
    st = crc_byte(st, (field[k >> 2] >> (8 * (3 - (k & 3)))) & 0xFFu);
  if (kind == 1u) {
    for (uint32_t p = 0; p < f[ZF_PIECES]; p++) {
      const uint32_t *rec = scratch + ((size_t)i * pieces + p) * RecWords;
      st = crc_mulmod(st, crc_x8_pow_len(rec[ZR_BLEN])) ^ rec[ZR_BCRC];
    }
  } else {
    /* clocking the frame in from register st: st * x^(8 len) + raw(frame), and state = 0xFFFFFFFF * x^(8 len) + raw(frame) */
    st = crc_mulmod(st ^ 0xFFFFFFFFu, crc_x8_pow_len(L)) ^ f[ZF_STATE];
  }
  pkt_crc_out[i] = bad ? 0u : ~st;
}

} // namespace zpack
} // namespace achip
