/*
 * zseq_kernels.hpp -- the sequence form of the zstd wire pass ("zseq"): the frame is cut every ACHIP_ZSEQ_PIECE
 * bytes into blocks, a block's bytes are parsed greedily into matches of the 64 bytes in front of them (across the block cut,
 * never across the frame's start), the unmatched bytes travel as the wide form's literals section (zpack_kernels.hpp, or raw
 * literals where that is no shorter) and the matches as a sequences section coded with zstd's predefined FSE tables.  The frame
 * header, the frame rule, RLE and raw blocks are the zhuf forms'.  tests/zseq_ref.py restates every byte.
 *
 * Four launches on one stream, one 256-thread workgroup per (frame, piece) in the two that touch the bytes:
 *   build   the piece and the 64 bytes in front of it -> LDS (16-byte loads, the CRC-32C register of the original bytes in the
 *           same read); per position the longest match among distances 1 .. 64 (a candidate's 4-byte word is compared before it
 *           is extended; the smallest distance among equals; at most 130 bytes, never past the block's end); the greedy parse by
 *           pointer jumping over next[i] (i + match or i + 1); literals and sequences compacted by a scan; the literals' code
 *           lengths, codes and tree by the wide form's routines; the three FSE state chains walked by one wave each (the
 *           table one entry per lane, read by the wave-uniform state), last sequence first; a scan of the sequences' bit counts places every one of them, the bits are ORed into an LDS image
 *           of the body as the Huffman streams are.  A compressed block's body -> its slot in scratch; record -> scratch.
 *   plan    zpack_plan_kernel with this form's piece size.
 *   place   the image of the block at the destination's phase: frame header (piece 0), block header, the body from its slot
 *           (raw: the piece's bytes, RLE: one byte), checksummed and drained as zpack_encode_kernel does.
 *   close   zpack_close_kernel.
 * The slab is read once for a compressed block (twice for a raw one and a frame sent as it is); the bodies are read back once.
 * Scratch: achip_zseq_scratch_bytes (zpack.h) -- 64 bytes per piece, 32 per frame, and a slot of min(piece, max_len) bytes per
 * piece.  Nothing is stored at or behind dst + capacity.
 */
#pragma once

#include "zpack_kernels.hpp"

namespace achip {
namespace zseq {

using namespace achip::zpack;

constexpr uint32_t kSeqPiece = ACHIP_ZSEQ_PIECE;
constexpr uint32_t kWindow = 64u;    /* distances tried */
constexpr uint32_t kMaxMatch = 130u; /* Match_Length code 42 is the last one used */
constexpr uint32_t kMinMatch = 4u;

/* zstd's predefined coding tables (FSE_buildCTable over the default distributions) and the code tables, 512 words:
 * stateTable of LL (64), ML (64), OF (32); deltaNbBits and deltaFindState per symbol, LL at +0, ML at +36, OF at +89;
 * baseline | extra bits << 24 per Literals_Length and Match_Length code. */
enum { T_ST = 0, T_DNB = 160, T_DFS = 288, T_LLX = 416, T_MLX = 452, T_WORDS = 512 };
struct SeqTab {
  uint32_t w[T_WORDS];
};
constexpr void seq_fill_table(SeqTab &t, const int *prob, int count, int log, int st_at, int sym_at) {
  const int size = 1 << log, step = (size >> 1) + (size >> 3) + 3;
  int cell[64] = {}, cumul[64] = {};
  int high = size - 1;
  for (int s = 0; s < count; s++) /* "less than 1": one cell each from the top down */
    if (prob[s] < 0)
      cell[high--] = s;
  int pos = 0, total = 0;
  for (int s = 0; s < count; s++) {
    for (int k = 0; k < prob[s]; k++) {
      cell[pos] = s;
      do
        pos = (pos + step) & (size - 1);
      while (pos > high);
    }
    const int n = prob[s] < 0 ? 1 : prob[s];
    cumul[s] = total;
    if (n == 1) {
      t.w[T_DNB + sym_at + s] = (uint32_t)((log << 16) - size);
      t.w[T_DFS + sym_at + s] = (uint32_t)(total - 1);
    } else {
      int hb = 0;
      while (((n - 1) >> (hb + 1)) != 0)
        hb++;
      const int b = log - hb;
      t.w[T_DNB + sym_at + s] = (uint32_t)((b << 16) - (n << b));
      t.w[T_DFS + sym_at + s] = (uint32_t)(total - n);
    }
    total += n;
  }
  for (int u = 0; u < size; u++)
    t.w[T_ST + st_at + cumul[cell[u]]++] = (uint32_t)(size + u);
}
constexpr SeqTab seq_make_tab() {
  SeqTab t = {};
  const int ll[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
  const int ml[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                      1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
  const int of[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
  seq_fill_table(t, ll, 36, 6, 0, 0);
  seq_fill_table(t, ml, 53, 6, 64, 36);
  seq_fill_table(t, of, 29, 5, 128, 89);
  const int ll_bits[20] = {1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
  const int ml_bits[21] = {1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
  uint32_t base = 16u;
  for (int c = 0; c < 36; c++) {
    const uint32_t bits = c < 16 ? 0u : (uint32_t)ll_bits[c - 16];
    t.w[T_LLX + c] = (c < 16 ? (uint32_t)c : base) | (bits << 24);
    if (c >= 16)
      base += 1u << bits;
  }
  base = 35u;
  for (int c = 0; c < 53; c++) {
    const uint32_t bits = c < 32 ? 0u : (uint32_t)ml_bits[c - 32];
    t.w[T_MLX + c] = (c < 32 ? (uint32_t)c + 3u : base) | (bits << 24);
    if (c >= 32)
      base += 1u << bits;
  }
  return t;
}
__device__ const SeqTab SEQ_TAB = seq_make_tab();
static_assert(seq_make_tab().w[T_LLX + 35] == (65536u | (16u << 24)) && seq_make_tab().w[T_MLX + 52] == (65539u | (16u << 24)) &&
                  seq_make_tab().w[T_MLX + 43] == (131u | (7u << 24)),
              "the baselines follow from the extra bits");

/* LDS of the build kernel, in the order of its phases.  The checksum's tables are dead once the piece's register is closed:
 * the pointer-jumping arrays take their place, and once the parse is known the literals and the sequences take the first of
 * those, the literals' code builder (the MLdsT<true> arrays, 12288 bytes) and the code table the second.  The sequences'
 * codes and state bits then take the place of the piece and its per-position matches, the body's image that of the marks. */
template <uint32_t P>
struct BLds {
  static constexpr int o_ja = 0;                           /* uint16 [P + 1] twice: next^(2^k) */
  static constexpr int o_jb = o_ja + 2 * ((int)P + 16);
  static constexpr int o_lit = o_ja;                       /* ... then: the literals */
  static constexpr int o_seq = o_lit + (int)P + 16;        /* uint32 [P / 4]: literals in front | match << 16 | distance << 24 */
  static constexpr int o_hist = o_jb;                      /* ... and: uint32 [4][256] per stream */
  static constexpr int o_tot = o_hist + 4096;              /* uint32 [256] */
  static constexpr int o_sorted = o_tot + 1024;            /* uint32 [256] */
  static constexpr int o_wt = o_sorted + 1024;             /* uint32 [512] */
  static constexpr int o_par = o_wt + 2048;                /* uint32 [512] */
  static constexpr int o_len = o_par + 2048;               /* uint32 [256] */
  static constexpr int o_fse = o_len + 1024;               /* uint32 [192] */
  static constexpr int o_code = o_fse + 768;               /* uint32 [256]: code | length << 16 */
  static constexpr int a_jump = 4 * ((int)P + 16), a_code = o_code + 1024, a_crc = CrcLds::bytes;
  static constexpr int o_tab = (a_jump > a_code ? (a_jump > a_crc ? a_jump : a_crc) : (a_code > a_crc ? a_code : a_crc)); /* SeqTab */
  static constexpr int o_misc = o_tab + 4 * T_WORDS;       /* uint32 [64]: M_* of zpack_kernels.hpp and X_* below */
  static constexpr int o_ftree = o_misc + 256;             /* uint32 [32]: the FSE form of the literals' tree */
  static constexpr int o_buf = o_ftree + 128;              /* the 64 bytes in front of the piece, the piece */
  static constexpr int o_ml = o_buf + 64 + (int)P + 16;    /* uint16 [P]: match | distance << 8 per position */
  static constexpr int o_scode = o_buf;                    /* ... then: uint32 [P / 4]: LL code | ML code << 8 | OF code << 16 */
  static constexpr int o_sb = o_scode + (int)P;            /* uint16 [3][P / 4]: state bits | their count << 8, per chain */
  static constexpr int o_vis = o_ml + 2 * (int)P;          /* uint8 [P + 1]: the parse passes here */
  static constexpr int o_img = o_vis;                      /* ... then the body's image (shorter than the piece) */
  static constexpr int bytes = o_vis + (int)P + 16;
  static_assert(o_seq + (int)P <= o_jb && o_sb + 3 * (int)P / 2 <= o_vis, "what takes an array's place fits in it");
};
enum { X_DIFF = 44, X_WSUM = 48 /* [4] */, X_FINAL = 52 /* [3] */ };
static_assert(2 * BLds<kSeqPiece>::bytes <= 160 * 1024, "two workgroups of the build kernel share the LDS of a CU");
static_assert(BLds<kSeqPiece>::o_buf % 16 == 0 && BLds<kSeqPiece>::o_lit % 16 == 0 && BLds<kSeqPiece>::o_img % 16 == 0 && BLds<kSeqPiece>::o_jb % 16 == 0,
              "16-byte groups");

/* exclusive prefix of v over the workgroup's threads, and the total; every thread calls (two barriers) */
__device__ inline uint32_t block_exclusive_scan(uint32_t v, uint32_t *wsum, int lane, int wave, uint32_t *total) {
  const uint32_t incl = wave_inclusive_scan(v);
  if (lane == 63)
    wsum[wave] = incl;
  __syncthreads();
  uint32_t below = 0, all = 0;
  for (int w = 0; w < kBlock / 64; w++) {
    const uint32_t s = wsum[w];
    below += w < wave ? s : 0u;
    all += s;
  }
  __syncthreads();
  *total = all;
  return below + incl - v;
}

/* an LSB-first bit writer into a zeroed LDS image through ds_or_b32; pos: bit address from the start of LDS */
struct LdsBits {
  uint64_t acc;
  uint32_t pos, word;
  __device__ inline void start(uint32_t at) {
    pos = at;
    word = at >> 5;
    acc = 0;
  }
  __device__ inline void put(uint32_t v, uint32_t nb) { /* nb <= 32 */
    if ((pos >> 5) != word) {
      ds_or_u32(lds_base_addr() + 4u * word, (uint32_t)acc);
      acc >>= 32;
      word += 1u;
    }
    acc |= (uint64_t)v << (pos - 32u * word);
    pos += nb;
  }
  __device__ inline void flush() {
    if ((uint32_t)acc != 0u)
      ds_or_u32(lds_base_addr() + 4u * word, (uint32_t)acc);
    if ((uint32_t)(acc >> 32) != 0u)
      ds_or_u32(lds_base_addr() + 4u * word + 4u, (uint32_t)(acc >> 32));
  }
};

/* workgroup b: frame b / pieces, piece b % pieces.  tab: the image of crc_frame_tables_init_kernel<256>; slot: bytes of a
 * body slot (achip_zseq_slot_bytes). */
template <uint32_t P = kSeqPiece>
__global__ void __launch_bounds__(ACHIP_ZPACK_BLOCK)
    zseq_build_kernel(const uint8_t *__restrict__ base, uint64_t stride, const uint32_t *__restrict__ len, int n_frames, uint32_t pieces,
                      uint32_t *__restrict__ scratch, uint32_t slot, const uint4 *__restrict__ tab) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  const uint32_t i = blockIdx.x / pieces, p = blockIdx.x - i * pieces;
  if (i >= (uint32_t)n_frames)
    return;
  using BL = BLds<P>;
  uint32_t *rec = scratch + ((size_t)i * pieces + p) * ACHIP_ZSEQ_REC_WORDS;
  const uint32_t L = len[i];
  const uint64_t lo = (uint64_t)p * P;
  if (L >= 0xFFFFFFF0u || (p > 0u && lo >= L)) {
    if (tid == 0) {
      rec[ZR_KIND] = 3u;
      rec[ZR_N] = 0u;
      rec[ZR_BODY] = 0u;
    }
    return;
  }
  /* (a piece is no longer than its slot wherever len[i] <= max_len, as the contract has it; a caller that breaks it gets
   * wrong bytes -- the plan kernel still counts with the unclamped length -- but no store behind the slot) */
  const uint32_t n = (uint32_t)min(min((uint64_t)L - lo, (uint64_t)P), (uint64_t)slot);
  const uint8_t *src = base + (size_t)i * stride + lo;
  uint32_t *slice = lds_ptr<uint32_t>(CrcLds::o_slice), *mulh = lds_ptr<uint32_t>(CrcLds::o_mulh), *tree = lds_ptr<uint32_t>(CrcLds::o_tree);
  uint32_t *stab = lds_ptr<uint32_t>(BL::o_tab), *misc = lds_ptr<uint32_t>(BL::o_misc);
  uint8_t *buf = lds_ptr<uint8_t>(BL::o_buf), *blk = buf + kWindow, *vis = lds_ptr<uint8_t>(BL::o_vis), *lit = lds_ptr<uint8_t>(BL::o_lit);
  uint32_t *seq = lds_ptr<uint32_t>(BL::o_seq), *code = lds_ptr<uint32_t>(BL::o_code);
  uint16_t *ml = lds_ptr<uint16_t>(BL::o_ml);
  const uint32_t lane_k = CRC_LANE_TAB.k[lane], lane_xk = CRC_LANE_TAB.xk[lane];
  for (int k = tid; k < ACHIP_FRAME_CRC_TAB_BYTES / 16; k += kBlock)
    lds_ptr<uint4>(CrcLds::o_slice)[k] = tab[k];
  for (int k = tid; k < T_WORDS; k += kBlock)
    stab[k] = SEQ_TAB.w[k];
  if (tid < 64)
    misc[tid] = 0u;
  if (p > 0u && tid < (int)kWindow / 16) /* the window: the end of the piece in front (a piece is at least 64 bytes) */
    reinterpret_cast<uint4 *>(buf)[tid] = *reinterpret_cast<const uint4 *>(src - kWindow + 16u * (uint32_t)tid);
  const int full = (int)(n >> 4);
  const int rounds = (full + kBlock - 1) / kBlock;
  const int lead = rounds * kBlock - full;
  const uint32_t ntail = n & 15u;
  const uint32_t tail_byte = (uint32_t)tid < ntail ? src[(size_t)full * 16u + (uint32_t)tid] : 0u;
  if ((uint32_t)tid < ntail)
    blk[(uint32_t)full * 16u + (uint32_t)tid] = (uint8_t)tail_byte;
  __syncthreads();

  /* ---- the piece -> LDS, the CRC register of its bytes (zpack_measure_kernel's read) ---- */
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
        if (g >= 0)
          reinterpret_cast<uint4 *>(blk)[g] = d[u];
      }
    }
  }
  const uint32_t whole = crc_reduce_waves<kBlock>(tree, s, tid, lane_k, lane_xk); /* (one barrier: the piece is whole behind it) */
  if (wave == 0) {
    const uint32_t reg = full > 0 ? whole : (p == 0u ? 0xFFFFFFFFu : 0u);
    const CrcClose c = crc_close_wave(slice, lds_ptr<const uint32_t>(CrcLds::o_powtab), reg, ntail, tail_byte, false, 0u, 0u, lane, lane_xk);
    if (lane == 0)
      rec[ZR_CRC] = c.st;
  }
  __syncthreads(); /* the checksum's tables are done with: the arrays below take their place */
  if (n == 0u) { /* an empty frame: one raw block of no bytes */
    if (tid == 0) {
      rec[ZR_KIND] = 0u;
      rec[ZR_N] = 0u;
      rec[ZR_BODY] = 0u;
      rec[ZR_RLE] = 0u;
    }
    return;
  }

  /* ---- the longest match at every position ----
   * The 68 bytes from 64 in front of the position to 4 behind it are read as 18 aligned words and shifted into place once;
   * the four bytes at every distance are then two registers apart at most, and the 64 comparisons with the position's own
   * four bytes cost no LDS access.  Only the distances that pass are extended, four bytes per step. */
  {
    uint16_t *ja = lds_ptr<uint16_t>(BL::o_ja);
    const uint32_t first = blk[0];
    bool differs = false;
    /* the four bytes at blk[x ..], x >= -64, from two aligned words */
    auto word_at = [&](int x) {
      const uint32_t at = (uint32_t)(x + (int)kWindow);
      const uint32_t *wp = reinterpret_cast<const uint32_t *>(buf + (at & ~3u));
      return alignbit(wp[1], wp[0], 8u * (at & 3u));
    };
    for (uint32_t q = (uint32_t)tid; q < n; q += kBlock) {
      differs = differs || blk[q] != first;
      uint32_t best = 0, bd = 0;
      if (n - q >= kMinMatch) {
        const uint32_t cap = min(kMaxMatch, n - q);
        const uint32_t maxd = (uint32_t)min((uint64_t)kWindow, lo + q); /* never across the frame's start */
        const uint32_t *wp = reinterpret_cast<const uint32_t *>(buf + (q & ~3u)); /* buf[q] is blk[q - 64] */
        const uint32_t sh8 = 8u * (q & 3u);
        uint32_t u[17]; /* u[j]: blk[q - 64 + 4 j ..] */
        uint32_t prev = wp[0];
#pragma unroll
        for (int j = 0; j < 17; j++) {
          const uint32_t next = wp[j + 1];
          u[j] = alignbit(next, prev, sh8);
          prev = next;
        }
        const uint32_t w0 = u[16];
        uint64_t cand = 0; /* bit d - 1: the four bytes at distance d are the position's */
#pragma unroll
        for (int d = 1; d <= (int)kWindow; d++) {
          const int o = (int)kWindow - d;
          const uint32_t wd = (o & 3) ? alignbit(u[(o >> 2) + 1], u[o >> 2], 8u * (uint32_t)(o & 3)) : u[o >> 2];
          cand |= (uint64_t)(wd == w0 ? 1u : 0u) << (d - 1);
        }
        if (maxd < kWindow)
          cand &= (1ull << maxd) - 1ull;
        while (cand != 0ull) { /* distances ascend: the smallest one among equals stays */
          const uint32_t d = (uint32_t)__ffsll((unsigned long long)cand);
          cand &= cand - 1ull;
          uint32_t m = kMinMatch;
          while (m < cap) {
            const uint32_t x = word_at((int)(q + m)) ^ word_at((int)(q + m) - (int)d);
            if (x != 0u) {
              m += ((uint32_t)__ffs((int)x) - 1u) >> 3;
              break;
            }
            m += 4u;
          }
          m = min(m, cap); /* (the words behind blk[n] are LDS nobody wrote: they may compare as they like, the cap cuts them off) */
          if (m > best) {
            best = m;
            bd = d;
            if (best == cap)
              break;
          }
        }
      }
      ml[q] = (uint16_t)(best | (bd << 8));
      ja[q] = (uint16_t)(best >= kMinMatch ? q + best : q + 1u);
      vis[q] = q == 0u ? 1u : 0u;
    }
    if (tid == 0) {
      ja[n] = (uint16_t)n;
      vis[n] = 0u;
    }
    if (differs)
      misc[X_DIFF] = 1u;
  }
  __syncthreads();
  if (misc[X_DIFF] == 0u) { /* one byte value: RLE */
    if (tid == 0) {
      rec[ZR_KIND] = 1u;
      rec[ZR_N] = n;
      rec[ZR_BODY] = 1u;
      rec[ZR_RLE] = blk[0];
    }
    return;
  }

  /* ---- the greedy parse: positions reached from 0 in fewer than `reach` steps are marked; every round doubles it ---- */
  {
    uint16_t *cur = lds_ptr<uint16_t>(BL::o_ja), *nxt = lds_ptr<uint16_t>(BL::o_jb);
    for (uint32_t reach = 1; reach <= n; reach <<= 1) {
      for (uint32_t q0 = (uint32_t)tid; q0 <= n; q0 += 8u * kBlock) { /* eight positions' loads in flight, then their stores */
        uint32_t j[8], jj[8], v[8];
#pragma unroll
        for (uint32_t e = 0; e < 8u; e++) {
          const uint32_t q = q0 + e * kBlock;
          j[e] = q <= n ? cur[q] : 0u;
          v[e] = q <= n ? vis[q] : 0u;
        }
#pragma unroll
        for (uint32_t e = 0; e < 8u; e++)
          jj[e] = cur[j[e]];
#pragma unroll
        for (uint32_t e = 0; e < 8u; e++) {
          const uint32_t q = q0 + e * kBlock;
          if (q <= n) {
            if (v[e] != 0u)
              vis[j[e]] = 1u;
            nxt[q] = (uint16_t)jj[e];
          }
        }
      }
      __syncthreads();
      uint16_t *t = cur;
      cur = nxt;
      nxt = t;
    }
  }

  /* ---- literals and sequences, in order ---- */
  uint32_t *hist = lds_ptr<uint32_t>(BL::o_hist), *tot = lds_ptr<uint32_t>(BL::o_tot), *sorted = lds_ptr<uint32_t>(BL::o_sorted);
  uint32_t *wt = lds_ptr<uint32_t>(BL::o_wt), *par = lds_ptr<uint32_t>(BL::o_par), *clen = lds_ptr<uint32_t>(BL::o_len);
  uint32_t nlit, nseq;
  {
    const uint32_t per = (n + kBlock - 1u) / kBlock, q0 = min(n, (uint32_t)tid * per), q1 = min(n, q0 + per);
    uint32_t cnt = 0;
    for (uint32_t q = q0; q < q1; q++)
      if (vis[q] != 0u)
        cnt += (ml[q] & 0xFFu) >= kMinMatch ? 0x10000u : 1u;
    for (int k = tid; k < 1024; k += kBlock) /* (the jump arrays are done with) */
      hist[k] = 0u;
    clen[tid] = 0u;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan(cnt, misc + X_WSUM, lane, wave, &total);
    nlit = total & 0xFFFFu, nseq = total >> 16;
    uint32_t li = ex & 0xFFFFu, si = ex >> 16;
    for (uint32_t q = q0; q < q1; q++)
      if (vis[q] != 0u) {
        const uint32_t e = ml[q];
        if ((e & 0xFFu) >= kMinMatch)
          seq[si++] = li | ((e & 0xFFu) << 16) | ((e >> 8) << 24);
        else
          lit[li++] = blk[q];
      }
  }
  __syncthreads();

  /* ---- the literals section: the wide form's over the literals where it exists and is shorter than the raw one ---- */
  const uint32_t seg = (nlit + 3u) >> 2;
  for (uint32_t k = (uint32_t)tid; k < nlit; k += kBlock)
    atomicAdd(&hist[stream_of(k, seg) * 256u + lit[k]], 1u);
  __syncthreads();
  const uint32_t mine = hist[tid] + hist[256 + tid] + hist[512 + tid] + hist[768 + tid];
  tot[tid] = mine;
  {
    const uint64_t mask = wave_ballot(mine != 0u);
    if (lane == 0) {
      misc[M_TOP + wave] = mask ? (uint32_t)(64 * wave + 63 - __clzll((long long)mask)) : 0xFFFFFFFFu;
      misc[M_COUNT + wave] = (uint32_t)__popcll(mask);
    }
  }
  __syncthreads();
  const uint32_t m = misc[M_COUNT] + misc[M_COUNT + 1] + misc[M_COUNT + 2] + misc[M_COUNT + 3];
  uint32_t top = 0;
  for (int w = 0; w < 4; w++)
    if (misc[M_TOP + w] != 0xFFFFFFFFu)
      top = misc[M_TOP + w];
  const uint32_t raw_head = nlit < 32u ? 1u : nlit < 4096u ? 2u : 3u;
  uint32_t lit_len = raw_head + nlit, fmt = 0u, csize = 0u, tree_len = 0u, maxbits = 0u;
  bool huf = false;
  if (m >= 2u && nlit >= ACHIP_ZPACK_MIN_HUF) {
    if (mine != 0u) { /* by (count, value) ascending */
      uint32_t rank = 0;
      for (int u = 0; u < 256; u++) {
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
      uint32_t mb = 0;
      for (uint32_t j = 0; j < m; j++) {
        clen[sorted[j]] = wt[j];
        count[wt[j]] += 1u;
        mb = max(mb, wt[j]);
      }
      uint32_t c = 0;
      for (uint32_t d = mb; d >= 1u; d--) {
        misc[M_START + d] = c;
        c = (c + count[d]) >> 1;
      }
      misc[M_MAXBITS] = mb;
      misc[M_TREE] = top <= 128u ? 1u + (top + 1u) / 2u
                                 : zpack_fse_tree(clen, top, mb, lds_ptr<uint32_t>(BL::o_fse), lds_ptr<uint32_t>(BL::o_ftree));
    }
    __syncthreads();
    maxbits = misc[M_MAXBITS];
    {
      const uint32_t l = clen[tid];
      uint32_t entry = 0u;
      if (l != 0u) {
        uint32_t c = misc[M_START + l];
        for (int u = 0; u < tid; u++)
          c += clen[u] == l ? 1u : 0u;
        entry = c | (l << 16);
      }
      code[tid] = entry;
    }
    uint32_t bits = hist[256 * wave + lane] * clen[lane] + hist[256 * wave + 64 + lane] * clen[64 + lane] +
                    hist[256 * wave + 128 + lane] * clen[128 + lane] + hist[256 * wave + 192 + lane] * clen[192 + lane];
    bits = wave_read_lane(wave_inclusive_scan(bits), 63);
    if (lane == 0)
      misc[M_SIZE + wave] = bits / 8u + 1u; /* + the end mark, padded to a byte */
    __syncthreads();
    tree_len = misc[M_TREE];
    csize = tree_len + 6u + misc[M_SIZE] + misc[M_SIZE + 1] + misc[M_SIZE + 2] + misc[M_SIZE + 3];
    fmt = (nlit < 1024u && csize < 1024u) ? 1u : (nlit < 16384u && csize < 16384u) ? 2u : 3u;
    huf = tree_len != 0u && 2u + fmt + csize < lit_len;
    if (huf)
      lit_len = 2u + fmt + csize;
  }

  /* ---- the sequences' codes, then the three state chains from the last sequence to the first, one lane each ---- */
  uint32_t *scode = lds_ptr<uint32_t>(BL::o_scode);
  uint16_t *sb = lds_ptr<uint16_t>(BL::o_sb);
  constexpr uint32_t kSeqs = P / 4u;
  for (uint32_t k = (uint32_t)tid; k < nseq; k += kBlock) {
    const uint32_t e = seq[k], ll = (e & 0xFFFFu) - (k ? seq[k - 1u] & 0xFFFFu : 0u), mlen = (e >> 16) & 0xFFu, off = e >> 24;
    uint32_t lc = ll, mc = mlen - 3u;
    if (ll >= 16u)
      for (lc = 16u; lc < 35u && (stab[T_LLX + lc + 1u] & 0xFFFFFFu) <= ll; lc++)
        ;
    if (mlen > 34u)
      for (mc = 32u; mc < 52u && (stab[T_MLX + mc + 1u] & 0xFFFFFFu) <= mlen; mc++)
        ;
    scode[k] = lc | (mc << 8) | ((31u - (uint32_t)__clz((int)(off + 3u))) << 16);
  }
  __syncthreads();
  if (wave < 3 && nseq != 0u) { /* wave 0: LL, 1: ML, 2: OF.  The state is wave-uniform: the table lies one entry per lane and is
                                  walked with lane reads, the codes' table entries are fetched 64 sequences at a time */
    const int sym_at = wave == 0 ? 0 : wave == 1 ? 36 : 89;
    const uint32_t st_lane = stab[T_ST + (wave == 0 ? 0 : wave == 1 ? 64 : 128) + (wave == 2 ? lane & 31 : lane)];
    const uint32_t *dnb = stab + T_DNB + sym_at, *dfs = stab + T_DFS + sym_at;
    const uint32_t sh = 8u * (uint32_t)wave;
    uint16_t *out = sb + (uint32_t)wave * kSeqs;
    const uint32_t c0 = (scode[nseq - 1u] >> sh) & 0xFFu, dn0 = dnb[c0];
    const uint32_t nb0 = (dn0 + 32768u) >> 16;
    uint32_t state = wave_read_lane(st_lane, (int)(((nb0 << 16) - dn0) >> nb0) + (int)dfs[c0]);
    for (int kb = wave_uniform((int)nseq) - 2; kb >= 0; kb -= 64) { /* lane l: sequence kb - l */
      const int k = kb - lane;
      uint32_t dn_l = 0u, df_l = 0u;
      if (k >= 0) {
        const uint32_t c = (scode[k] >> sh) & 0xFFu;
        dn_l = dnb[c];
        df_l = dfs[c];
      }
      const int steps = min(64, kb + 1);
      uint32_t mine = 0u;
      for (int t = 0; t < steps; t++) {
        const uint32_t dn = wave_read_lane(dn_l, t);
        const int df = (int)wave_read_lane(df_l, t);
        const uint32_t nb = (state + dn) >> 16;
        if (lane == t)
          mine = (state & ((1u << nb) - 1u)) | (nb << 8);
        state = wave_read_lane(st_lane, (int)(state >> nb) + df);
      }
      if (k >= 0)
        out[k] = (uint16_t)mine;
    }
    if (lane == 0)
      misc[X_FINAL + wave] = state;
  }
  __syncthreads();

  /* ---- every sequence's place in the bitstream: thread t owns a run of them, the last sequence is written first ---- */
  const uint32_t sper = (nseq + kBlock - 1u) / kBlock, r0 = min(nseq, (uint32_t)tid * sper), r1 = min(nseq, r0 + sper);
  uint32_t mybits = 0;
  for (uint32_t r = r0; r < r1; r++) {
    const uint32_t k = nseq - 1u - r, c = scode[k];
    mybits += (stab[T_LLX + (c & 0xFFu)] >> 24) + (stab[T_MLX + ((c >> 8) & 0xFFu)] >> 24) + (c >> 16);
    if (r != 0u)
      mybits += (uint32_t)(sb[k] >> 8) + (uint32_t)(sb[kSeqs + k] >> 8) + (uint32_t)(sb[2u * kSeqs + k] >> 8);
  }
  uint32_t allbits;
  const uint32_t before = block_exclusive_scan(mybits, misc + X_WSUM, lane, wave, &allbits);
  const uint32_t count_bytes = nseq < 128u ? 1u : 2u;
  /* the states (6 + 5 + 6 bits) and the end mark behind the sequences' bits, padded to a byte */
  const uint32_t seq_len = nseq == 0u ? 1u : count_bytes + 1u + (allbits + 18u + 7u) / 8u;
  const uint32_t body = lit_len + seq_len;
  if (body >= n) { /* no gain: raw */
    if (tid == 0) {
      rec[ZR_KIND] = 0u;
      rec[ZR_N] = n;
      rec[ZR_BODY] = n;
      rec[ZR_RLE] = 0u;
    }
    return;
  }

  /* ---- the body's image: byte stores first, then the bits ---- */
  uint8_t *img = lds_ptr<uint8_t>(BL::o_img);
  for (uint32_t g = (uint32_t)tid; g < (body + 15u) >> 4; g += kBlock)
    reinterpret_cast<uint4 *>(img)[g] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();
  const uint32_t hl = 2u + fmt;
  const uint32_t z0 = misc[M_SIZE], z1 = misc[M_SIZE + 1], z2 = misc[M_SIZE + 2];
  if (huf) {
    if (tid == 0) {
      const uint64_t hv = 2ull | ((uint64_t)fmt << 2) | ((uint64_t)nlit << 4) | ((uint64_t)csize << (4u + (fmt == 1u ? 10u : fmt == 2u ? 14u : 18u)));
      for (uint32_t k = 0; k < hl; k++)
        img[k] = (uint8_t)(hv >> (8u * k));
      if (top <= 128u)
        img[hl] = (uint8_t)(127u + top);
      uint8_t *jt = img + hl + tree_len;
      jt[0] = (uint8_t)z0, jt[1] = (uint8_t)(z0 >> 8), jt[2] = (uint8_t)z1, jt[3] = (uint8_t)(z1 >> 8), jt[4] = (uint8_t)z2, jt[5] = (uint8_t)(z2 >> 8);
    }
    if (top > 128u) { /* the FSE form, as zpack_fse_tree left it */
      if ((uint32_t)tid < tree_len)
        img[hl + (uint32_t)tid] = lds_ptr<const uint8_t>(BL::o_ftree)[tid];
    } else if ((uint32_t)tid < (top + 1u) / 2u) { /* weights of symbols 0 .. top - 1, high nibble first */
      const uint32_t sa = 2u * (uint32_t)tid, sbb = sa + 1u;
      const uint32_t la = code[sa] >> 16, lb = sbb < top ? code[sbb] >> 16 : 0u;
      const uint32_t wa = la ? maxbits + 1u - la : 0u, wb = lb ? maxbits + 1u - lb : 0u;
      img[hl + 1u + (uint32_t)tid] = (uint8_t)((wa << 4) | wb);
    }
  } else {
    if (tid == 0) {
      const uint32_t hv = raw_head == 1u ? nlit << 3 : raw_head == 2u ? (nlit << 4) | 4u : (nlit << 4) | 12u;
      for (uint32_t k = 0; k < raw_head; k++)
        img[k] = (uint8_t)(hv >> (8u * k));
    }
    for (uint32_t k = (uint32_t)tid; k < nlit; k += kBlock)
      img[raw_head + k] = lit[k];
  }
  if (tid == 0 && nseq != 0u) { /* the sequence count; the modes byte stays 0: three predefined tables */
    if (nseq < 128u) {
      img[lit_len] = (uint8_t)nseq;
    } else {
      img[lit_len] = (uint8_t)((nseq >> 8) + 0x80u);
      img[lit_len + 1u] = (uint8_t)nseq;
    }
  }
  __syncthreads(); /* byte stores and the ORs below may share a word */
  if (huf) {
    const uint32_t zb = hl + tree_len + 6u + (wave > 0 ? z0 : 0u) + (wave > 1 ? z1 : 0u) + (wave > 2 ? z2 : 0u);
    encode_stream(lit, (uint32_t)wave * seg, min(nlit, ((uint32_t)wave + 1u) * seg), code, (uint32_t)BL::o_img + zb, lane);
  }
  if (nseq != 0u) {
    const uint32_t bit0 = 8u * ((uint32_t)BL::o_img + lit_len + count_bytes + 1u);
    LdsBits w;
    w.start(bit0 + before);
    for (uint32_t r = r0; r < r1; r++) {
      const uint32_t k = nseq - 1u - r, c = scode[k], e = seq[k];
      const uint32_t ll = (e & 0xFFFFu) - (k ? seq[k - 1u] & 0xFFFFu : 0u), mlen = (e >> 16) & 0xFFu, ov = (e >> 24) + 3u;
      const uint32_t lx = stab[T_LLX + (c & 0xFFu)], mx = stab[T_MLX + ((c >> 8) & 0xFFu)], oc = c >> 16;
      if (r != 0u) { /* the states take this sequence's codes: OF, ML, LL */
        const uint32_t so = sb[2u * kSeqs + k], sm = sb[kSeqs + k], sl = sb[k];
        w.put(so & 0xFFu, so >> 8);
        w.put(sm & 0xFFu, sm >> 8);
        w.put(sl & 0xFFu, sl >> 8);
      }
      w.put(ll - (lx & 0xFFFFFFu), lx >> 24);
      w.put(mlen - (mx & 0xFFFFFFu), mx >> 24);
      w.put(ov - (1u << oc), oc);
    }
    if (r1 > r0)
      w.flush();
    if (tid == 0) { /* the states: ML, OF, LL; the end mark */
      w.start(bit0 + allbits);
      w.put((misc[X_FINAL + 1] & 63u) | ((misc[X_FINAL + 2] & 31u) << 6) | ((misc[X_FINAL] & 63u) << 11) | (1u << 17), 18u);
      w.flush();
    }
  }
  lds_store_fence();
  __syncthreads();
  uint2 *out = reinterpret_cast<uint2 *>(reinterpret_cast<uint8_t *>(scratch + (size_t)n_frames * pieces * ACHIP_ZSEQ_REC_WORDS + (size_t)n_frames * ACHIP_ZPACK_FRM_WORDS) +
                                         ((size_t)i * pieces + p) * slot);
  for (uint32_t g = (uint32_t)tid; g < (body + 7u) >> 3; g += kBlock) /* (body < n <= slot, and the slot is whole 16-byte groups) */
    out[g] = reinterpret_cast<const uint2 *>(img)[g];
  if (tid == 0) {
    rec[ZR_KIND] = 2u;
    rec[ZR_N] = n;
    rec[ZR_BODY] = body;
    rec[ZR_RLE] = 0u;
  }
}

/* LDS of the place kernel: the checksum's, the image of the block at any phase */
template <uint32_t P>
struct PLds {
  static constexpr int o_img = CrcLds::bytes;
  static constexpr size_t bytes(uint32_t max_piece) { return (size_t)o_img + (((size_t)max_piece + 9u + 3u + 15u + 15u) & ~(size_t)15u); }
};
static_assert(PLds<kSeqPiece>::o_img % 16 == 0, "the image's groups are aligned");

/* workgroup b: frame b / pieces, piece b % pieces: zpack_encode_kernel with the compressed body taken from its slot */
template <uint32_t P = kSeqPiece>
__global__ void __launch_bounds__(ACHIP_ZPACK_BLOCK)
    zseq_place_kernel(const uint8_t *__restrict__ base, uint64_t stride, int n_frames, uint32_t pieces, uint32_t *__restrict__ scratch, uint32_t slot,
                      uint8_t *__restrict__ dst, const uint4 *__restrict__ tab) {
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const uint32_t i = blockIdx.x / pieces, p = blockIdx.x - i * pieces;
  if (i >= (uint32_t)n_frames)
    return;
  using PL = PLds<P>;
  const uint32_t *f = scratch + (size_t)n_frames * pieces * ACHIP_ZSEQ_REC_WORDS + (size_t)i * ACHIP_ZPACK_FRM_WORDS;
  uint32_t *rec = scratch + ((size_t)i * pieces + p) * ACHIP_ZSEQ_REC_WORDS;
  const uint32_t fkind = f[ZF_KIND], np = f[ZF_PIECES];
  if (fkind == 2u || p >= np)
    return;
  const uint32_t n = rec[ZR_N];
  const bool fits = f[ZF_FITS] != 0u;
  const uint64_t off = (uint64_t)f[ZF_OFF_LO] | ((uint64_t)f[ZF_OFF_HI] << 32);
  const uint8_t *src = base + (size_t)i * stride + (size_t)p * P;
  if (fkind == 0u) { /* as it is: whole 16-byte groups, the frame's last one included (padding the layout allows) */
    if (fits) {
      uint4 *out = reinterpret_cast<uint4 *>(dst + off + (size_t)p * P);
      for (uint32_t g = (uint32_t)tid; g < (n + 15u) >> 4; g += kBlock)
        out[g] = *reinterpret_cast<const uint4 *>(src + (size_t)g * 16u);
    }
    return;
  }
  const uint32_t bkind = rec[ZR_KIND], body = rec[ZR_BODY], at = rec[ZR_AT];
  const uint32_t pre = p == 0u ? 9u : 0u, sh = at & 15u; /* piece 0 starts the frame: at == 0 */
  const uint32_t blen = pre + 3u + body, span = sh + blen;
  uint8_t *img = lds_ptr<uint8_t>(PL::o_img);
  const uint32_t lane_k = CRC_LANE_TAB.k[lane], lane_xk = CRC_LANE_TAB.xk[lane];
  for (int k = tid; k < ACHIP_FRAME_CRC_TAB_BYTES / 16; k += kBlock)
    lds_ptr<uint4>(CrcLds::o_slice)[k] = tab[k];
  for (uint32_t g = (uint32_t)tid; g < (span + 15u) >> 4; g += kBlock)
    reinterpret_cast<uint4 *>(img)[g] = make_uint4(0u, 0u, 0u, 0u);
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
    const uint8_t *from = reinterpret_cast<const uint8_t *>(scratch + (size_t)n_frames * pieces * ACHIP_ZSEQ_REC_WORDS + (size_t)n_frames * ACHIP_ZPACK_FRM_WORDS) +
                          ((size_t)i * pieces + p) * slot;
    for (uint32_t g = (uint32_t)tid; g < (body + 7u) >> 3; g += kBlock) {
      const uint2 d = reinterpret_cast<const uint2 *>(from)[g];
      const uint32_t w[2] = {d.x, d.y};
      for (uint32_t k = 0; k < 8u && 8u * g + k < body; k++)
        img[hb + 8u * g + k] = (uint8_t)(w[k >> 2] >> (8u * (k & 3u)));
    }
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

} // namespace zseq
} // namespace achip
