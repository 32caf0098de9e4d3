/* zpack.h -- the "zhuf" wire pass: the scratch layout shared by its four kernels (zpack_kernels.hpp), and the
 * launcher (zpack.hip) between them and the host side (zpack.c).  Not installed. */
#ifndef ACHIP_ZPACK_H
#define ACHIP_ZPACK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACHIP_ZPACK_BLOCK 256
#ifndef ACHIP_ZPACK_PIECE /* (only the second emulator library of the tests defines it, smaller: tests/zpack_support.py) */
#define ACHIP_ZPACK_PIECE 131072u /* bytes of a frame per zstd block */
#endif
#ifdef __cplusplus
static_assert(ACHIP_ZPACK_PIECE % 16u == 0u && ACHIP_ZPACK_PIECE >= 16u, "blocks start a piece apart in the slab: whole 16-byte groups");
static_assert(ACHIP_ZPACK_PIECE <= 131072u, "Block_Maximum_Size");
#else
_Static_assert(ACHIP_ZPACK_PIECE % 16u == 0u && ACHIP_ZPACK_PIECE >= 16u, "blocks start a piece apart in the slab: whole 16-byte groups");
_Static_assert(ACHIP_ZPACK_PIECE <= 131072u, "Block_Maximum_Size");
#endif
#define ACHIP_ZPACK_MAX_BITS 11
#define ACHIP_ZPACK_MIN_HUF 17u   /* no compressed block is below 16 bytes: shorter pieces never gain */

/* one record per (frame, piece), then one per frame; 32-bit words */
#define ACHIP_ZPACK_REC_WORDS 160
#define ACHIP_ZPACK_FRM_WORDS 8
enum {
  ZR_KIND = 0,   /* block type: 0 raw, 1 RLE, 2 compressed; 3: the frame has no such piece */
  ZR_N = 1,      /* bytes of the piece */
  ZR_BODY = 2,   /* bytes of the block behind its 3-byte header */
  ZR_CRC = 3,    /* CRC register after the piece's bytes: from 0xFFFFFFFF for piece 0, from 0 for the others */
  ZR_STREAM = 4, /* 4 words: bytes of the four Huffman streams */
  ZR_MAXBITS = 8,
  ZR_TOP = 9,    /* the largest symbol present (its weight is implied) */
  ZR_RLE = 10,   /* the byte of an RLE block */
  ZR_CSIZE = 11, /* Compressed_Size of the literals section */
  ZR_FMT = 12,   /* its Size_Format: 1, 2, 3 */
  ZR_AT = 13,    /* where the block starts in the zhuf frame (piece 0: 0, the frame header travels with it) */
  ZR_BCRC = 14,  /* CRC register (from 0) over the block as sent */
  ZR_BLEN = 15,  /* ... and its bytes */
  ZR_TABLE = 16  /* 129 words: code | length << 16 */
};
/* the wide form's record: the words above with a table of 256 entries, then the tree as it is sent */
#define ACHIP_ZPACK_WIDE_REC_WORDS 320
enum {
  ZWR_TREELEN = 272, /* bytes of the tree description in the literals section, its header byte included (either form) */
  ZWR_TREE = 276     /* 32 words: the FSE form's bytes, header byte first (largest symbol above 128 only) */
};
enum {
  ZF_KIND = 0, /* 0: sent as it is, 1: sent as a zhuf frame, 2: a render error code */
  ZF_SENT = 1,
  ZF_OFF_LO = 2,
  ZF_OFF_HI = 3,
  ZF_FITS = 4,
  ZF_STATE = 5, /* CRC register after the original frame (from 0xFFFFFFFF) */
  ZF_PIECES = 6,
  ZF_LEN = 7 /* the original length (0 for an error code) */
};

static inline uint32_t achip_zpack_pieces(uint32_t max_len) {
  return max_len <= ACHIP_ZPACK_PIECE ? 1u : (uint32_t)(((uint64_t)max_len + ACHIP_ZPACK_PIECE - 1u) / ACHIP_ZPACK_PIECE);
}
static inline size_t achip_zpack_scratch_bytes(uint32_t max_len, int n) {
  if (n <= 0)
    return 0;
  return 4u * (size_t)n * ((size_t)achip_zpack_pieces(max_len) * ACHIP_ZPACK_REC_WORDS + ACHIP_ZPACK_FRM_WORDS);
}

static inline size_t achip_zpack_wide_scratch_bytes(uint32_t max_len, int n) {
  if (n <= 0)
    return 0;
  return 4u * (size_t)n * ((size_t)achip_zpack_pieces(max_len) * ACHIP_ZPACK_WIDE_REC_WORDS + ACHIP_ZPACK_FRM_WORDS);
}

/* ---- the sequence form ("zseq", zseq_kernels.hpp): the frame cut every ACHIP_ZSEQ_PIECE bytes, a block's matches in a 64-byte
 * window as a sequences section under the predefined tables, its other bytes as the wide form's literals section.  A piece's
 * record is the words ZR_KIND .. ZR_BLEN above (ZR_STREAM .. ZR_FMT unused); behind the records of the frames lies one slot per
 * (frame, piece) that holds a compressed block's body between the pass that builds it and the pass that places it. */
#ifndef ACHIP_ZSEQ_PIECE /* (only the second emulator library of the tests defines it, smaller) */
#define ACHIP_ZSEQ_PIECE 8192u
#endif
#ifdef __cplusplus
static_assert(ACHIP_ZSEQ_PIECE % 16u == 0u && ACHIP_ZSEQ_PIECE >= 64u && ACHIP_ZSEQ_PIECE <= 8192u, "a piece and its arrays live in LDS (zseq_kernels.hpp: BLds); the window of the next one lies inside it");
#else
_Static_assert(ACHIP_ZSEQ_PIECE % 16u == 0u && ACHIP_ZSEQ_PIECE >= 64u && ACHIP_ZSEQ_PIECE <= 8192u, "a piece and its arrays live in LDS (zseq_kernels.hpp: BLds); the window of the next one lies inside it");
#endif
#define ACHIP_ZSEQ_REC_WORDS 16
static inline uint32_t achip_zseq_pieces(uint32_t max_len) {
  return max_len <= ACHIP_ZSEQ_PIECE ? 1u : (uint32_t)(((uint64_t)max_len + ACHIP_ZSEQ_PIECE - 1u) / ACHIP_ZSEQ_PIECE);
}
/* bytes of a body slot: a compressed block is shorter than its piece */
static inline uint32_t achip_zseq_slot_bytes(uint32_t max_len) {
  return ((max_len < ACHIP_ZSEQ_PIECE ? max_len : ACHIP_ZSEQ_PIECE) + 15u) & ~15u;
}
/* records of the pieces, records of the frames, body slots */
static inline size_t achip_zseq_scratch_bytes(uint32_t max_len, int n) {
  if (n <= 0)
    return 0;
  return (size_t)n * ((size_t)achip_zseq_pieces(max_len) * (4u * ACHIP_ZSEQ_REC_WORDS + achip_zseq_slot_bytes(max_len)) + 4u * ACHIP_ZPACK_FRM_WORDS);
}

/* a form's launcher: frames i < n at base + i * stride, len_dev[i] bytes each (<= max_len): see
 * asciichat_hip_frame_packets_zpacked.  Returns a hipError_t. */
typedef int achip_zpack_launch_fn(const uint8_t *base, uint64_t stride, const uint32_t *len_dev, uint32_t max_len, int n, const uint32_t *dims_dev,
                                  uint32_t *crc_out, uint8_t *hdr_out, uint32_t *pkt_crc_out, uint8_t *dst, uint64_t dst_capacity,
                                  uint64_t *off_out, uint32_t *len_out, uint32_t *scratch, void *stream);
achip_zpack_launch_fn achip_launch_zpack;      /* the narrow form; scratch: achip_zpack_scratch_bytes */
achip_zpack_launch_fn achip_launch_zpack_wide; /* the same over all 256 byte values (asciichat_hip_frame_packets_zpacked_wide); scratch:
                                                  achip_zpack_wide_scratch_bytes */
achip_zpack_launch_fn achip_launch_zseq;       /* the sequence form (asciichat_hip_frame_packets_zpacked_seq); scratch: achip_zseq_scratch_bytes */

#ifdef __cplusplus
}
#endif
#endif
