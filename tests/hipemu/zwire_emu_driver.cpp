/* zwire_emu_driver.cpp -- the three compressed wire forms under the fiber emulator: the narrow and the wide zhuf form
 * (ascii-chat_amd/csrc/zpack_kernels.hpp: Form<Wide>) launched as zpack.hip launches them, the sequence form
 * (zseq_kernels.hpp) as zseq.hip does.  `form` is tests/zwire.py's index.  TESTS ONLY. */
#define ACHIP_FRAME_KERNEL_ONLY
#include "zseq_kernels.hpp"

namespace z = achip::zpack;
namespace q = achip::zseq;

enum { NARROW = 0, WIDE = 1, SEQ = 2 };

static const uint4 *crc_tab_256() {
  static uint32_t *t = nullptr;
  if (!t) {
    t = (uint32_t *)aligned_alloc(16, ACHIP_FRAME_CRC_TAB_BYTES);
    hipemu::launch(dim3(1), dim3(256), ACHIP_FRAME_CRC_TAB_BYTES, [&] { achip::crc_frame_tables_init_kernel<256>(t); });
  }
  return reinterpret_cast<const uint4 *>(t);
}

extern "C" uint32_t emu_zwire_piece(int form) { return form == SEQ ? ACHIP_ZSEQ_PIECE : ACHIP_ZPACK_PIECE; }

extern "C" uint32_t emu_zwide_rec_words() { return ACHIP_ZPACK_WIDE_REC_WORDS; }

/* the coding and code tables the sequence kernels hold (zseq_kernels.hpp: SeqTab), 512 words */
extern "C" const uint32_t *emu_zseq_tables() { return q::SEQ_TAB.w; }

extern "C" size_t emu_zwire_scratch_bytes(int form, uint32_t max_len, int n) {
  return form == SEQ ? achip_zseq_scratch_bytes(max_len, n) : form == WIDE ? achip_zpack_wide_scratch_bytes(max_len, n) : achip_zpack_scratch_bytes(max_len, n);
}

template <bool Wide>
static void zhuf(const uint8_t *base, uint64_t stride, const uint32_t *len, uint32_t max_len, int n, const uint32_t *dims, uint32_t *crc_out,
                 uint8_t *hdr_out, uint32_t *pkt_crc_out, uint8_t *dst, uint64_t capacity, uint64_t *off_out, uint32_t *len_out,
                 uint32_t *scratch) {
  constexpr int rec = z::Form<Wide>::rec_words;
  const uint4 *tab = crc_tab_256();
  const uint32_t pieces = achip_zpack_pieces(max_len);
  const uint32_t max_piece = max_len < ACHIP_ZPACK_PIECE ? max_len : ACHIP_ZPACK_PIECE;
  const dim3 grid((unsigned)n * pieces), block(ACHIP_ZPACK_BLOCK);
  hipemu::launch(grid, block, z::MLdsT<Wide>::bytes, [&] { z::zpack_measure_kernel<Wide>(base, stride, len, n, pieces, scratch, tab); });
  hipemu::launch(dim3(1), block, 8 * ACHIP_ZPACK_BLOCK,
                 [&] { z::zpack_plan_kernel<rec>(len, n, pieces, scratch, capacity, off_out, len_out, crc_out); });
  hipemu::launch(grid, block, z::ELdsT<Wide>::bytes(max_piece), [&] { z::zpack_encode_kernel<Wide>(base, stride, n, pieces, scratch, dst, tab); });
  hipemu::launch(dim3(((unsigned)n + ACHIP_ZPACK_BLOCK - 1u) / ACHIP_ZPACK_BLOCK), block, 0,
                 [&] { z::zpack_close_kernel<rec>(len, n, pieces, scratch, dims, hdr_out, pkt_crc_out); });
}

static void zseq(const uint8_t *base, uint64_t stride, const uint32_t *len, uint32_t max_len, int n, const uint32_t *dims, uint32_t *crc_out,
                 uint8_t *hdr_out, uint32_t *pkt_crc_out, uint8_t *dst, uint64_t capacity, uint64_t *off_out, uint32_t *len_out,
                 uint32_t *scratch) {
  constexpr int rec = ACHIP_ZSEQ_REC_WORDS;
  constexpr uint32_t piece = ACHIP_ZSEQ_PIECE;
  const uint4 *tab = crc_tab_256();
  const uint32_t pieces = achip_zseq_pieces(max_len), slot = achip_zseq_slot_bytes(max_len);
  const dim3 grid((unsigned)n * pieces), block(ACHIP_ZPACK_BLOCK);
  hipemu::launch(grid, block, q::BLds<piece>::bytes, [&] { q::zseq_build_kernel<piece>(base, stride, len, n, pieces, scratch, slot, tab); });
  hipemu::launch(dim3(1), block, 8 * ACHIP_ZPACK_BLOCK,
                 [&] { z::zpack_plan_kernel<rec, piece>(len, n, pieces, scratch, capacity, off_out, len_out, crc_out); });
  hipemu::launch(grid, block, q::PLds<piece>::bytes(max_len < piece ? max_len : piece),
                 [&] { q::zseq_place_kernel<piece>(base, stride, n, pieces, scratch, slot, dst, tab); });
  hipemu::launch(dim3(((unsigned)n + ACHIP_ZPACK_BLOCK - 1u) / ACHIP_ZPACK_BLOCK), block, 0,
                 [&] { z::zpack_close_kernel<rec>(len, n, pieces, scratch, dims, hdr_out, pkt_crc_out); });
}

extern "C" void emu_zwire(int form, const uint8_t *base, uint64_t stride, const uint32_t *len, uint32_t max_len, int n, const uint32_t *dims,
                          uint32_t *crc_out, uint8_t *hdr_out, uint32_t *pkt_crc_out, uint8_t *dst, uint64_t capacity, uint64_t *off_out,
                          uint32_t *len_out, uint32_t *scratch) {
  (form == SEQ ? zseq : form == WIDE ? zhuf<true> : zhuf<false>)(base, stride, len, max_len, n, dims, crc_out, hdr_out, pkt_crc_out, dst, capacity,
                                                                 off_out, len_out, scratch);
}
