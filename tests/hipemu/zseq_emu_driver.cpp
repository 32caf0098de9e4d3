/* zseq_emu_driver.cpp -- the sequence form of the zstd wire pass (ascii-chat_amd/csrc/zseq_kernels.hpp) under the fiber
 * emulator, launched as zseq.hip launches it.  TESTS ONLY. */
#define ACHIP_FRAME_KERNEL_ONLY
#include "zseq_kernels.hpp"

static const uint4 *crc_tab_256() {
  static uint32_t *t = nullptr;
  if (!t) {
    t = (uint32_t *)aligned_alloc(16, ACHIP_FRAME_CRC_TAB_BYTES);
    hipemu::launch(dim3(1), dim3(256), ACHIP_FRAME_CRC_TAB_BYTES, [&] { achip::crc_frame_tables_init_kernel<256>(t); });
  }
  return reinterpret_cast<const uint4 *>(t);
}

extern "C" uint32_t emu_zseq_piece() { return ACHIP_ZSEQ_PIECE; }

extern "C" size_t emu_zseq_scratch_bytes(uint32_t max_len, int n) { return achip_zseq_scratch_bytes(max_len, n); }

/* the coding and code tables the kernels hold (zseq_kernels.hpp: SeqTab), 512 words */
extern "C" const uint32_t *emu_zseq_tables() { return achip::zseq::SEQ_TAB.w; }

extern "C" void emu_zseq(const uint8_t *base, uint64_t stride, const uint32_t *len, uint32_t max_len, int n, const uint32_t *dims,
                         uint32_t *crc_out, uint8_t *hdr_out, uint32_t *pkt_crc_out, uint8_t *dst, uint64_t capacity, uint64_t *off_out,
                         uint32_t *len_out, uint32_t *scratch) {
  namespace z = achip::zpack;
  namespace q = achip::zseq;
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
