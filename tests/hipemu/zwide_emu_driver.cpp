/* zwide_emu_driver.cpp -- the wide form of the zhuf wire pass (ascii-chat_amd/csrc/zpack_kernels.hpp: Form<true>) under the
 * fiber emulator, launched as zpack.hip launches it.  TESTS ONLY. */
#define ACHIP_FRAME_KERNEL_ONLY
#include "zpack_kernels.hpp"

static const uint4 *crc_tab_256() {
  static uint32_t *t = nullptr;
  if (!t) {
    t = (uint32_t *)aligned_alloc(16, ACHIP_FRAME_CRC_TAB_BYTES);
    hipemu::launch(dim3(1), dim3(256), ACHIP_FRAME_CRC_TAB_BYTES, [&] { achip::crc_frame_tables_init_kernel<256>(t); });
  }
  return reinterpret_cast<const uint4 *>(t);
}

extern "C" uint32_t emu_zwide_piece() { return ACHIP_ZPACK_PIECE; }

extern "C" uint32_t emu_zwide_rec_words() { return ACHIP_ZPACK_WIDE_REC_WORDS; }

extern "C" size_t emu_zwide_scratch_bytes(uint32_t max_len, int n) { return achip_zpack_wide_scratch_bytes(max_len, n); }

extern "C" void emu_zwide(const uint8_t *base, uint64_t stride, const uint32_t *len, uint32_t max_len, int n, const uint32_t *dims,
                          uint32_t *crc_out, uint8_t *hdr_out, uint32_t *pkt_crc_out, uint8_t *dst, uint64_t capacity, uint64_t *off_out,
                          uint32_t *len_out, uint32_t *scratch) {
  namespace z = achip::zpack;
  constexpr int rec = ACHIP_ZPACK_WIDE_REC_WORDS;
  const uint4 *tab = crc_tab_256();
  const uint32_t pieces = achip_zpack_pieces(max_len);
  const uint32_t max_piece = max_len < ACHIP_ZPACK_PIECE ? max_len : ACHIP_ZPACK_PIECE;
  const dim3 grid((unsigned)n * pieces), block(ACHIP_ZPACK_BLOCK);
  hipemu::launch(grid, block, z::MLdsT<true>::bytes, [&] { z::zpack_measure_kernel<true>(base, stride, len, n, pieces, scratch, tab); });
  hipemu::launch(dim3(1), block, 8 * ACHIP_ZPACK_BLOCK,
                 [&] { z::zpack_plan_kernel<rec>(len, n, pieces, scratch, capacity, off_out, len_out, crc_out); });
  hipemu::launch(grid, block, z::ELdsT<true>::bytes(max_piece), [&] { z::zpack_encode_kernel<true>(base, stride, n, pieces, scratch, dst, tab); });
  hipemu::launch(dim3(((unsigned)n + ACHIP_ZPACK_BLOCK - 1u) / ACHIP_ZPACK_BLOCK), block, 0,
                 [&] { z::zpack_close_kernel<rec>(len, n, pieces, scratch, dims, hdr_out, pkt_crc_out); });
}
