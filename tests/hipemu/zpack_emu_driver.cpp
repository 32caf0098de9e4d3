/* zpack_emu_driver.cpp -- the four kernels of the zhuf wire pass (ascii-chat_amd/csrc/zpack_kernels.hpp) under the fiber
 * emulator, launched as zpack.hip launches them.  TESTS ONLY. */
#define ACHIP_FRAME_KERNEL_ONLY
#include "zpack_kernels.hpp"

#include <vector>

static const uint4 *crc_tab_256() {
  static uint32_t *t = nullptr;
  if (!t) {
    t = (uint32_t *)aligned_alloc(16, ACHIP_FRAME_CRC_TAB_BYTES);
    hipemu::launch(dim3(1), dim3(256), ACHIP_FRAME_CRC_TAB_BYTES, [&] { achip::crc_frame_tables_init_kernel<256>(t); });
  }
  return reinterpret_cast<const uint4 *>(t);
}

extern "C" uint32_t emu_zpack_piece() { return ACHIP_ZPACK_PIECE; }

extern "C" size_t emu_zpack_scratch_bytes(uint32_t max_len, int n) { return achip_zpack_scratch_bytes(max_len, n); }

extern "C" void emu_zpack(const uint8_t *base, uint64_t stride, const uint32_t *len, uint32_t max_len, int n, const uint32_t *dims,
                          uint32_t *crc_out, uint8_t *hdr_out, uint32_t *pkt_crc_out, uint8_t *dst, uint64_t capacity, uint64_t *off_out,
                          uint32_t *len_out, uint32_t *scratch) {
  namespace z = achip::zpack;
  const uint4 *tab = crc_tab_256();
  const uint32_t pieces = achip_zpack_pieces(max_len);
  const uint32_t max_piece = max_len < ACHIP_ZPACK_PIECE ? max_len : ACHIP_ZPACK_PIECE;
  const dim3 grid((unsigned)n * pieces), block(ACHIP_ZPACK_BLOCK);
  hipemu::launch(grid, block, z::MLds::bytes, [&] { z::zpack_measure_kernel(base, stride, len, n, pieces, scratch, tab); });
  hipemu::launch(dim3(1), block, 8 * ACHIP_ZPACK_BLOCK, [&] { z::zpack_plan_kernel(len, n, pieces, scratch, capacity, off_out, len_out, crc_out); });
  hipemu::launch(grid, block, z::ELds::bytes(max_piece), [&] { z::zpack_encode_kernel(base, stride, n, pieces, scratch, dst, tab); });
  hipemu::launch(dim3(((unsigned)n + ACHIP_ZPACK_BLOCK - 1u) / ACHIP_ZPACK_BLOCK), block, 0,
                 [&] { z::zpack_close_kernel(len, n, pieces, scratch, dims, hdr_out, pkt_crc_out); });
}
