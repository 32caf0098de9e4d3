/* rain_emu_driver.cpp -- the digital rain kernel (ascii-chat_amd/csrc/rain_kernels.hpp) under the fiber emulator, as
 * rain.hip launches it.  TESTS ONLY. */
#include "rain_kernels.hpp"

extern "C" void emu_rain(const achip_rain_desc_t *desc, int n, int table_entries, const uint8_t *src, uint64_t src_stride,
                         const uint32_t *src_len, uint8_t *dst, uint64_t dst_stride, uint32_t *dst_len) {
  hipemu::launch(dim3((unsigned)n), dim3(ACHIP_RAIN_BLOCK), achip::rain::lds_bytes(table_entries), [&] {
    achip::rain::rain_kernel(desc, table_entries, src, src_stride, src_len, dst, dst_stride, dst_len);
  });
}
