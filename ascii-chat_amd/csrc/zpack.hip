/* zpack.hip -- the launcher of the zhuf wire pass (zpack_kernels.hpp); the host side is zpack.c. */
#include <hip/hip_runtime.h>

#define ACHIP_FRAME_KERNEL_ONLY /* (crc_math.hpp brings render_kernels.hpp along: its non-template kernels live in hip_launch.hip) */
#include "zpack.h"
#include "zpack_kernels.hpp"
#include "launch_common.hpp"

namespace z = achip::zpack;

/* the four launches of either form (zpack_kernels.hpp: Form) */
template <bool Wide>
static int launch(const uint8_t *base, uint64_t stride, const uint32_t *len_dev, uint32_t max_len, int n, const uint32_t *dims_dev,
                  uint32_t *crc_out, uint8_t *hdr_out, uint32_t *pkt_crc_out, uint8_t *dst, uint64_t dst_capacity, uint64_t *off_out,
                  uint32_t *len_out, uint32_t *scratch, void *stream) {
  using EL = z::ELdsT<Wide>;
  constexpr int rec = z::Form<Wide>::rec_words;
  if (n <= 0)
    return (int)hipSuccess;
  const uint32_t pieces = achip_zpack_pieces(max_len);
  if (!base || !len_dev || !crc_out || !hdr_out || !dst || !scratch || (uint64_t)n * pieces > 0x7FFFFFFFull)
    return (int)hipErrorInvalidValue;
  const uint4 *tab = nullptr;
  hipError_t e = (hipError_t)achipk_frame_crc_tables(256, &tab);
  if (e != hipSuccess)
    return (int)e;
  const uint32_t max_piece = max_len < ACHIP_ZPACK_PIECE ? max_len : ACHIP_ZPACK_PIECE;
  const size_t enc_lds = EL::bytes(max_piece);
  /* (the attribute is raised to the largest image once: a later launch with shorter frames asks for less) */
  e = achip::ensure_dynamic_lds<z::zpack_encode_kernel<Wide>>((int)EL::bytes(ACHIP_ZPACK_PIECE));
  if (e != hipSuccess)
    return (int)e;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)n * pieces), block(ACHIP_ZPACK_BLOCK);
  hipLaunchKernelGGL(z::zpack_measure_kernel<Wide>, grid, block, (size_t)z::MLdsT<Wide>::bytes, s, base, stride, len_dev, n, pieces, scratch, tab);
  hipLaunchKernelGGL(z::zpack_plan_kernel<rec>, dim3(1), block, (size_t)(8 * ACHIP_ZPACK_BLOCK), s, len_dev, n, pieces, scratch, dst_capacity,
                     off_out, len_out, crc_out);
  hipLaunchKernelGGL(z::zpack_encode_kernel<Wide>, grid, block, enc_lds, s, base, stride, n, pieces, scratch, dst, tab);
  hipLaunchKernelGGL(z::zpack_close_kernel<rec>, dim3(((unsigned)n + ACHIP_ZPACK_BLOCK - 1u) / ACHIP_ZPACK_BLOCK), block, 0, s, len_dev, n, pieces,
                     (const uint32_t *)scratch, dims_dev, hdr_out, pkt_crc_out);
  return (int)hipGetLastError();
}

extern "C" int achip_launch_zpack(const uint8_t *base, uint64_t stride, const uint32_t *len_dev, uint32_t max_len, int n, const uint32_t *dims_dev,
                                  uint32_t *crc_out, uint8_t *hdr_out, uint32_t *pkt_crc_out, uint8_t *dst, uint64_t dst_capacity,
                                  uint64_t *off_out, uint32_t *len_out, uint32_t *scratch, void *stream) {
  return launch<false>(base, stride, len_dev, max_len, n, dims_dev, crc_out, hdr_out, pkt_crc_out, dst, dst_capacity, off_out, len_out, scratch,
                       stream);
}

extern "C" int achip_launch_zpack_wide(const uint8_t *base, uint64_t stride, const uint32_t *len_dev, uint32_t max_len, int n,
                                       const uint32_t *dims_dev, uint32_t *crc_out, uint8_t *hdr_out, uint32_t *pkt_crc_out, uint8_t *dst,
                                       uint64_t dst_capacity, uint64_t *off_out, uint32_t *len_out, uint32_t *scratch, void *stream) {
  return launch<true>(base, stride, len_dev, max_len, n, dims_dev, crc_out, hdr_out, pkt_crc_out, dst, dst_capacity, off_out, len_out, scratch,
                      stream);
}
