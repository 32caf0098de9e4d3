/* zseq.hip -- the launcher of the sequence form of the zstd wire pass (zseq_kernels.hpp); the host side is zpack.c. */
#include <hip/hip_runtime.h>

#define ACHIP_FRAME_KERNEL_ONLY /* (crc_math.hpp brings render_kernels.hpp along: its non-template kernels live in hip_launch.hip) */
#include "zpack.h"
#include "zseq_kernels.hpp"
#include "launch_common.hpp"

namespace z = achip::zpack;
namespace q = achip::zseq;

extern "C" int achip_launch_zseq(const uint8_t *base, uint64_t stride, const uint32_t *len_dev, uint32_t max_len, int n, const uint32_t *dims_dev,
                                 uint32_t *crc_out, uint8_t *hdr_out, uint32_t *pkt_crc_out, uint8_t *dst, uint64_t dst_capacity,
                                 uint64_t *off_out, uint32_t *len_out, uint32_t *scratch, void *stream) {
  constexpr int rec = ACHIP_ZSEQ_REC_WORDS;
  constexpr uint32_t piece = ACHIP_ZSEQ_PIECE;
  if (n <= 0)
    return (int)hipSuccess;
  const uint32_t pieces = achip_zseq_pieces(max_len), slot = achip_zseq_slot_bytes(max_len);
  if (!base || !len_dev || !crc_out || !hdr_out || !dst || !scratch || (uint64_t)n * pieces > 0x7FFFFFFFull)
    return (int)hipErrorInvalidValue;
  const uint4 *tab = nullptr;
  hipError_t e = (hipError_t)achipk_frame_crc_tables(256, &tab);
  if (e != hipSuccess)
    return (int)e;
  e = achip::ensure_dynamic_lds<q::zseq_build_kernel<piece>>(q::BLds<piece>::bytes);
  if (e == hipSuccess)
    e = achip::ensure_dynamic_lds<q::zseq_place_kernel<piece>>((int)q::PLds<piece>::bytes(piece));
  if (e != hipSuccess)
    return (int)e;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)n * pieces), block(ACHIP_ZPACK_BLOCK);
  hipLaunchKernelGGL(q::zseq_build_kernel<piece>, grid, block, (size_t)q::BLds<piece>::bytes, s, base, stride, len_dev, n, pieces, scratch, slot, tab);
  hipLaunchKernelGGL((z::zpack_plan_kernel<rec, piece>), dim3(1), block, (size_t)(8 * ACHIP_ZPACK_BLOCK), s, len_dev, n, pieces, scratch, dst_capacity,
                     off_out, len_out, crc_out);
  hipLaunchKernelGGL(q::zseq_place_kernel<piece>, grid, block, q::PLds<piece>::bytes(max_len < piece ? max_len : piece), s, base, stride, n, pieces,
                     scratch, slot, dst, tab);
  hipLaunchKernelGGL(z::zpack_close_kernel<rec>, dim3(((unsigned)n + ACHIP_ZPACK_BLOCK - 1u) / ACHIP_ZPACK_BLOCK), block, 0, s, len_dev, n, pieces,
                     (const uint32_t *)scratch, dims_dev, hdr_out, pkt_crc_out);
  return (int)hipGetLastError();
}
