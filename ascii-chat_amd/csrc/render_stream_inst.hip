/*
 * render_stream_inst.hip -- instantiates the stream kernel (render_stream.hpp) for ONE geometry
 * (-DACHIP_SINST=<variant id>): four per-cell modes x {plain, composite sampler} and the forms render_variants.h gives the
 * geometry, behind ONE launcher that takes the launch record (render_inst.h) and switches on its form.  One translation unit
 * per geometry so that the build runs in parallel.  Built only with hipcc --offload-arch=gfx950.
 */
#include <hip/hip_runtime.h>

#include "launch_common.hpp"
#include "render_inst.h"
#define ACHIP_FRAME_KERNEL_ONLY
#include "render_stream.hpp"
#include "render_variants.h"

#ifndef ACHIP_SINST
#error "compile with -DACHIP_SINST=<stream variant id>"
#endif

namespace {

template <int ID> struct SGeometry;
#define X(id, W, C)                                                                                                    \
  template <> struct SGeometry<id> {                                                                                   \
    static constexpr int WAVES = W, CPL = C;                                                                           \
  };
ACHIP_STREAM_VARIANTS(X)
#undef X
using G = SGeometry<ACHIP_SINST>;

/* the forms this geometry carries besides the plain launch (render_variants.h): the frame CRC riding the drain, the
 * exact-length forms (PACK: frames staged in LDS, with or without the wire stage; LF: length-first), the multi-byte-palette
 * form of truecolor foreground, a frame's blocks shared out over workgroups */
constexpr bool HAS_CRC = ACHIP_STREAM_VARIANT_CRC(ACHIP_SINST), HAS_EXACT = ACHIP_STREAM_VARIANT_EXACT(ACHIP_SINST),
               HAS_U8 = ACHIP_STREAM_VARIANT_U8(ACHIP_SINST), HAS_PARTS = ACHIP_STREAM_VARIANT_PARTS(ACHIP_SINST);

/* every instantiation's launch.  What a form does not use travels empty: the slab and the stamps (the entry points leave
 * l.out / l.prof NULL for the exact-length forms), the wire record, the pack record, the parts record */
template <int MODE, bool COMP, bool CRC, int PACK = 0, bool PARTS = false, bool LF = false>
hipError_t launch_one(const achipk_launch_t &l, const achip_uniform_t &uni) {
  using L = achip::SLds<MODE, G::WAVES, G::CPL, CRC, PACK>;
  constexpr auto kern = achip::render_stream_kernel<MODE, G::WAVES, G::CPL, COMP, CRC, PACK, PARTS, LF>;
  hipError_t e = achip::ensure_dynamic_lds<kern>(L::bytes); /* (PACK: always above 48 KB -- ACHIP_PACK_FRAME_CAP alone is) */
  if (e != hipSuccess)
    return e;
  /* CRC: the constant tables of <MODE>'s instantiation, built at its first launch (not warmed at plan creation); PACK with
   * the wire stage: the library's one Horner table of the checksumming waves (warmed) */
  const uint4 *tab = nullptr;
  if constexpr (CRC)
    e = achip::device_table<achip::crc_tables_init_kernel<L>, L::TAB_BYTES, 0>(&tab);
  else if constexpr (PACK == 2)
    e = (hipError_t)achipk_frame_crc_tables(64 * achip::pack_crc_waves(G::WAVES), &tab);
  if (e != hipSuccess)
    return e;
  /* the per-block words are sized by the launch's largest frame when the host states it: a small footprint lets
   * workgroups of launches in flight on other streams share a CU.  PACK: behind them the frame's image -- as long as the
   * launch's frames can be (l.stride, the plan's bound): two 8-wave workgroups of 1080p -> 80x24 frames share a CU */
  const int maxblk = achip::stream_maxblk(uni.flags, L::EFF);
  const size_t lds = (size_t)(((PACK ? L::bytes_for_pack(maxblk, (int)l.stride) : L::bytes_for(maxblk)) + 15) & ~15);
  hipLaunchKernelGGL(kern, dim3((unsigned)l.n * (unsigned)(PARTS ? l.ps.parts : 1)), dim3(G::WAVES * 64), lds,
                     static_cast<hipStream_t>(l.stream), l.frames, l.lut, l.out, l.stride, l.len, l.n, uni, l.prof,
                     CRC || PACK == 2 ? *l.wire : achip_wire_t{}, tab, PACK || LF ? *l.pack : achip_packdev_t{},
                     PARTS ? l.ps : achip_partsdev_t{});
  return hipGetLastError();
}

/* one form in the launch's mode; M(m) says what the form launches for mode m */
#define BY_MODE(...)                                                                                                   \
  switch (l.mode) {                                                                                                    \
    M(ACHIP_MODE_TRUE_FG) M(ACHIP_MODE_256_FG) M(ACHIP_MODE_16_FG) __VA_ARGS__                                         \
  }                                                                                                                    \
  return hipErrorInvalidValue;
#define M(m)                                                                                                           \
  case m:                                                                                                              \
    return l.comp ? launch_one<m, true, CRC, 0, PARTS>(l, uni) : launch_one<m, false, CRC, 0, PARTS>(l, uni);
template <bool CRC, bool PARTS> hipError_t launch_slab(const achipk_launch_t &l, const achip_uniform_t &uni) { BY_MODE(M(ACHIP_MODE_TRUE_BG)) }
#undef M
#define M(m)                                                                                                           \
  case m:                                                                                                              \
    return l.wire ? launch_one<m, false, false, 2>(l, uni) : launch_one<m, false, false, 1>(l, uni);
template <bool = true> /* (a template: only a unit that launches it instantiates the PACK kernels) */
hipError_t launch_pack(const achipk_launch_t &l, const achip_uniform_t &uni) { BY_MODE() }
#undef M
#undef BY_MODE

} // namespace

#define ACHIP_CAT2(a, b) a##b
#define ACHIP_CAT(a, b) ACHIP_CAT2(a, b)

extern "C" int ACHIP_CAT(achipk_render_sinst_launch_, ACHIP_SINST)(const achipk_launch_t *lp) {
  const achipk_launch_t &l = *lp;
  const achip_uniform_t uni = achip::launch_uniform(l.uniform);
  const bool ascii = (uni.flags & ACHIP_UNIFORM_PALETTE_ASCII) != 0;
  switch (l.form) {
  case ACHIPK_FORM_PLAIN:
    /* truecolor foreground with a palette that holds multi-byte glyphs: an instantiation of its own (render_stream.hpp);
     * whole frames of single sources without the fused checksum (the host plans the rest elsewhere) */
    if (l.mode == ACHIP_MODE_TRUE_FG && !ascii) {
      if constexpr (HAS_U8)
        return (int)(l.comp ? hipErrorInvalidValue : launch_one<ACHIP_STREAM_MODE_TRUE_FG_U8, false, false>(l, uni));
      break;
    }
    return (int)launch_slab<false, false>(l, uni);
  case ACHIPK_FORM_CRC:
    if constexpr (HAS_CRC)
      if (l.wire && l.wire->crc && (l.mode != ACHIP_MODE_TRUE_FG || ascii))
        return (int)launch_slab<true, false>(l, uni);
    break;
  case ACHIPK_FORM_PARTS: /* (a PARTS launch without its hand-off words must not reach the kernel) */
    if constexpr (HAS_PARTS)
      if (l.ps.parts >= 2 && l.ps.parts <= 64 && l.ps.sync && l.ps.epoch != 0u)
        return (int)launch_slab<false, true>(l, uni);
    break;
  case ACHIPK_FORM_PACK:
    if constexpr (HAS_EXACT)
      if (l.pack && l.pack->dst && l.pack->cursor && (!l.wire || l.wire->crc))
        return (int)launch_pack(l, uni);
    break;
  case ACHIPK_FORM_LENFIRST: /* the lean loop run twice (render_stream.hpp LF) */
    if constexpr (HAS_EXACT)
      if (l.pack && l.pack->dst && l.pack->cursor && ascii)
        return (int)launch_one<ACHIP_MODE_TRUE_FG, false, false, 0, false, true>(l, uni);
    break;
  }
  return (int)hipErrorInvalidValue;
}

extern "C" int ACHIP_CAT(achipk_render_sinst_lds_, ACHIP_SINST)(int mode) {
  switch (mode) {
#define M(m)                                                                                                           \
  case m:                                                                                                              \
    return achip::SLds<m, G::WAVES, G::CPL>::bytes;
    M(ACHIP_MODE_TRUE_FG)
    M(ACHIP_MODE_256_FG)
    M(ACHIP_MODE_16_FG)
    M(ACHIP_MODE_TRUE_BG)
#undef M
  }
  return -1;
}
