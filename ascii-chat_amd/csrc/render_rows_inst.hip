/*
 * render_rows_inst.hip -- instantiates the rows kernel (render_rows.hpp) for ONE geometry and ONE mode
 * (-DACHIP_RINST=<variant id> -DACHIP_RMODE=<mode id>): {plain, composite sampler} x {plain, frame CRC riding the drain}.
 * One translation unit per (geometry, mode) so that the build runs in parallel (the seven-slot geometry's five modes in
 * one unit were the build's critical path: 55 s); render_inst.h dispatches on the mode, the unit's one launcher takes the
 * launch record.  Built only with hipcc --offload-arch=gfx950.
 */
#include <hip/hip_runtime.h>

#include "launch_common.hpp"
#include "render_inst.h"
#define ACHIP_FRAME_KERNEL_ONLY
#include "render_rows.hpp"
#include "render_variants.h"

#if !defined(ACHIP_RINST) || !defined(ACHIP_RMODE)
#error "compile with -DACHIP_RINST=<rows variant id> -DACHIP_RMODE=<mode id>"
#endif

namespace {

template <int ID> struct RGeometry;
#define X(id, W, C)                                                                                                    \
  template <> struct RGeometry<id> {                                                                                   \
    static constexpr int WAVES = W, CPL = C;                                                                           \
    static constexpr bool WIDE = ACHIP_ROWS_VARIANT_WIDE(id), PARTS = ACHIP_ROWS_VARIANT_PARTS(id);                    \
  };
ACHIP_ROWS_VARIANTS(X)
#undef X
using G = RGeometry<ACHIP_RINST>;

/* the frame CRC riding the drain (-DACHIP_ALL_GEOMETRIES builds only) / the composite sampler: render_variants.h */
constexpr bool HAS_CRC = ACHIP_ROWS_VARIANT_CRC(ACHIP_RINST), HAS_COMP = ACHIP_ROWS_VARIANT_COMP(ACHIP_RINST);

template <int MODE, bool COMP, bool CRC> hipError_t launch_one(const achipk_launch_t &l, const achip_uniform_t &uni) {
  using L = achip::RLds<MODE, G::WAVES, CRC, G::WIDE>;
  constexpr auto kern = achip::render_rows_kernel<MODE, G::WAVES, G::CPL, COMP, CRC, G::WIDE, G::PARTS>;
  hipError_t e = achip::ensure_dynamic_lds<kern>(L::bytes);
  if (e != hipSuccess)
    return e;
  /* the constant tables of <MODE>'s CRC instantiation: built at its first launch (not warmed at plan creation) */
  const uint4 *tab = nullptr;
  if constexpr (CRC) {
    e = achip::device_table<achip::crc_tables_init_kernel<L>, L::TAB_BYTES, 0>(&tab);
    if (e != hipSuccess)
      return e;
  }
  /* uni.flags carries the blocks of the launch's largest frame (achip_rows_max_blocks): the per-block words */
  const size_t lds = (size_t)((L::bytes_for(achip::stream_maxblk(uni.flags, 1)) + 15) & ~15);
  /* (PARTS: workgroup f * parts + p renders the p-th run of frame f's blocks) */
  hipLaunchKernelGGL(kern, dim3((unsigned)l.n * (unsigned)(G::PARTS ? l.ps.parts : 1)), dim3(G::WAVES * 64), lds,
                     static_cast<hipStream_t>(l.stream), l.frames, l.lut, l.out, l.stride, l.len, l.n, uni, CRC ? *l.wire : achip_wire_t{},
                     tab, l.ps);
  return hipGetLastError();
}

} // namespace

#define ACHIP_CAT2(a, b) a##b
#define ACHIP_CAT(a, b) ACHIP_CAT2(a, b)

extern "C" int ACHIP_CAT(ACHIP_CAT(ACHIP_CAT(achipk_render_rinst_launch_, ACHIP_RINST), _m), ACHIP_RMODE)(const achipk_launch_t *l) {
  const achip_partsdev_t &ps = l->ps;
  if (ps.parts < 1 || ps.parts > 64 || (ps.parts > 1 && (!G::PARTS || !ps.sync || ps.epoch == 0u)) ||
      (G::PARTS && (!ps.sync || ps.epoch == 0u))) /* (a PARTS kernel publishes to ps.sync even as one part) */
    return (int)hipErrorInvalidValue;
  if (l->mode != ACHIP_RMODE)
    return (int)hipErrorInvalidValue;
  const achip_uniform_t uni = achip::launch_uniform(l->uniform);
  switch (l->form) {
  case ACHIPK_FORM_CRC:
    if constexpr (HAS_CRC)
      return (int)(!l->wire || !l->wire->crc ? hipErrorInvalidValue
                   : l->comp                 ? launch_one<ACHIP_RMODE, true, true>(*l, uni)
                                             : launch_one<ACHIP_RMODE, false, true>(*l, uni));
    break;
  case ACHIPK_FORM_PLAIN:
  case ACHIPK_FORM_PARTS:
    if (!l->comp)
      return (int)launch_one<ACHIP_RMODE, false, false>(*l, uni);
    if constexpr (HAS_COMP)
      return (int)launch_one<ACHIP_RMODE, true, false>(*l, uni);
    break;
  }
  return (int)hipErrorInvalidValue;
}

extern "C" int ACHIP_CAT(ACHIP_CAT(ACHIP_CAT(achipk_render_rinst_lds_, ACHIP_RINST), _m), ACHIP_RMODE)(int mode) {
  switch (mode) {
#define M(m)                                                                                                           \
  case m:                                                                                                              \
    return achip::RLds<m, G::WAVES, false, G::WIDE>::bytes;
    M(ACHIP_RMODE)
#undef M
  }
  return -1;
}
