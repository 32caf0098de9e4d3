/*
 * render_inst.hip -- instantiates the frame kernel for ONE geometry (-DACHIP_INST=<variant id>): ten modes x
 * {plain, composite sampler} x {whole-frame, row-band} launches, behind one launcher that takes the launch record
 * (render_inst.h).  One translation unit per geometry so that the build runs in parallel (make -j).  Built only with
 * hipcc --offload-arch=gfx950.
 */
#include <hip/hip_runtime.h>

#include "launch_common.hpp"
#include "render_inst.h"
#define ACHIP_FRAME_KERNEL_ONLY
#include "render_kernels.hpp"
#include "render_variants.h"

#if !defined(ACHIP_INST) || !defined(ACHIP_PART)
#error "compile with -DACHIP_INST=<variant id> -DACHIP_PART=<0: modes 0..2 | 1: modes 3, 4 | 2: modes 5..7 | 3: modes 8, 9> (render_inst.h: ACHIP_INST_PART_OF)"
#endif
#define ACHIP_IN_PART(m) (ACHIP_INST_PART_OF(m) == ACHIP_PART)

namespace {

#define X(id, B, C, R)                                                                                                 \
  template <> struct Geometry<id> {                                                                                    \
    static constexpr int BLOCK = B, CAP = C, RING = R;                                                                 \
  };
template <int ID> struct Geometry;
ACHIP_VARIANTS(X)
#undef X
using G = Geometry<ACHIP_INST>;

/* row bands / the half-block modes: instantiated only where a launch can take them (render_variants.h) */
constexpr bool HAS_SPLIT = ACHIP_FRAME_VARIANT_BANDS(ACHIP_INST);
template <int MODE> constexpr bool has_mode() {
  return ACHIP_IN_PART(MODE) && (!achip::mode_is_halfblock(MODE) || ACHIP_FRAME_VARIANT_HALFBLOCK(ACHIP_INST));
}

template <int MODE, bool COMP, bool SPLIT> hipError_t launch_one(const achipk_launch_t &l, const achip_uniform_t &uni) {
  using L = achip::Lds<MODE, G::BLOCK, G::CAP, G::RING>;
  constexpr auto kern = achip::render_frames_kernel<MODE, G::BLOCK, G::CAP, G::RING, COMP, SPLIT>;
  const hipError_t e = achip::ensure_dynamic_lds<kern>(L::bytes);
  if (e != hipSuccess)
    return e;
  const int parts = SPLIT ? l.ps.parts : 1;
  hipLaunchKernelGGL(kern, dim3((unsigned)l.n * (unsigned)parts), dim3(G::BLOCK), (size_t)L::bytes, static_cast<hipStream_t>(l.stream),
                     l.frames, l.lut, l.out, l.stride, l.len, l.n, l.prof, parts, l.rows_per_part, SPLIT ? l.ps.sync : nullptr,
                     l.ps.epoch, uni);
  return hipGetLastError();
}

template <int MODE> hipError_t launch_mode(const achipk_launch_t &l, const achip_uniform_t &uni) {
  if (l.form == ACHIPK_FORM_PARTS) {
    if constexpr (HAS_SPLIT)
      return l.comp ? launch_one<MODE, true, true>(l, uni) : launch_one<MODE, false, true>(l, uni);
    else
      return hipErrorInvalidValue;
  }
  return l.comp ? launch_one<MODE, true, false>(l, uni) : launch_one<MODE, false, false>(l, uni);
}

} // namespace

#define ACHIP_CAT2(a, b) a##b
#define ACHIP_CAT(a, b) ACHIP_CAT2(a, b)

extern "C" int ACHIP_CAT(ACHIP_CAT(ACHIP_CAT(achipk_render_inst_launch_, ACHIP_INST), _p), ACHIP_PART)(const achipk_launch_t *l) {
  if (l->form != ACHIPK_FORM_PLAIN && l->form != ACHIPK_FORM_PARTS) /* (no checksum, no exact-length form in the phase kernel) */
    return (int)hipErrorInvalidValue;
  const achip_uniform_t uni = achip::launch_uniform(l->uniform);
  switch (l->mode) {
#define M(m)                                                                                                           \
  case m:                                                                                                              \
    if constexpr (has_mode<m>())                                                                                       \
      return (int)launch_mode<m>(*l, uni);                                                                             \
    else                                                                                                               \
      return (int)hipErrorInvalidValue;
    M(ACHIP_MODE_MONO)
    M(ACHIP_MODE_TRUE_FG)
    M(ACHIP_MODE_256_FG)
    M(ACHIP_MODE_16_FG)
    M(ACHIP_MODE_TRUE_BG)
    M(ACHIP_MODE_HB_TRUE)
    M(ACHIP_MODE_HB_256)
    M(ACHIP_MODE_HB_16)
    M(ACHIP_MODE_HB_MONO)
    M(ACHIP_MODE_16_DITHER_BG)
#undef M
  }
  return (int)hipErrorInvalidValue;
}

extern "C" int ACHIP_CAT(ACHIP_CAT(ACHIP_CAT(achipk_render_inst_lds_, ACHIP_INST), _p), ACHIP_PART)(int mode) {
  switch (mode) {
#define M(m)                                                                                                           \
  case m:                                                                                                              \
    return ACHIP_IN_PART(m) ? achip::Lds<m, G::BLOCK, G::CAP, G::RING>::bytes : -1;
    M(ACHIP_MODE_MONO)
    M(ACHIP_MODE_TRUE_FG)
    M(ACHIP_MODE_256_FG)
    M(ACHIP_MODE_16_FG)
    M(ACHIP_MODE_TRUE_BG)
    M(ACHIP_MODE_HB_TRUE)
    M(ACHIP_MODE_HB_256)
    M(ACHIP_MODE_HB_16)
    M(ACHIP_MODE_HB_MONO)
    M(ACHIP_MODE_16_DITHER_BG)
#undef M
  }
  return -1;
}
