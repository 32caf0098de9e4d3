/* render_inst.h -- the launch record and the entry points of the per-geometry translation units (render_inst.hip,
 * render_stream_inst.hip, render_rows_inst.hip): one `launch` and one `lds` function each.  Their names start with achipk_, not
 * achip_: they are the library's own plumbing and stay local (exports.map). */
#ifndef ACHIP_RENDER_INST_H
#define ACHIP_RENDER_INST_H

#include <stdint.h>

#include "achip_types.h"
#include "render_variants.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What a render launch can carry: the entry points of hip_launch.h fill one, every translation unit takes it whole and
 * answers hipErrorInvalidValue for a form it does not instantiate */
enum {
  ACHIPK_FORM_PLAIN = 0, /* whole frames into a slab                                                                     */
  ACHIPK_FORM_PARTS,     /* a frame shared out over ps.parts > 1 workgroups: row bands of rows_per_part text rows (frame
                            geometries), runs of blocks (stream / rows PARTS geometries, which read `ps` as one part too) */
  ACHIPK_FORM_CRC,       /* whole frames, the frame CRC riding the drain: `wire` (wire->crc required)                    */
  ACHIPK_FORM_PACK,      /* stream kernel: exact-length frames staged in LDS, into `pack`; `wire` optional; no slab       */
  ACHIPK_FORM_LENFIRST   /* stream kernel: exact-length truecolor frames of any size, into `pack`; no slab                */
};
typedef struct {
  int form, mode, comp; /* comp: some frame samples a virtual composite (the general sampler) */
  const achip_frame_t *frames;
  int n;
  const achip_lut_t *lut;
  uint8_t *out;    /* the slab; NULL for the exact-length forms                                  */
  uint64_t stride; /* of the slab; for the exact-length forms the bound of a frame's length       */
  uint32_t *len;
  const achip_uniform_t *uniform; /* NULL, or the batch's common descriptor / launch-wide flags */
  unsigned long long *prof;       /* NULL, or 8 u64 per frame (diagnostics; the rows kernel has none) */
  const achip_wire_t *wire;
  const achip_packdev_t *pack;
  achip_partsdev_t ps; /* {1, 1, NULL} unless shared out */
  int rows_per_part;
  void *stream;
} achipk_launch_t;

/* four translation units per frame geometry (render_inst.hip, -DACHIP_INST=id -DACHIP_PART=p): _p0 = modes 0..2 (mono,
 * truecolor / 256-colour foreground), _p1 = 3, 4 (16-colour foreground, truecolor background), _p2 = 5..7 (the coloured
 * half-block modes), _p3 = 8, 9 (mono half blocks, dither) */
#define ACHIP_INST_PART_OF(m) ((m) <= 2 ? 0 : (m) <= 4 ? 1 : (m) <= 7 ? 2 : 3)
#define ACHIP_INST_PARTS(Y, id) Y(id, 0) Y(id, 1) Y(id, 2) Y(id, 3)
#define Y(id, p)                                                                                                       \
  int achipk_render_inst_launch_##id##_p##p(const achipk_launch_t *l);                                                  \
  int achipk_render_inst_lds_##id##_p##p(int mode);
#define X(id, B, C, R) ACHIP_INST_PARTS(Y, id)
ACHIP_VARIANTS(X)
#undef X
#undef Y

/* the stream-kernel geometries (render_stream_inst.hip, -DACHIP_SINST=id): one unit per geometry, every form it carries */
#define X(id, W, C)                                                                                                    \
  int achipk_render_sinst_launch_##id(const achipk_launch_t *l);                                                        \
  int achipk_render_sinst_lds_##id(int mode);
ACHIP_STREAM_VARIANTS(X)
#undef X

/* the rows-kernel geometries (render_rows_inst.hip, -DACHIP_RINST=id -DACHIP_RMODE=mode): run-structured modes, whole
 * frames; one translation unit per (geometry, mode) */
#define ACHIP_RINST_MODES(Y, id) Y(id, 0) Y(id, 5) Y(id, 6) Y(id, 7) Y(id, 8) /* mono, the four half-block modes */
#define Y(id, m)                                                                                                       \
  int achipk_render_rinst_launch_##id##_m##m(const achipk_launch_t *l);                                                 \
  int achipk_render_rinst_lds_##id##_m##m(int mode);
#define X(id, W, C) ACHIP_RINST_MODES(Y, id)
ACHIP_ROWS_VARIANTS(X)
#undef X
#undef Y

/* a geometry's units as one: the unit of the launch's mode */
#define YL(id, p) case p: return achipk_render_inst_launch_##id##_p##p(l);
#define ZL(id, p) case p: return achipk_render_inst_lds_##id##_p##p(mode);
#define X(id, B, C, R)                                                                                                 \
  static inline int achipk_render_inst_launch_##id(const achipk_launch_t *l) {                                          \
    switch (ACHIP_INST_PART_OF(l->mode)) { ACHIP_INST_PARTS(YL, id) }                                                  \
    return 1; /* hipErrorInvalidValue */                                                                               \
  }                                                                                                                    \
  static inline int achipk_render_inst_lds_##id(int mode) {                                                             \
    switch (ACHIP_INST_PART_OF(mode)) { ACHIP_INST_PARTS(ZL, id) }                                                     \
    return -1;                                                                                                         \
  }
ACHIP_VARIANTS(X)
#undef X
#undef YL
#undef ZL
#define YL(id, m) case m: return achipk_render_rinst_launch_##id##_m##m(l);
#define ZL(id, m) case m: return achipk_render_rinst_lds_##id##_m##m(mode);
#define X(id, W, C)                                                                                                    \
  static inline int achipk_render_rinst_launch_##id(const achipk_launch_t *l) {                                         \
    switch (l->mode) { ACHIP_RINST_MODES(YL, id) }                                                                     \
    return 1; /* hipErrorInvalidValue */                                                                               \
  }                                                                                                                    \
  static inline int achipk_render_rinst_lds_##id(int mode) {                                                            \
    switch (mode) { ACHIP_RINST_MODES(ZL, id) }                                                                        \
    return -1;                                                                                                         \
  }
ACHIP_ROWS_VARIANTS(X)
#undef X
#undef YL
#undef ZL

#ifdef __cplusplus
}
#endif
#endif
