/* box.h -- the area-average downscale pass: the per-frame descriptor shared by the host C (box.c) and the kernel
 * (box_kernels.hpp), and the launcher between them (box.hip).  Not installed. */
#ifndef ACHIP_BOX_H
#define ACHIP_BOX_H

#include <stdint.h>
#include <string.h>

#include "achip_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one frame of a box batch: what the pass reads of a render descriptor (achip_frame_t), the stride resolved */
typedef struct {
  const uint8_t *src;     /* RGB24 rows, any alignment */
  int64_t src_stride;     /* bytes per source row, >= 3 * src_w */
  int32_t src_w, src_h;   /* 1..3840 x 1..2160 */
  int32_t out_w, out_h;   /* the averaged image: 1..ACHIP_BOX_MAX_OUT each */
  uint32_t flips;         /* ACHIP_OP_FLIP_X | ACHIP_OP_FLIP_Y, applied to the averaged image */
  uint32_t _pad;
} achip_box_desc_t;

/* A launch whose descriptors differ only in their source, and there by a constant pitch: the common descriptor travels in
 * the kernel arguments (frame i reads d.src + i * src_pitch), as achip_uniform_t does for the renderers. */
typedef struct {
  achip_box_desc_t d;
  int64_t src_pitch;
  uint32_t enabled;
  uint32_t _pad;
} achip_box_uniform_t;

/* why a render descriptor is refused (achip_box_desc_from_frame) */
enum { ACHIP_BOX_OK = 0, ACHIP_BOX_COMPOSITE, ACHIP_BOX_NO_SOURCE, ACHIP_BOX_SOURCE_SIZE, ACHIP_BOX_OUT_SIZE, ACHIP_BOX_STRIDE };

#define ACHIP_BOX_BLOCK 256      /* threads per workgroup: one workgroup per (frame, output row) */
#define ACHIP_BOX_MAX_SRC_W 3840 /* image_validate_dimensions: the LDS stage holds 3 * src_w column sums (45 KB) */
#define ACHIP_BOX_MAX_SRC_H 2160
#define ACHIP_BOX_MAX_OUT 16384  /* (out * src) stays far below 2^32 in the box bounds */

/* frames i < n: desc_dev[i] (device memory; unused when uniform->enabled), averaged image i at images + i * pitch
 * (3 * out_w * out_h bytes, tight rows).  max_out_h / max_src_w: the largest of the launch.  Returns a hipError_t. */
int achip_launch_box(const achip_box_desc_t *desc_dev, const achip_box_uniform_t *uniform, int n, int max_out_h, int max_src_w,
                     uint8_t *images, uint64_t pitch, void *stream);

/* one render descriptor as the pass reads it: ACHIP_BOX_OK and *d, or the refusal */
static inline int achip_box_desc_from_frame(const achip_frame_t *f, achip_box_desc_t *d) {
  if (f->comp)
    return ACHIP_BOX_COMPOSITE;
  if (!f->src)
    return ACHIP_BOX_NO_SOURCE;
  if (f->src_w <= 0 || f->src_h <= 0 || f->src_w > ACHIP_BOX_MAX_SRC_W || f->src_h > ACHIP_BOX_MAX_SRC_H)
    return ACHIP_BOX_SOURCE_SIZE;
  if (f->out_w <= 0 || f->out_h <= 0 || f->out_w > ACHIP_BOX_MAX_OUT || f->out_h > ACHIP_BOX_MAX_OUT)
    return ACHIP_BOX_OUT_SIZE;
  if (f->src_stride != 0 && f->src_stride < 3 * f->src_w)
    return ACHIP_BOX_STRIDE;
  memset(d, 0, sizeof(*d));
  d->src = f->src;
  d->src_stride = f->src_stride ? f->src_stride : 3 * f->src_w;
  d->src_w = f->src_w;
  d->src_h = f->src_h;
  d->out_w = f->out_w;
  d->out_h = f->out_h;
  d->flips = f->ops & (ACHIP_OP_FLIP_X | ACHIP_OP_FLIP_Y);
  return ACHIP_BOX_OK;
}

/* fills u for d[0..n): enabled iff every field but src is equal and src[i] == src[0] + i * pitch for one pitch (n == 1:
 * always), as achip_frames_uniform decides for the renderers.  Returns u->enabled. */
static inline int achip_box_uniform(const achip_box_desc_t *d, int n, achip_box_uniform_t *u) {
  memset(u, 0, sizeof(*u));
  if (n <= 0)
    return 0;
  const int64_t pitch = n > 1 ? (int64_t)((intptr_t)d[1].src - (intptr_t)d[0].src) : 0;
  for (int i = 1; i < n; i++) {
    achip_box_desc_t a = d[i];
    if ((int64_t)((intptr_t)a.src - (intptr_t)d[0].src) != pitch * i)
      return 0;
    a.src = d[0].src;
    if (memcmp(&a, &d[0], sizeof(a)) != 0) /* descriptors are memset by achip_box_desc_from_frame: padding is zero */
      return 0;
  }
  u->d = d[0];
  u->src_pitch = pitch;
  u->enabled = 1;
  return 1;
}

#ifdef __cplusplus
}
#endif
#endif
