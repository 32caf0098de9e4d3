/* yuv_math.h -- the arithmetic and the addressing of the YUV sources (include/asciichat_yuv.h states the rule and the four
 * layouts), with the pure-C checks of a source and of a set beside them: one text for the kernels (yuv_kernels.hpp), the host
 * (yuv.c), the emulator driver and the sanitizer program of the tests.  Plain C; __host__ __device__ under hipcc.  The
 * arithmetic and the I420 / UYVY layouts are the reference's convert_pixel_buffer_to_rgb24
 * (lib/video/webcam/macos/webcam_avfoundation.m:406-472).  Not installed. */
#ifndef ASCIICHAT_YUV_MATH_H
#define ASCIICHAT_YUV_MATH_H

#include "achip_desc.h"
#include "asciichat_yuv.h"

#if defined(__HIPCC__)
#define YUV_FN __host__ __device__ static inline
#else
#define YUV_FN static inline
#endif

#define YUV_MAX_SIDE 8192
#define YUV_MAX_STRIDE (1 << 24) /* exclusive */
#define YUV_MAX_FRAMES 65535
#define YUV_BLOCK 256 /* threads of every workgroup */

/* ---- the arithmetic (.m:419-425, :461-467) ---- */
/* clamp255(s >> 8) << 8 of a channel's sum s, with >> arithmetic as the reference's is: the clamp comes first -- a negative sum
 * gives 0, one of 65536 or more 255 -- and the shift never happens, the channel stands in bits 15..8.  (Written shift first,
 * hipcc 7 folds two neighbouring channels into one v_ashr_pk_u8_i32 and then reads that register as if its upper half were
 * clear, which it is not: a saturated red set bit 0 of blue.) */
YUV_FN uint32_t yuv_channel_at8(int32_t s) { return (uint32_t)(s < 0 ? 0 : s > 65535 ? 65535 : s) & 0xFF00u; }
/* (Y, U, V) -> R | G << 8 | B << 16 */
YUV_FN uint32_t yuv_rgb(uint32_t Y, uint32_t U, uint32_t V) {
  const int32_t y = 298 * ((int32_t)Y - 16) + 128, u = (int32_t)U - 128, v = (int32_t)V - 128;
  return yuv_channel_at8(y + 409 * v) >> 8 | yuv_channel_at8(y - 100 * u - 208 * v) | yuv_channel_at8(y + 516 * u) << 8;
}

/* ---- the addressing ---- */
YUV_FN int32_t yuv_chroma_w(int32_t w) { return (w + 1) / 2; }
YUV_FN int32_t yuv_chroma_h(int32_t h) { return (h + 1) / 2; }
YUV_FN int yuv_is_packed(int32_t format) { return format == ASCIICHAT_YUV_YUYV || format == ASCIICHAT_YUV_UYVY; }
YUV_FN int yuv_planes(int32_t format) { return format == ASCIICHAT_YUV_I420 ? 3 : format == ASCIICHAT_YUV_NV12 ? 2 : 1; }
/* the bytes a format's plane k holds per row (its stride when the field says 0) and its rows, for a w x h source */
YUV_FN int32_t yuv_plane_row_bytes(int32_t format, int k, int32_t w) {
  if (yuv_is_packed(format))
    return 2 * w;
  return k == 0 ? w : format == ASCIICHAT_YUV_NV12 ? 2 * yuv_chroma_w(w) : yuv_chroma_w(w);
}
YUV_FN int32_t yuv_plane_rows(int32_t format, int k, int32_t h) { return k == 0 || yuv_is_packed(format) ? h : yuv_chroma_h(h); }

/* The four layouts as one: the samples of pixel (sx, sy) are
 *   Y at y_plane[sy * y_stride + y_mul * sx + y_off]        (packed: 4*(sx/2) + 2*(sx&1) = 2*sx)
 *   U at u_plane[(sy >> c_shift) * u_stride + c_mul * (sx / 2) + u_off],  V alike */
typedef struct {
  const uint8_t *y_plane, *u_plane, *v_plane;
  int64_t y_stride, u_stride, v_stride;
  int32_t y_mul, y_off, c_shift, c_mul, u_off, v_off;
  int32_t width, height;
} yuv_layout_t;

/* of a checked source whose strides are resolved (no 0) */
YUV_FN yuv_layout_t yuv_layout(const asciichat_yuv_source_t *s) {
  yuv_layout_t l;
  l.width = s->width, l.height = s->height;
  l.y_plane = s->plane[0];
  l.y_stride = s->stride[0];
  if (yuv_is_packed(s->format)) { /* UYVY: U Y V Y; YUYV: Y U Y V */
    const int32_t uyvy = s->format == ASCIICHAT_YUV_UYVY;
    l.u_plane = l.v_plane = s->plane[0];
    l.u_stride = l.v_stride = s->stride[0];
    l.y_mul = 2, l.y_off = uyvy ? 1 : 0;
    l.c_shift = 0, l.c_mul = 4, l.u_off = uyvy ? 0 : 1, l.v_off = uyvy ? 2 : 3;
  } else {
    const int32_t nv12 = s->format == ASCIICHAT_YUV_NV12;
    l.u_plane = s->plane[1];
    l.v_plane = nv12 ? s->plane[1] : s->plane[2];
    l.u_stride = s->stride[1];
    l.v_stride = nv12 ? s->stride[1] : s->stride[2];
    l.y_mul = 1, l.y_off = 0;
    l.c_shift = 1, l.c_mul = nv12 ? 2 : 1, l.u_off = 0, l.v_off = nv12 ? 1 : 0;
  }
  return l;
}
/* byte offsets into their planes; rows are 64-bit (8191 rows of 2^24 - 1 bytes) */
YUV_FN int64_t yuv_at_y(const yuv_layout_t *l, int32_t sx, int32_t sy) { return (int64_t)sy * l->y_stride + l->y_mul * sx + l->y_off; }
YUV_FN int64_t yuv_at_u(const yuv_layout_t *l, int32_t sx, int32_t sy) {
  return (int64_t)(sy >> l->c_shift) * l->u_stride + l->c_mul * (sx >> 1) + l->u_off;
}
YUV_FN int64_t yuv_at_v(const yuv_layout_t *l, int32_t sx, int32_t sy) {
  return (int64_t)(sy >> l->c_shift) * l->v_stride + l->c_mul * (sx >> 1) + l->v_off;
}
/* pixel (sx, sy) converted */
YUV_FN uint32_t yuv_pixel(const yuv_layout_t *l, int32_t sx, int32_t sy) {
  return yuv_rgb(l->y_plane[yuv_at_y(l, sx, sy)], l->u_plane[yuv_at_u(l, sx, sy)], l->v_plane[yuv_at_v(l, sx, sy)]);
}

/* the renderers' sampling rule (achip_types.h): the source pixel of image pixel (x, y) of a checked descriptor */
YUV_FN void yuv_sample_at(const achip_frame_t *f, int32_t x, int32_t y, int32_t *sx, int32_t *sy) {
  uint32_t cx = ((uint32_t)x * f->x_ratio) >> 16, cy = ((uint32_t)y * f->y_ratio) >> 16;
  if (cx > (uint32_t)f->src_w - 1u)
    cx = (uint32_t)f->src_w - 1u;
  if (cy > (uint32_t)f->src_h - 1u)
    cy = (uint32_t)f->src_h - 1u;
  *sx = (f->ops & ACHIP_OP_FLIP_X) ? f->src_w - 1 - (int32_t)cx : (int32_t)cx;
  *sy = (f->ops & ACHIP_OP_FLIP_Y) ? f->src_h - 1 - (int32_t)cy : (int32_t)cy;
}

/* ---- the checks (host) ---- */
/* NULL when a source is taken, else what is wrong */
static inline const char *yuv_source_check(const asciichat_yuv_source_t *s) {
  if (!s)
    return "no source";
  if (s->format < ASCIICHAT_YUV_I420 || s->format > ASCIICHAT_YUV_UYVY)
    return "format outside 0..3";
  if (s->width < 1 || s->width > YUV_MAX_SIDE || s->height < 1 || s->height > YUV_MAX_SIDE)
    return "width or height outside 1..8192";
  if (yuv_is_packed(s->format) && (s->width & 1))
    return "an odd width in a packed format";
  const int planes = yuv_planes(s->format);
  for (int k = 0; k < 3; k++) {
    if (k >= planes) {
      if (s->plane[k])
        return "a plane the format does not use";
      continue; /* (its stride is not read) */
    }
    if (!s->plane[k])
      return "a plane is missing";
    if (s->stride[k] < 0 || s->stride[k] >= YUV_MAX_STRIDE)
      return "a stride outside 0..2^24 - 1";
    if (s->stride[k] != 0 && s->stride[k] < yuv_plane_row_bytes(s->format, k, s->width))
      return "a stride below its plane's row";
  }
  return NULL;
}

/* a checked source as the kernels take it: every stride stated, those of unused planes 0 */
static inline asciichat_yuv_source_t yuv_source_resolved(const asciichat_yuv_source_t *s) {
  asciichat_yuv_source_t r = *s;
  for (int k = 0; k < 3; k++)
    r.stride[k] = k >= yuv_planes(s->format) ? 0 : s->stride[k] ? s->stride[k] : yuv_plane_row_bytes(s->format, k, s->width);
  return r;
}

/* NULL when set() takes (sources[0..n-1], frames[0..n-1] or no frames) for a handle of max_frames, else what is wrong.
 * *bad (optional): the offending entry, -1 when it is none of them; *unsupported (optional): 1 when the refusal is a
 * composite descriptor (ERR_NOT_SUPPORTED rather than ERR_INVALID_PARAM). */
static inline const char *yuv_frames_check(const asciichat_yuv_source_t *sources, const achip_frame_t *frames, int n, int max_frames,
                                           int *bad, int *unsupported) {
  if (bad)
    *bad = -1;
  if (unsupported)
    *unsupported = 0;
  if (!sources || n < 1 || n > max_frames)
    return "no sources, or their number outside 1..max_frames";
  for (int i = 0; i < n; i++) {
    if (bad)
      *bad = i;
    const char *why = yuv_source_check(&sources[i]);
    if (why)
      return why;
    if (!frames)
      continue;
    const achip_frame_t *f = &frames[i];
    if (f->comp) {
      if (unsupported)
        *unsupported = 1;
      return "a composite descriptor (its YUV tiles go through run_whole first)";
    }
    if (f->src_w != sources[i].width || f->src_h != sources[i].height)
      return "src_w x src_h of the descriptor is not the source's size";
    if (f->out_w < 1 || f->out_h < 1 || (uint64_t)f->out_w * (uint64_t)f->out_h > 0x7FFFFFFFull / 3u)
      return "an image size below 1, or an image of 2^31 bytes or more";
    if (!achip_desc_ratios_ok(f))
      return "(out_w - 1) * x_ratio or (out_h - 1) * y_ratio reaches 2^32";
  }
  if (bad)
    *bad = -1;
  return NULL;
}

/* where the handle keeps a set of n: n resolved sources, then n descriptors (16-aligned), in one block */
static inline size_t yuv_set_at_frames(int n) { return ((size_t)n * sizeof(asciichat_yuv_source_t) + 15u) & ~(size_t)15u; }
static inline size_t yuv_set_bytes(int n) { return yuv_set_at_frames(n) + (size_t)n * sizeof(achip_frame_t); }

#endif
