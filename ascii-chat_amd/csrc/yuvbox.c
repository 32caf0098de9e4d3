/*
 * yuvbox.c -- the host side of libasciichat_yuvbox.so (include/asciichat_yuvbox.h): a set of sources and descriptors is checked
 * on the host (yuvbox.h) before anything of the handle changes, then staged as items through the one pinned block the handle
 * owns and copied by one asynchronous transfer on the caller's stream; run() and downscale() only launch (yuvbox.hip),
 * render_frames() only rewrites the descriptors the set came with.  Both blocks are allocated by create(); nothing allocates
 * afterwards.  Nothing here comes from the other four libraries.
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "asciichat_yuvbox.h"
#include "yuvbox.h"

#define YUVBOX_MAGIC 0x595556424F583031ull

struct asciichat_yuvbox {
  uint64_t magic;
  int device, max_frames;
  uint8_t *dev, *pinned; /* one block each, max_frames items */
  achip_frame_t *frames; /* the descriptors of the last set as given (host): render_frames rewrites these */
  int n;                 /* images of the last set, 0 before any */
  int dma_queued;        /* the pinned block may still be read by the copy of the last set */
  int max_out_h;         /* the largest out_h among the descriptors */
  int max_src_w;         /* the largest width among the sources */
  size_t max_bytes;      /* the largest 3 * out_w * out_h among the descriptors */
};

static _Thread_local char g_error[256];

static int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
  return code;
}

static int hip_check(hipError_t e, const char *what) {
  if (e == hipSuccess)
    return 0;
  return fail(e == hipErrorOutOfMemory ? ASCIICHAT_YUV_ERR_MEMORY : ASCIICHAT_YUV_ERR_NO_DEVICE, "%s: %s", what, hipGetErrorString(e));
}

const char *asciichat_yuvbox_last_error(void) { return g_error; }

int asciichat_yuvbox_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

static asciichat_yuvbox_t *box_of(const asciichat_yuvbox_t *b) { return b && b->magic == YUVBOX_MAGIC ? (asciichat_yuvbox_t *)b : NULL; }

static size_t round128(size_t v) { return (v + 127u) & ~(size_t)127u; }

static void box_free(asciichat_yuvbox_t *h) {
  (void)hipFree(h->dev);
  if (h->pinned)
    (void)hipHostFree(h->pinned);
  free(h->frames);
  h->magic = 0;
  free(h);
}

int asciichat_yuvbox_create(asciichat_yuvbox_t **b, int max_frames) {
  if (!b)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuvbox_create: no handle");
  *b = NULL;
  if (max_frames < 1 || max_frames > YUV_MAX_FRAMES)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuvbox_create: max_frames %d outside 1..%d", max_frames, YUV_MAX_FRAMES);
  if (asciichat_yuvbox_device_count() <= 0)
    return fail(ASCIICHAT_YUV_ERR_NO_DEVICE, "yuvbox_create: no HIP device");
  asciichat_yuvbox_t *h = (asciichat_yuvbox_t *)calloc(1, sizeof(*h));
  achip_frame_t *frames = (achip_frame_t *)calloc((size_t)max_frames, sizeof(achip_frame_t));
  if (!h || !frames) {
    free(h);
    free(frames);
    return fail(ASCIICHAT_YUV_ERR_MEMORY, "yuvbox_create: out of memory");
  }
  h->magic = YUVBOX_MAGIC;
  h->max_frames = max_frames;
  h->frames = frames;
  const size_t bytes = (size_t)max_frames * sizeof(yuvbox_item_t);
  int rc = hip_check(hipGetDevice(&h->device), "hipGetDevice");
  if (!rc)
    rc = hip_check(hipMalloc((void **)&h->dev, bytes), "hipMalloc(yuvbox set)");
  if (!rc)
    rc = hip_check(hipHostMalloc((void **)&h->pinned, bytes, hipHostMallocDefault), "hipHostMalloc(yuvbox set)");
  if (rc) {
    box_free(h);
    return rc;
  }
  *b = h;
  return 0;
}

int asciichat_yuvbox_set(asciichat_yuvbox_t *b, const asciichat_yuv_source_t *sources, const achip_frame_t *frames, int n, void *stream) {
  asciichat_yuvbox_t *h = box_of(b);
  if (!h)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuvbox_set: not a handle");
  int bad = -1, unsupported = 0;
  const char *why = yuvbox_set_check(sources, frames, n, h->max_frames, &bad, &unsupported);
  if (why) {
    const int code = unsupported ? ASCIICHAT_YUV_ERR_NOT_SUPPORTED : ASCIICHAT_YUV_ERR_INVALID_PARAM;
    return bad >= 0 ? fail(code, "yuvbox_set: frame %d: %s", bad, why) : fail(code, "yuvbox_set: %s", why);
  }
  /* the pinned block may still be in flight from the set before, on this stream (a handle's calls are ordered on one): wait
   * before it is overwritten, and before anything of the handle changes */
  if (h->dma_queued) {
    const int rc = hip_check(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
    if (rc)
      return rc;
  }
  h->dma_queued = 0;
  yuvbox_item_t *staged = (yuvbox_item_t *)h->pinned;
  int max_out_h = 0, max_src_w = 0;
  size_t max_bytes = 0;
  for (int i = 0; i < n; i++) {
    staged[i] = yuvbox_item(&sources[i], frames[i].out_w, frames[i].out_h, frames[i].ops);
    max_out_h = frames[i].out_h > max_out_h ? frames[i].out_h : max_out_h;
    max_src_w = sources[i].width > max_src_w ? sources[i].width : max_src_w;
    const size_t bytes = 3u * (size_t)frames[i].out_w * (size_t)frames[i].out_h;
    max_bytes = bytes > max_bytes ? bytes : max_bytes;
  }
  memcpy(h->frames, frames, (size_t)n * sizeof(achip_frame_t));
  h->n = 0; /* (should the copy fail, nothing is set) */
  const int rc = hip_check(hipMemcpyAsync(h->dev, h->pinned, (size_t)n * sizeof(yuvbox_item_t), hipMemcpyHostToDevice, (hipStream_t)stream),
                           "hipMemcpyAsync(yuvbox set)");
  if (rc)
    return rc;
  h->dma_queued = 1;
  h->n = n;
  h->max_out_h = max_out_h;
  h->max_src_w = max_src_w;
  h->max_bytes = max_bytes;
  return 0;
}

size_t asciichat_yuvbox_image_pitch(const asciichat_yuvbox_t *b) {
  const asciichat_yuvbox_t *h = box_of(b);
  return h && h->n ? round128(h->max_bytes) : 0;
}

/* what run and render_frames ask of a handle and of the images' place */
static int images_ok(const asciichat_yuvbox_t *h, const uint8_t *images_dev, size_t pitch, const char *what) {
  if (!h)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "%s: not a handle", what);
  if (!h->n)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "%s: nothing is set (asciichat_yuvbox_set)", what);
  if (!images_dev || ((uintptr_t)images_dev & 15u) || (pitch & 15u))
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "%s: images and pitch must be multiples of 16", what);
  if (pitch < h->max_bytes)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "%s: pitch %zu below the largest image's %zu bytes", what, pitch, h->max_bytes);
  return 0;
}

int asciichat_yuvbox_run(asciichat_yuvbox_t *b, uint8_t *images_dev, size_t pitch, void *stream) {
  asciichat_yuvbox_t *h = box_of(b);
  const int rc = images_ok(h, images_dev, pitch, "yuvbox_run");
  if (rc)
    return rc;
  return hip_check((hipError_t)yuvbox_launch((const yuvbox_item_t *)h->dev, NULL, h->n, h->max_out_h, h->max_src_w, images_dev, (uint64_t)pitch,
                                             stream),
                   "yuvbox launch");
}

int asciichat_yuvbox_render_frames(const asciichat_yuvbox_t *b, const uint8_t *images_dev, size_t pitch, achip_frame_t *frames_out) {
  const asciichat_yuvbox_t *h = box_of(b);
  const int rc = images_ok(h, images_dev, pitch, "yuvbox_render_frames");
  if (rc)
    return rc;
  if (!frames_out)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuvbox_render_frames: no descriptors to write");
  for (int i = 0; i < h->n; i++) {
    achip_frame_t f = h->frames[i]; /* paddings and out_w x out_h stay */
    f.src = images_dev + (size_t)i * pitch;
    f.comp = NULL;
    f.src_w = f.out_w;
    f.src_h = f.out_h;
    f.x_ratio = f.y_ratio = 65537u; /* ((s << 16) / s) + 1: the identity */
    f.src_stride = 3 * f.out_w;
    f.ops &= ~(ACHIP_OP_FLIP_X | ACHIP_OP_FLIP_Y); /* the pass applied them */
    frames_out[i] = f;
  }
  return 0;
}

int asciichat_yuvbox_downscale(const asciichat_yuv_source_t *src, uint8_t *dst_dev, int dst_w, int dst_h, int flip_x, int flip_y,
                               void *stream) {
  const char *why = yuvbox_source_check(src);
  if (why)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuvbox_downscale: %s", why);
  if (!dst_dev)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuvbox_downscale: no destination");
  if (dst_w < 1 || dst_h < 1 || dst_w > YUVBOX_MAX_OUT || dst_h > YUVBOX_MAX_OUT)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuvbox_downscale: %d x %d outside 1..%d", dst_w, dst_h, YUVBOX_MAX_OUT);
  const yuvbox_item_t one = yuvbox_item(src, dst_w, dst_h, (flip_x ? ACHIP_OP_FLIP_X : 0u) | (flip_y ? ACHIP_OP_FLIP_Y : 0u));
  return hip_check((hipError_t)yuvbox_launch(NULL, &one, 1, dst_h, src->width, dst_dev, 0, stream), "yuvbox downscale launch");
}

void asciichat_yuvbox_destroy(asciichat_yuvbox_t *b) {
  asciichat_yuvbox_t *h = box_of(b);
  if (!h)
    return;
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(h->device);
  box_free(h);
  (void)hipSetDevice(cur);
}
