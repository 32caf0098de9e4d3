/*
 * yuv.c -- the host side of libasciichat_yuv.so (include/asciichat_yuv.h): a set of sources and descriptors is checked on the
 * host (yuv_math.h) before anything of the handle changes, then staged through the one pinned block the handle owns and copied
 * by one asynchronous transfer on the caller's stream; run(), run_whole() and convert() only launch (yuv.hip).  Both blocks are
 * allocated by create(); nothing allocates afterwards.  Nothing here comes from the other two libraries.
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "asciichat_yuv.h"
#include "yuv.h"

#define YUV_MAGIC 0x5955565352433031ull

struct asciichat_yuv {
  uint64_t magic;
  int device, max_frames;
  uint8_t *dev, *pinned;  /* one block each, yuv_set_bytes(max_frames): the resolved sources, then the descriptors */
  achip_frame_t *frames;  /* the descriptors of the last set as given (host): render_frames rewrites these */
  int n;                  /* sources of the last set, 0 before any */
  int has_frames;         /* the last set came with descriptors */
  int dma_queued;         /* the pinned block may still be read by the copy of the last set */
  unsigned formats;       /* bit f: some source of the set has format f */
  int max_w, max_h;       /* the largest width and height among the sources */
  uint32_t max_pixels;    /* the largest out_w * out_h among the descriptors */
  size_t max_whole_bytes; /* the largest 3 * width * height among the sources */
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

const char *asciichat_yuv_last_error(void) { return g_error; }

int asciichat_yuv_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

static asciichat_yuv_t *yuv_of(const asciichat_yuv_t *y) { return y && y->magic == YUV_MAGIC ? (asciichat_yuv_t *)y : NULL; }

static size_t round128(size_t v) { return (v + 127u) & ~(size_t)127u; }

static void yuv_free(asciichat_yuv_t *h) {
  (void)hipFree(h->dev);
  if (h->pinned)
    (void)hipHostFree(h->pinned);
  free(h->frames);
  h->magic = 0;
  free(h);
}

int asciichat_yuv_create(asciichat_yuv_t **y, int max_frames) {
  if (!y)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuv_create: no handle");
  *y = NULL;
  if (max_frames < 1 || max_frames > YUV_MAX_FRAMES)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuv_create: max_frames %d outside 1..%d", max_frames, YUV_MAX_FRAMES);
  if (asciichat_yuv_device_count() <= 0)
    return fail(ASCIICHAT_YUV_ERR_NO_DEVICE, "yuv_create: no HIP device");
  asciichat_yuv_t *h = (asciichat_yuv_t *)calloc(1, sizeof(*h));
  achip_frame_t *frames = (achip_frame_t *)calloc((size_t)max_frames, sizeof(achip_frame_t));
  if (!h || !frames) {
    free(h);
    free(frames);
    return fail(ASCIICHAT_YUV_ERR_MEMORY, "yuv_create: out of memory");
  }
  h->magic = YUV_MAGIC;
  h->max_frames = max_frames;
  h->frames = frames;
  const size_t bytes = yuv_set_bytes(max_frames);
  int rc = hip_check(hipGetDevice(&h->device), "hipGetDevice");
  if (!rc)
    rc = hip_check(hipMalloc((void **)&h->dev, bytes), "hipMalloc(yuv set)");
  if (!rc)
    rc = hip_check(hipHostMalloc((void **)&h->pinned, bytes, hipHostMallocDefault), "hipHostMalloc(yuv set)");
  if (rc) {
    yuv_free(h);
    return rc;
  }
  *y = h;
  return 0;
}

int asciichat_yuv_set(asciichat_yuv_t *y, const asciichat_yuv_source_t *sources, const achip_frame_t *frames, int n, void *stream) {
  asciichat_yuv_t *h = yuv_of(y);
  if (!h)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuv_set: not a handle");
  int bad = -1, unsupported = 0;
  const char *why = yuv_frames_check(sources, frames, n, h->max_frames, &bad, &unsupported);
  if (why) {
    const int code = unsupported ? ASCIICHAT_YUV_ERR_NOT_SUPPORTED : ASCIICHAT_YUV_ERR_INVALID_PARAM;
    return bad >= 0 ? fail(code, "yuv_set: frame %d: %s", bad, why) : fail(code, "yuv_set: %s", why);
  }
  /* the pinned block may still be in flight from the set before, on this stream (a handle's calls are ordered on one): wait
   * before it is overwritten, and before anything of the handle changes */
  if (h->dma_queued) {
    const int rc = hip_check(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
    if (rc)
      return rc;
  }
  h->dma_queued = 0;
  asciichat_yuv_source_t *staged = (asciichat_yuv_source_t *)h->pinned;
  unsigned formats = 0u;
  int max_w = 0, max_h = 0;
  uint32_t max_pixels = 0u;
  for (int i = 0; i < n; i++) {
    staged[i] = yuv_source_resolved(&sources[i]);
    formats |= 1u << sources[i].format;
    max_w = sources[i].width > max_w ? sources[i].width : max_w;
    max_h = sources[i].height > max_h ? sources[i].height : max_h;
    if (frames) {
      const uint32_t pixels = (uint32_t)frames[i].out_w * (uint32_t)frames[i].out_h;
      max_pixels = pixels > max_pixels ? pixels : max_pixels;
    }
  }
  if (frames) {
    memcpy(h->pinned + yuv_set_at_frames(n), frames, (size_t)n * sizeof(achip_frame_t));
    memcpy(h->frames, frames, (size_t)n * sizeof(achip_frame_t));
  }
  h->n = 0; /* (should the copy fail, nothing is set) */
  const size_t bytes = frames ? yuv_set_bytes(n) : (size_t)n * sizeof(asciichat_yuv_source_t);
  const int rc = hip_check(hipMemcpyAsync(h->dev, h->pinned, bytes, hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync(yuv set)");
  if (rc)
    return rc;
  h->dma_queued = 1;
  h->n = n;
  h->has_frames = frames != NULL;
  h->formats = formats;
  h->max_w = max_w;
  h->max_h = max_h;
  h->max_pixels = max_pixels;
  h->max_whole_bytes = 0;
  for (int i = 0; i < n; i++) {
    const size_t b = 3u * (size_t)sources[i].width * (size_t)sources[i].height;
    h->max_whole_bytes = b > h->max_whole_bytes ? b : h->max_whole_bytes;
  }
  return 0;
}

size_t asciichat_yuv_image_pitch(const asciichat_yuv_t *y) {
  const asciichat_yuv_t *h = yuv_of(y);
  return h && h->n && h->has_frames ? round128(3u * (size_t)h->max_pixels) : 0;
}

size_t asciichat_yuv_whole_pitch(const asciichat_yuv_t *y) {
  const asciichat_yuv_t *h = yuv_of(y);
  return h && h->n ? round128(h->max_whole_bytes) : 0;
}

/* what run and render_frames ask of a handle and of the images' place */
static int images_ok(const asciichat_yuv_t *h, const uint8_t *images_dev, size_t pitch, const char *what) {
  if (!h)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "%s: not a handle", what);
  if (!h->n || !h->has_frames)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "%s: no descriptors are set (asciichat_yuv_set with frames)", what);
  if (!images_dev || ((uintptr_t)images_dev & 15u) || (pitch & 15u))
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "%s: images and pitch must be multiples of 16", what);
  if (pitch < 3u * (size_t)h->max_pixels)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "%s: pitch %zu below the largest image's %zu bytes", what, pitch, 3u * (size_t)h->max_pixels);
  return 0;
}

int asciichat_yuv_run(asciichat_yuv_t *y, uint8_t *images_dev, size_t pitch, void *stream) {
  asciichat_yuv_t *h = yuv_of(y);
  const int rc = images_ok(h, images_dev, pitch, "yuv_run");
  if (rc)
    return rc;
  return hip_check((hipError_t)yuv_launch_sample((const asciichat_yuv_source_t *)h->dev, (const achip_frame_t *)(h->dev + yuv_set_at_frames(h->n)),
                                                 h->n, h->max_pixels, images_dev, (uint64_t)pitch, stream),
                   "yuv sample launch");
}

int asciichat_yuv_render_frames(const asciichat_yuv_t *y, const uint8_t *images_dev, size_t pitch, achip_frame_t *frames_out) {
  const asciichat_yuv_t *h = yuv_of(y);
  const int rc = images_ok(h, images_dev, pitch, "yuv_render_frames");
  if (rc)
    return rc;
  if (!frames_out)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuv_render_frames: no descriptors to write");
  for (int i = 0; i < h->n; i++) {
    achip_frame_t f = h->frames[i]; /* paddings and out_w x out_h stay */
    f.src = images_dev + (size_t)i * pitch;
    f.comp = NULL;
    f.src_w = f.out_w;
    f.src_h = f.out_h;
    f.x_ratio = f.y_ratio = 65537u; /* ((s << 16) / s) + 1: the identity */
    f.src_stride = 3 * f.out_w;
    f.ops &= ~(ACHIP_OP_FLIP_X | ACHIP_OP_FLIP_Y);
    frames_out[i] = f;
  }
  return 0;
}

int asciichat_yuv_run_whole(asciichat_yuv_t *y, uint8_t *rgb_dev, size_t pitch, void *stream) {
  asciichat_yuv_t *h = yuv_of(y);
  if (!h)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuv_run_whole: not a handle");
  if (!h->n)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuv_run_whole: no sources are set (asciichat_yuv_set)");
  if (!rgb_dev || pitch < h->max_whole_bytes)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuv_run_whole: a destination and a pitch of at least %zu are required", h->max_whole_bytes);
  yuv_whole_args_t a;
  memset(&a, 0, sizeof(a));
  a.sources = (const asciichat_yuv_source_t *)h->dev;
  a.rgb = rgb_dev;
  a.pitch = (uint64_t)pitch;
  return hip_check((hipError_t)yuv_launch_whole(&a, h->n, h->max_w, h->max_h, h->formats, stream), "yuv whole launch");
}

int asciichat_yuv_convert(const asciichat_yuv_source_t *src, uint8_t *rgb_dev, int rgb_stride, void *stream) {
  const char *why = yuv_source_check(src);
  if (why)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuv_convert: %s", why);
  if (!rgb_dev)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuv_convert: no destination");
  if (rgb_stride != 0 && (rgb_stride < 3 * src->width || rgb_stride >= YUV_MAX_STRIDE))
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuv_convert: rgb_stride %d outside %d..2^24 - 1", rgb_stride, 3 * src->width);
  yuv_whole_args_t a;
  memset(&a, 0, sizeof(a));
  a.one = yuv_source_resolved(src);
  a.rgb = rgb_dev;
  a.rgb_stride = rgb_stride;
  return hip_check((hipError_t)yuv_launch_whole(&a, 1, src->width, src->height, 1u << src->format, stream), "yuv convert launch");
}

void asciichat_yuv_destroy(asciichat_yuv_t *y) {
  asciichat_yuv_t *h = yuv_of(y);
  if (!h)
    return;
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(h->device);
  yuv_free(h);
  (void)hipSetDevice(cur);
}
