/*
 * pix.c -- the host side of libasciichat_pix.so (include/asciichat_pix.h): a set of sources and descriptors is checked on the
 * host (pix_math.h) before anything of the handle changes, then staged through the one pinned block the handle owns and copied
 * by one asynchronous transfer on the caller's stream; run(), run_box(), run_whole(), convert() and downscale() only launch
 * (pix.hip), render_frames() only rewrites the descriptors the set came with.  Both blocks are allocated by create(); nothing
 * allocates afterwards.  Nothing here comes from the other six libraries.
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "asciichat_pix.h"
#include "pix.h"

#define PIX_MAGIC 0x5049585352433031ull

struct asciichat_pix {
  uint64_t magic;
  int device, max_frames;
  uint8_t *dev, *pinned;  /* one block each, pix_set_bytes(max_frames): the resolved sources, then the descriptors */
  achip_frame_t *frames;  /* the descriptors of the last set as given (host): render_frames rewrites these */
  int n;                  /* sources of the last set, 0 before any */
  int has_frames;         /* the last set came with descriptors */
  int boxable;            /* ... and every source and image side of it lies within the box pass's limits */
  int dma_queued;         /* the pinned block may still be read by the copy of the last set */
  unsigned bpps;          /* bit 0: some source of the set has 3 bytes per pixel, bit 1: some has 4 */
  int max_w, max_h;       /* the largest width and height among the sources */
  int max_out_h;          /* the largest out_h among the descriptors */
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
  return fail(e == hipErrorOutOfMemory ? ASCIICHAT_PIX_ERR_MEMORY : ASCIICHAT_PIX_ERR_NO_DEVICE, "%s: %s", what, hipGetErrorString(e));
}

const char *asciichat_pix_last_error(void) { return g_error; }

int asciichat_pix_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

static asciichat_pix_t *pix_of(const asciichat_pix_t *p) { return p && p->magic == PIX_MAGIC ? (asciichat_pix_t *)p : NULL; }

static size_t round128(size_t v) { return (v + 127u) & ~(size_t)127u; }

static void pix_free(asciichat_pix_t *h) {
  (void)hipFree(h->dev);
  if (h->pinned)
    (void)hipHostFree(h->pinned);
  free(h->frames);
  h->magic = 0;
  free(h);
}

int asciichat_pix_create(asciichat_pix_t **p, int max_frames) {
  if (!p)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pix_create: no handle");
  *p = NULL;
  if (max_frames < 1 || max_frames > PIX_MAX_FRAMES)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pix_create: max_frames %d outside 1..%d", max_frames, PIX_MAX_FRAMES);
  if (asciichat_pix_device_count() <= 0)
    return fail(ASCIICHAT_PIX_ERR_NO_DEVICE, "pix_create: no HIP device");
  asciichat_pix_t *h = (asciichat_pix_t *)calloc(1, sizeof(*h));
  achip_frame_t *frames = (achip_frame_t *)calloc((size_t)max_frames, sizeof(achip_frame_t));
  if (!h || !frames) {
    free(h);
    free(frames);
    return fail(ASCIICHAT_PIX_ERR_MEMORY, "pix_create: out of memory");
  }
  h->magic = PIX_MAGIC;
  h->max_frames = max_frames;
  h->frames = frames;
  const size_t bytes = pix_set_bytes(max_frames);
  int rc = hip_check(hipGetDevice(&h->device), "hipGetDevice");
  if (!rc)
    rc = hip_check(hipMalloc((void **)&h->dev, bytes), "hipMalloc(pix set)");
  if (!rc)
    rc = hip_check(hipHostMalloc((void **)&h->pinned, bytes, hipHostMallocDefault), "hipHostMalloc(pix set)");
  if (rc) {
    pix_free(h);
    return rc;
  }
  *p = h;
  return 0;
}

int asciichat_pix_set(asciichat_pix_t *p, const asciichat_pix_source_t *sources, const achip_frame_t *frames, int n, void *stream) {
  asciichat_pix_t *h = pix_of(p);
  if (!h)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pix_set: not a handle");
  int bad = -1, unsupported = 0;
  const char *why = pix_set_check(sources, frames, n, h->max_frames, &bad, &unsupported);
  if (why) {
    const int code = unsupported ? ASCIICHAT_PIX_ERR_NOT_SUPPORTED : ASCIICHAT_PIX_ERR_INVALID_PARAM;
    return bad >= 0 ? fail(code, "pix_set: frame %d: %s", bad, why) : fail(code, "pix_set: %s", why);
  }
  /* the pinned block may still be in flight from the set before, on this stream (a handle's calls are ordered on one): wait
   * before it is overwritten, and before anything of the handle changes */
  if (h->dma_queued) {
    const int rc = hip_check(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
    if (rc)
      return rc;
  }
  h->dma_queued = 0;
  asciichat_pix_source_t *staged = (asciichat_pix_source_t *)h->pinned;
  unsigned bpps = 0u;
  int max_w = 0, max_h = 0, max_out_h = 0;
  uint32_t max_pixels = 0u;
  size_t max_whole_bytes = 0;
  for (int i = 0; i < n; i++) {
    staged[i] = pix_source_resolved(&sources[i]);
    bpps |= 1u << (sources[i].format & 1);
    max_w = sources[i].width > max_w ? sources[i].width : max_w;
    max_h = sources[i].height > max_h ? sources[i].height : max_h;
    const size_t b = 3u * (size_t)sources[i].width * (size_t)sources[i].height;
    max_whole_bytes = b > max_whole_bytes ? b : max_whole_bytes;
    if (frames) {
      const uint32_t pixels = (uint32_t)frames[i].out_w * (uint32_t)frames[i].out_h;
      max_pixels = pixels > max_pixels ? pixels : max_pixels;
      max_out_h = frames[i].out_h > max_out_h ? frames[i].out_h : max_out_h;
    }
  }
  if (frames) {
    memcpy(h->pinned + pix_set_at_frames(n), frames, (size_t)n * sizeof(achip_frame_t));
    memcpy(h->frames, frames, (size_t)n * sizeof(achip_frame_t));
  }
  h->n = 0; /* (should the copy fail, nothing is set) */
  const size_t bytes = frames ? pix_set_bytes(n) : (size_t)n * sizeof(asciichat_pix_source_t);
  const int rc = hip_check(hipMemcpyAsync(h->dev, h->pinned, bytes, hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync(pix set)");
  if (rc)
    return rc;
  h->dma_queued = 1;
  h->n = n;
  h->has_frames = frames != NULL;
  h->boxable = frames != NULL && pix_set_boxable(sources, frames, n);
  h->bpps = bpps;
  h->max_w = max_w;
  h->max_h = max_h;
  h->max_out_h = max_out_h;
  h->max_pixels = max_pixels;
  h->max_whole_bytes = max_whole_bytes;
  return 0;
}

size_t asciichat_pix_image_pitch(const asciichat_pix_t *p) {
  const asciichat_pix_t *h = pix_of(p);
  return h && h->n && h->has_frames ? round128(3u * (size_t)h->max_pixels) : 0;
}

size_t asciichat_pix_whole_pitch(const asciichat_pix_t *p) {
  const asciichat_pix_t *h = pix_of(p);
  return h && h->n ? round128(h->max_whole_bytes) : 0;
}

/* what run, run_box and render_frames ask of a handle and of the images' place */
static int images_ok(const asciichat_pix_t *h, const uint8_t *images_dev, size_t pitch, const char *what) {
  if (!h)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "%s: not a handle", what);
  if (!h->n || !h->has_frames)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "%s: no descriptors are set (asciichat_pix_set with frames)", what);
  if (!images_dev || ((uintptr_t)images_dev & 15u) || (pitch & 15u))
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "%s: images and pitch must be multiples of 16", what);
  if (pitch < 3u * (size_t)h->max_pixels)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "%s: pitch %zu below the largest image's %zu bytes", what, pitch, 3u * (size_t)h->max_pixels);
  return 0;
}

int asciichat_pix_run(asciichat_pix_t *p, uint8_t *images_dev, size_t pitch, void *stream) {
  asciichat_pix_t *h = pix_of(p);
  const int rc = images_ok(h, images_dev, pitch, "pix_run");
  if (rc)
    return rc;
  return hip_check((hipError_t)pix_launch_sample((const asciichat_pix_source_t *)h->dev, (const achip_frame_t *)(h->dev + pix_set_at_frames(h->n)),
                                                 h->n, h->max_pixels, images_dev, (uint64_t)pitch, stream),
                   "pix sample launch");
}

int asciichat_pix_run_box(asciichat_pix_t *p, uint8_t *images_dev, size_t pitch, void *stream) {
  asciichat_pix_t *h = pix_of(p);
  const int rc = images_ok(h, images_dev, pitch, "pix_run_box");
  if (rc)
    return rc;
  if (!h->boxable)
    return fail(ASCIICHAT_PIX_ERR_NOT_SUPPORTED, "pix_run_box: a source of the set exceeds %d x %d, or an image side %d (the box pass's limits)",
                PIX_BOX_MAX_SRC_W, PIX_BOX_MAX_SRC_H, PIX_BOX_MAX_OUT);
  pix_box_args_t a;
  memset(&a, 0, sizeof(a));
  a.sources = (const asciichat_pix_source_t *)h->dev;
  a.frames = (const achip_frame_t *)(h->dev + pix_set_at_frames(h->n));
  a.rows_per_image = (uint32_t)h->max_out_h;
  a.images = images_dev;
  a.pitch = (uint64_t)pitch;
  return hip_check((hipError_t)pix_launch_box(&a, h->n, h->max_w, stream), "pix box launch");
}

int asciichat_pix_render_frames(const asciichat_pix_t *p, const uint8_t *images_dev, size_t pitch, achip_frame_t *frames_out) {
  const asciichat_pix_t *h = pix_of(p);
  const int rc = images_ok(h, images_dev, pitch, "pix_render_frames");
  if (rc)
    return rc;
  if (!frames_out)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pix_render_frames: no descriptors to write");
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

int asciichat_pix_run_whole(asciichat_pix_t *p, uint8_t *rgb_dev, size_t pitch, void *stream) {
  asciichat_pix_t *h = pix_of(p);
  if (!h)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pix_run_whole: not a handle");
  if (!h->n)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pix_run_whole: no sources are set (asciichat_pix_set)");
  if (!rgb_dev || pitch < h->max_whole_bytes)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pix_run_whole: a destination and a pitch of at least %zu are required", h->max_whole_bytes);
  pix_whole_args_t a;
  memset(&a, 0, sizeof(a));
  a.sources = (const asciichat_pix_source_t *)h->dev;
  a.rgb = rgb_dev;
  a.pitch = (uint64_t)pitch;
  return hip_check((hipError_t)pix_launch_whole(&a, h->n, h->max_w, h->max_h, h->bpps, stream), "pix whole launch");
}

int asciichat_pix_convert(const asciichat_pix_source_t *src, uint8_t *rgb_dev, int rgb_stride, void *stream) {
  const char *why = pix_source_check(src);
  if (why)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pix_convert: %s", why);
  if (!rgb_dev)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pix_convert: no destination");
  if (rgb_stride != 0 && (rgb_stride < 3 * src->width || rgb_stride >= PIX_MAX_STRIDE))
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pix_convert: rgb_stride %d outside %d..2^24 - 1", rgb_stride, 3 * src->width);
  pix_whole_args_t a;
  memset(&a, 0, sizeof(a));
  a.one = pix_source_resolved(src);
  a.rgb = rgb_dev;
  a.rgb_stride = rgb_stride;
  return hip_check((hipError_t)pix_launch_whole(&a, 1, src->width, src->height, 1u << (src->format & 1), stream), "pix convert launch");
}

int asciichat_pix_downscale(const asciichat_pix_source_t *src, uint8_t *dst_dev, int dst_w, int dst_h, int flip_x, int flip_y, void *stream) {
  const char *why = pix_source_check(src);
  if (why)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pix_downscale: %s", why);
  if (!pix_source_boxable(src))
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pix_downscale: a source larger than %d x %d", PIX_BOX_MAX_SRC_W, PIX_BOX_MAX_SRC_H);
  if (!dst_dev)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pix_downscale: no destination");
  if (dst_w < 1 || dst_h < 1 || dst_w > PIX_BOX_MAX_OUT || dst_h > PIX_BOX_MAX_OUT)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pix_downscale: %d x %d outside 1..%d", dst_w, dst_h, PIX_BOX_MAX_OUT);
  pix_box_args_t a;
  memset(&a, 0, sizeof(a));
  a.one = pix_source_resolved(src);
  a.one_w = dst_w;
  a.one_h = dst_h;
  a.one_flips = (flip_x ? ACHIP_OP_FLIP_X : 0u) | (flip_y ? ACHIP_OP_FLIP_Y : 0u);
  a.rows_per_image = (uint32_t)dst_h;
  a.images = dst_dev;
  return hip_check((hipError_t)pix_launch_box(&a, 1, src->width, stream), "pix downscale launch");
}

void asciichat_pix_destroy(asciichat_pix_t *p) {
  asciichat_pix_t *h = pix_of(p);
  if (!h)
    return;
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(h->device);
  pix_free(h);
  (void)hipSetDevice(cur);
}
