/*
 * box.c -- the opt-in area-average downscale pass in front of the renderers (asciichat_hip_box_*): a box object holds a
 * tick's render descriptors, averages every source frame to the out_w x out_h image its target would have point-sampled
 * (box_kernels.hpp) and hands back descriptors that render those images as they are.  NOT a parity path: the reference
 * point-samples; what is byte-identical is the reference's renderer run over the averaged image.
 *
 * A batch of equal descriptors at a constant source pitch travels in the kernel arguments; any other batch reads a device
 * array, refreshed by update() through a small ring of pinned host segments: a segment is rewritten only after the copy that
 * read it has finished (its event), so update() never waits on the GPU unless four earlier updates are all still in flight.
 * update() and run() take effect in the order of their stream, like plan_update and plan_render; create() has uploaded its
 * descriptors when it returns, so the first run() may go to any stream.  A failed update() leaves the box as it was.
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <stdlib.h>
#include <string.h>

#include "achip_host.h"
#include "asciichat_hip.h"
#include "box.h"
#include "internal.h"

#define BOX_MAGIC 0x424f584156475247ull
#define BOX_RING 4

struct asciichat_hip_box {
  uint64_t magic;
  int n, device;
  achip_frame_t *frames;      /* the descriptors as given (host copy): render_frames rewrites these */
  achip_box_desc_t *ring;     /* BOX_RING x n, pinned */
  achip_box_desc_t *desc_dev; /* n */
  hipEvent_t ev[BOX_RING];
  int ev_used[BOX_RING];
  int next;
  achip_box_uniform_t uni;
  int max_out_h, max_src_w;
  size_t image_bytes; /* the largest 3 * out_w * out_h */
};

/* one render descriptor as the pass reads it; 0, or the error code with its message recorded */
static int desc_from_frame(const achip_frame_t *f, int i, achip_box_desc_t *d) {
  switch (achip_box_desc_from_frame(f, d)) {
  case ACHIP_BOX_OK:
    return 0;
  case ACHIP_BOX_COMPOSITE:
    return achip_fail(ASCIICHAT_HIP_ERR_NOT_SUPPORTED, "box: frame %d samples a composite", i);
  case ACHIP_BOX_NO_SOURCE:
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box: frame %d has no source", i);
  case ACHIP_BOX_SOURCE_SIZE:
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box: frame %d: source %dx%d outside 1..%dx1..%d", i, f->src_w, f->src_h,
                      ACHIP_BOX_MAX_SRC_W, ACHIP_BOX_MAX_SRC_H);
  case ACHIP_BOX_OUT_SIZE:
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box: frame %d: averaged size %dx%d outside 1..%d", i, f->out_w, f->out_h,
                      ACHIP_BOX_MAX_OUT);
  default:
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box: frame %d: stride %d below a row's %d bytes", i, f->src_stride,
                      3 * f->src_w);
  }
}

static int frames_check(const achip_frame_t *frames, int n) {
  achip_box_desc_t d;
  for (int i = 0; i < n; i++) {
    const int rc = desc_from_frame(&frames[i], i, &d);
    if (rc)
      return rc;
  }
  return 0;
}

/* takes the (checked) descriptors: the uniform form where it applies, else the next ring segment and its copy on `stream`
 * (wait: the copy has landed on return -- box_create, whose caller may run on any stream next).  Nothing of the box
 * changes unless everything succeeded. */
static int box_set(asciichat_hip_box_t *b, const achip_frame_t *frames, hipStream_t stream, int wait) {
  const int s = b->next;
  if (b->ev_used[s]) { /* the copy that read this segment last must be done before it is rewritten */
    const int rc = achip_hip_check((int)hipEventSynchronize(b->ev[s]), "hipEventSynchronize(box ring)");
    if (rc)
      return rc;
    b->ev_used[s] = 0;
  }
  achip_box_desc_t *d = b->ring + (size_t)s * (size_t)b->n;
  int max_out_h = 0, max_src_w = 0;
  size_t image_bytes = 0;
  for (int i = 0; i < b->n; i++) {
    (void)desc_from_frame(&frames[i], i, &d[i]);
    const size_t bytes = 3u * (size_t)d[i].out_w * (size_t)d[i].out_h;
    if (bytes > image_bytes)
      image_bytes = bytes;
    if (d[i].out_h > max_out_h)
      max_out_h = d[i].out_h;
    if (d[i].src_w > max_src_w)
      max_src_w = d[i].src_w;
  }
  achip_box_uniform_t uni;
  if (!achip_box_uniform(d, b->n, &uni)) {
    int rc = achip_hip_check((int)hipMemcpyAsync(b->desc_dev, d, sizeof(*d) * (size_t)b->n, hipMemcpyHostToDevice, stream),
                             "hipMemcpyAsync(box descriptors)");
    if (!rc)
      rc = achip_hip_check((int)hipEventRecord(b->ev[s], stream), "hipEventRecord(box)");
    if (!rc && wait)
      rc = achip_hip_check((int)hipEventSynchronize(b->ev[s]), "hipEventSynchronize(box descriptors)");
    if (rc)
      return rc;
    b->ev_used[s] = !wait;
    b->next = (s + 1) % BOX_RING;
  }
  b->uni = uni;
  memcpy(b->frames, frames, sizeof(*frames) * (size_t)b->n);
  b->max_out_h = max_out_h;
  b->max_src_w = max_src_w;
  b->image_bytes = image_bytes;
  return 0;
}

static asciichat_hip_box_t *box_of(const asciichat_hip_box_t *box) { return box && box->magic == BOX_MAGIC ? (asciichat_hip_box_t *)box : NULL; }

int asciichat_hip_box_create(asciichat_hip_box_t **box, const achip_frame_t *frames, int n_frames) {
  if (!box || !frames || n_frames <= 0)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box_create: bad arguments");
  *box = NULL;
  int rc = frames_check(frames, n_frames);
  if (!rc)
    rc = achip_require_device();
  if (rc)
    return rc;
  asciichat_hip_box_t *b = (asciichat_hip_box_t *)calloc(1, sizeof(*b));
  if (b)
    b->frames = (achip_frame_t *)calloc((size_t)n_frames, sizeof(achip_frame_t));
  if (!b || !b->frames) {
    free(b);
    return achip_fail(ASCIICHAT_HIP_ERR_MEMORY, "box_create: out of memory");
  }
  b->magic = BOX_MAGIC;
  b->n = n_frames;
  int n_ev = 0;
  rc = achip_hip_check((int)hipGetDevice(&b->device), "hipGetDevice");
  if (!rc)
    rc = achip_hip_check((int)hipHostMalloc((void **)&b->ring, sizeof(achip_box_desc_t) * BOX_RING * (size_t)n_frames, hipHostMallocDefault),
                         "hipHostMalloc(box descriptors)");
  if (!rc)
    rc = achip_hip_check((int)hipMalloc((void **)&b->desc_dev, sizeof(achip_box_desc_t) * (size_t)n_frames), "hipMalloc(box descriptors)");
  for (; !rc && n_ev < BOX_RING; n_ev++)
    rc = achip_hip_check((int)hipEventCreateWithFlags(&b->ev[n_ev], hipEventDisableTiming), "hipEventCreate(box)");
  if (rc)
    n_ev--; /* the one that failed does not exist */
  if (!rc)
    rc = box_set(b, frames, NULL, 1); /* uploaded before create returns: the first run may be on any stream */
  if (rc) {
    for (int s = 0; s < n_ev; s++)
      (void)hipEventDestroy(b->ev[s]);
    (void)hipFree(b->desc_dev);
    if (b->ring)
      (void)hipHostFree(b->ring);
    free(b->frames);
    free(b);
    return rc;
  }
  *box = b;
  return 0;
}

int asciichat_hip_box_update(asciichat_hip_box_t *box, const achip_frame_t *frames, void *stream) {
  asciichat_hip_box_t *b = box_of(box);
  if (!b || !frames)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box_update: bad arguments");
  const int rc = frames_check(frames, b->n);
  return rc ? rc : box_set(b, frames, (hipStream_t)stream, 0);
}

size_t asciichat_hip_box_image_pitch(const asciichat_hip_box_t *box) {
  const asciichat_hip_box_t *b = box_of(box);
  return b ? (b->image_bytes + 127u) & ~(size_t)127u : 0;
}

int asciichat_hip_box_run(asciichat_hip_box_t *box, uint8_t *images_dev, size_t pitch, void *stream) {
  asciichat_hip_box_t *b = box_of(box);
  if (!b || !images_dev)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box_run: bad arguments");
  if (pitch < b->image_bytes)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box_run: pitch %zu below an image's %zu bytes", pitch, b->image_bytes);
  return achip_hip_check(achip_launch_box(b->desc_dev, &b->uni, b->n, b->max_out_h, b->max_src_w, images_dev, (uint64_t)pitch, stream),
                         "box launch");
}

int asciichat_hip_box_get_uniform(const asciichat_hip_box_t *box) {
  const asciichat_hip_box_t *b = box_of(box);
  return b ? (int)b->uni.enabled : 0;
}

int asciichat_hip_box_render_frames(const asciichat_hip_box_t *box, const uint8_t *images_dev, size_t pitch, achip_frame_t *frames_out) {
  const asciichat_hip_box_t *b = box_of(box);
  if (!b || !images_dev || !frames_out)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box_render_frames: bad arguments");
  if (pitch < b->image_bytes)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box_render_frames: pitch %zu below an image's %zu bytes", pitch, b->image_bytes);
  for (int i = 0; i < b->n; i++) {
    achip_frame_t f = b->frames[i];
    const int32_t pad_left = f.pad_left, pad_top = f.pad_top;
    const uint32_t ops = f.ops & ~(ACHIP_OP_FLIP_X | ACHIP_OP_FLIP_Y);
    (void)achip_frame_identity(&f, images_dev + (size_t)i * pitch, b->frames[i].out_w, b->frames[i].out_h);
    f.pad_left = pad_left;
    f.pad_top = pad_top;
    f.ops = ops;
    frames_out[i] = f;
  }
  return 0;
}

void asciichat_hip_box_destroy(asciichat_hip_box_t *box) {
  asciichat_hip_box_t *b = box_of(box);
  if (!b)
    return;
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(b->device);
  for (int s = 0; s < BOX_RING; s++) {
    if (b->ev_used[s])
      (void)hipEventSynchronize(b->ev[s]);
    (void)hipEventDestroy(b->ev[s]);
  }
  (void)hipFree(b->desc_dev);
  (void)hipHostFree(b->ring);
  (void)hipSetDevice(cur);
  b->magic = 0;
  free(b->frames);
  free(b);
}

int asciichat_hip_box_downscale(const uint8_t *src_dev, int src_w, int src_h, int src_stride, uint8_t *dst_dev, int dst_w, int dst_h,
                                int flip_x, int flip_y, void *stream) {
  if (!dst_dev)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box_downscale: no destination");
  achip_frame_t f;
  memset(&f, 0, sizeof(f));
  f.src = src_dev;
  f.src_w = src_w;
  f.src_h = src_h;
  f.out_w = dst_w;
  f.out_h = dst_h;
  f.src_stride = src_stride;
  f.ops = (flip_x ? ACHIP_OP_FLIP_X : 0u) | (flip_y ? ACHIP_OP_FLIP_Y : 0u);
  if (src_stride < 0)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box_downscale: stride %d", src_stride);
  achip_box_uniform_t uni;
  memset(&uni, 0, sizeof(uni));
  int rc = desc_from_frame(&f, 0, &uni.d);
  if (!rc)
    rc = achip_require_device();
  if (rc)
    return rc;
  uni.enabled = 1;
  return achip_hip_check(achip_launch_box(NULL, &uni, 1, dst_h, src_w, dst_dev, 3u * (uint64_t)dst_w * (uint64_t)dst_h, stream), "box launch");
}
