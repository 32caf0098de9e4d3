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
 *
 * Grid composites (asciichat_hip_box_composites): the plan step of box.h turns a tick's host composite descriptors into
 * unique tiles (ordinary box descriptors, averaged by the same kernel into a scratch slab the box owns) and one table per
 * composite frame (box_canvas_kernel assembles and averages the canvas from the tiles).  Tables and tile descriptors travel
 * behind the plain descriptors in the same ring segment and the same copy.  An update that needs more tile scratch than
 * the box holds allocates a larger slab and synchronises the given stream before it frees the old one: the second case in
 * which an update waits.
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
  achip_frame_t *frames; /* the descriptors as given (host copy): render_frames rewrites these */
  uint8_t *ring;         /* BOX_RING segments of seg_bytes, pinned: [plain n][canvas tables n][tiles 9 n] at most */
  uint8_t *desc_dev;     /* one segment: [plain n][canvas tables plan.n_canvas][tiles plan.n_tiles] */
  size_t seg_bytes;
  hipEvent_t ev[BOX_RING];
  int ev_used[BOX_RING];
  int next;
  achip_box_uniform_t uni;
  achip_box_plan_t plan;
  uint8_t *slab; /* the tiles of the composite frames, plan.n_tiles x plan.tile_pitch; grows, never shrinks */
  size_t slab_bytes;
};

/* a refusal of the plan step (box.h) as the error code with its message recorded; 0 for ACHIP_BOX_OK */
static int plan_fail(int why, const achip_frame_t *frames, const achip_composite_t *const *comps, const achip_box_plan_t *p) {
  if (why == ACHIP_BOX_OK)
    return 0;
  const int i = p->bad_frame, k = p->bad_src;
  const achip_frame_t *f = &frames[i];
  const achip_composite_t *c = comps ? comps[i] : NULL;
  if (c && k >= 0) {
    const achip_comp_src_t *s = &c->s[k];
    switch (why) {
    case ACHIP_BOX_SOURCE_SIZE:
      return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box: frame %d: composite source %d: %dx%d outside 1..%dx1..%d", i, k, s->src_w,
                        s->src_h, ACHIP_BOX_MAX_SRC_W, ACHIP_BOX_MAX_SRC_H);
    case ACHIP_BOX_STRIDE:
      return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box: frame %d: composite source %d: stride %d below a row's %d bytes", i, k,
                        s->src_stride, 3 * s->src_w);
    default:
      return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box: frame %d: composite source %d: tile %dx%d outside 1..%dx1..%d", i, k,
                        s->tile_w, s->tile_h, c->canvas_w, c->canvas_h);
    }
  }
  switch (why) {
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
  case ACHIP_BOX_CANVAS_SIZE:
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box: frame %d: canvas %dx%d outside 1..%dx1..%d", i, c->canvas_w, c->canvas_h,
                      ACHIP_BOX_MAX_SRC_W, ACHIP_BOX_MAX_SRC_H);
  case ACHIP_BOX_CANVAS_FRAME:
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box: frame %d: source size %dx%d is not its composite's canvas %dx%d", i, f->src_w,
                      f->src_h, c->canvas_w, c->canvas_h);
  case ACHIP_BOX_GRID:
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box: frame %d: composite of %d sources on a %dx%d grid", i, c->n_src, c->cols,
                      c->rows);
  default:
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box: frame %d: stride %d below a row's %d bytes", i, f->src_stride,
                      3 * f->src_w);
  }
}

static int frames_check(const achip_frame_t *frames, const achip_composite_t *const *comps, int n) {
  achip_box_plan_t p;
  return plan_fail(achip_box_plan(frames, comps, n, NULL, NULL, NULL, &p), frames, comps, &p);
}

/* takes the (checked) descriptors: the uniform form where it applies, else the next ring segment and its copy on `stream`
 * (wait: the copy has landed on return -- create, whose caller may run on any stream next).  A batch whose tiles outgrow
 * the scratch slab gets a larger one; the old one is freed once `stream` has drained (the runs that wrote it were ordered
 * on it).  Nothing of the box changes unless everything succeeded -- but for a slab that may have grown. */
static int box_set(asciichat_hip_box_t *b, const achip_frame_t *frames, const achip_composite_t *const *comps, hipStream_t stream,
                   int wait) {
  const int s = b->next;
  if (b->ev_used[s]) { /* the copy that read this segment last must be done before it is rewritten */
    const int rc = achip_hip_check((int)hipEventSynchronize(b->ev[s]), "hipEventSynchronize(box ring)");
    if (rc)
      return rc;
    b->ev_used[s] = 0;
  }
  const size_t n = (size_t)b->n;
  uint8_t *seg = b->ring + (size_t)s * b->seg_bytes;
  achip_box_desc_t *d = (achip_box_desc_t *)seg;
  achip_box_canvas_t *canvas = (achip_box_canvas_t *)(seg + sizeof(*d) * n);
  achip_box_desc_t *tiles = (achip_box_desc_t *)(seg + (sizeof(*d) + sizeof(*canvas)) * n);
  achip_box_plan_t plan;
  (void)achip_box_plan(frames, comps, b->n, d, tiles, canvas, &plan);
  achip_box_uniform_t uni;
  memset(&uni, 0, sizeof(uni));
  const int uniform = plan.n_canvas == 0 && achip_box_uniform(d, b->n, &uni);
  const size_t need = (size_t)plan.n_tiles * (size_t)plan.tile_pitch;
  if (need > b->slab_bytes) {
    uint8_t *slab = NULL;
    int rc = achip_hip_check((int)hipMalloc((void **)&slab, need), "hipMalloc(box tiles)");
    if (!rc && b->slab && (rc = achip_hip_check((int)hipStreamSynchronize(stream), "hipStreamSynchronize(box tiles)")) != 0)
      (void)hipFree(slab);
    if (rc)
      return rc;
    (void)hipFree(b->slab);
    b->slab = slab;
    b->slab_bytes = need;
  }
  if (!uniform) {
    /* the tables and the unique tiles follow the plain descriptors: one copy */
    uint8_t *tiles_at = (uint8_t *)(canvas + plan.n_canvas);
    memmove(tiles_at, tiles, sizeof(*tiles) * (size_t)plan.n_tiles);
    const size_t bytes = (size_t)(tiles_at - seg) + sizeof(*tiles) * (size_t)plan.n_tiles;
    int rc = achip_hip_check((int)hipMemcpyAsync(b->desc_dev, seg, bytes, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(box descriptors)");
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
  b->plan = plan;
  memcpy(b->frames, frames, sizeof(*frames) * n);
  return 0;
}

static asciichat_hip_box_t *box_of(const asciichat_hip_box_t *box) { return box && box->magic == BOX_MAGIC ? (asciichat_hip_box_t *)box : NULL; }

static void box_free(asciichat_hip_box_t *b, int n_ev) {
  for (int s = 0; s < n_ev; s++) {
    if (b->ev_used[s])
      (void)hipEventSynchronize(b->ev[s]);
    (void)hipEventDestroy(b->ev[s]);
  }
  (void)hipFree(b->slab);
  (void)hipFree(b->desc_dev);
  if (b->ring)
    (void)hipHostFree(b->ring);
  b->magic = 0;
  free(b->frames);
  free(b);
}

/* a new box of the (checked) batch; the ring is sized for the worst case, n composite frames of 9 tiles of their own each,
 * so that either entry may update any box */
static int box_new(asciichat_hip_box_t **box, const achip_frame_t *frames, const achip_composite_t *const *comps, int n_frames,
                   hipStream_t stream) {
  int rc = achip_require_device();
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
  b->seg_bytes = (sizeof(achip_box_canvas_t) + 10u * sizeof(achip_box_desc_t)) * (size_t)n_frames;
  int n_ev = 0;
  rc = achip_hip_check((int)hipGetDevice(&b->device), "hipGetDevice");
  if (!rc)
    rc = achip_hip_check((int)hipHostMalloc((void **)&b->ring, b->seg_bytes * BOX_RING, hipHostMallocDefault), "hipHostMalloc(box descriptors)");
  if (!rc)
    rc = achip_hip_check((int)hipMalloc((void **)&b->desc_dev, b->seg_bytes), "hipMalloc(box descriptors)");
  for (; !rc && n_ev < BOX_RING; n_ev++)
    rc = achip_hip_check((int)hipEventCreateWithFlags(&b->ev[n_ev], hipEventDisableTiming), "hipEventCreate(box)");
  if (rc)
    n_ev--; /* the one that failed does not exist */
  if (!rc)
    rc = box_set(b, frames, comps, stream, 1); /* uploaded before create returns: the first run may be on any stream */
  if (rc) {
    box_free(b, n_ev);
    return rc;
  }
  *box = b;
  return 0;
}

int asciichat_hip_box_create(asciichat_hip_box_t **box, const achip_frame_t *frames, int n_frames) {
  if (!box || !frames || n_frames <= 0)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box_create: bad arguments");
  *box = NULL;
  const int rc = frames_check(frames, NULL, n_frames);
  return rc ? rc : box_new(box, frames, NULL, n_frames, NULL);
}

int asciichat_hip_box_update(asciichat_hip_box_t *box, const achip_frame_t *frames, void *stream) {
  asciichat_hip_box_t *b = box_of(box);
  if (!b || !frames)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box_update: bad arguments");
  const int rc = frames_check(frames, NULL, b->n);
  return rc ? rc : box_set(b, frames, NULL, (hipStream_t)stream, 0);
}

int asciichat_hip_box_composites(asciichat_hip_box_t **box, const achip_frame_t *frames, const achip_composite_t *const *comps_host,
                                 int n_frames, void *stream) {
  if (!box || !frames || !comps_host || n_frames <= 0)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box_composites: bad arguments");
  asciichat_hip_box_t *b = NULL;
  if (*box) {
    b = box_of(*box);
    if (!b)
      return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box_composites: not a box");
    if (b->n != n_frames)
      return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box_composites: %d frames for a box of %d", n_frames, b->n);
  }
  const int rc = frames_check(frames, comps_host, n_frames);
  if (rc)
    return rc;
  if (!b)
    return box_new(box, frames, comps_host, n_frames, (hipStream_t)stream);
  return box_set(b, frames, comps_host, (hipStream_t)stream, 0);
}

size_t asciichat_hip_box_image_pitch(const asciichat_hip_box_t *box) {
  const asciichat_hip_box_t *b = box_of(box);
  return b ? ((size_t)b->plan.image_bytes + 127u) & ~(size_t)127u : 0;
}

int asciichat_hip_box_run(asciichat_hip_box_t *box, uint8_t *images_dev, size_t pitch, void *stream) {
  asciichat_hip_box_t *b = box_of(box);
  if (!b || !images_dev)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box_run: bad arguments");
  if (pitch < (size_t)b->plan.image_bytes)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box_run: pitch %zu below an image's %zu bytes", pitch, (size_t)b->plan.image_bytes);
  /* up to three launches, none with nothing to do: the plain frames into their images, the unique tiles of the composite
   * frames into the scratch slab, the composite frames assembled from those tiles into their images */
  const achip_box_plan_t *p = &b->plan;
  const uint8_t *canvas_dev = b->desc_dev + sizeof(achip_box_desc_t) * (size_t)b->n;
  const uint8_t *tiles_dev = canvas_dev + sizeof(achip_box_canvas_t) * (size_t)p->n_canvas;
  int rc = 0;
  if (p->n_plain)
    rc = achip_hip_check(achip_launch_box((const achip_box_desc_t *)b->desc_dev, &b->uni, b->n, p->plain_max_out_h, p->plain_max_src_w,
                                          images_dev, (uint64_t)pitch, stream),
                         "box launch");
  if (!rc && p->n_tiles)
    rc = achip_hip_check(achip_launch_box((const achip_box_desc_t *)tiles_dev, NULL, p->n_tiles, p->tile_max_out_h, p->tile_max_src_w,
                                          b->slab, p->tile_pitch, stream),
                         "box tile launch");
  if (!rc && p->n_canvas)
    rc = achip_hip_check(box_canvas_launch((const achip_box_canvas_t *)canvas_dev, p->n_canvas, p->canvas_max_out_h, p->canvas_max_w,
                                           b->slab, p->tile_pitch, images_dev, (uint64_t)pitch, stream),
                         "box canvas launch");
  return rc;
}

int asciichat_hip_box_get_uniform(const asciichat_hip_box_t *box) {
  const asciichat_hip_box_t *b = box_of(box);
  return b ? (int)b->uni.enabled : 0;
}

int asciichat_hip_box_render_frames(const asciichat_hip_box_t *box, const uint8_t *images_dev, size_t pitch, achip_frame_t *frames_out) {
  const asciichat_hip_box_t *b = box_of(box);
  if (!b || !images_dev || !frames_out)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box_render_frames: bad arguments");
  if (pitch < (size_t)b->plan.image_bytes)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "box_render_frames: pitch %zu below an image's %zu bytes", pitch, (size_t)b->plan.image_bytes);
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
  box_free(b, BOX_RING);
  (void)hipSetDevice(cur);
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
  int rc = frames_check(&f, NULL, 1);
  if (!rc)
    rc = achip_require_device();
  if (rc)
    return rc;
  (void)achip_box_desc_from_frame(&f, &uni.d);
  uni.enabled = 1;
  return achip_hip_check(achip_launch_box(NULL, &uni, 1, dst_h, src_w, dst_dev, 3u * (uint64_t)dst_w * (uint64_t)dst_h, stream), "box launch");
}
