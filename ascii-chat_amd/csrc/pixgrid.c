/*
 * pixgrid.c -- the host side of libasciichat_pixgrid.so (include/asciichat_pixgrid.h): a set of composites and their packed RGB
 * sources is checked on the host (pixgrid.h) before anything of the handle changes, then staged as items -- the sampling ratios
 * and the averaged pass's workgroup table both in them -- through the one pinned block the handle owns and copied by one
 * asynchronous transfer on the caller's stream; run() and run_box() only launch (pixgrid.hip), composites() only rewrites the
 * descriptors the set came with (yuvgrid_math.h's rewrite).  Both blocks are allocated by create(); nothing allocates
 * afterwards.  Nothing here comes from the other seven libraries.
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "asciichat_pixgrid.h"
#include "pixgrid.h"

#define PIXGRID_MAGIC 0x5049584752494431ull

struct asciichat_pixgrid {
  uint64_t magic;
  int device, max_tiles;
  uint8_t *dev, *pinned;       /* one block each, max_tiles items */
  achip_composite_t *comps;    /* the descriptors of the last set as given (host): composites() rewrites these */
  uint16_t *masks;             /* per composite of the last set: bit k, slot k is a packed slot */
  int n_comps;                 /* composites of the last set, 0 before any */
  int n_tiles;                 /* its packed slots */
  int dma_queued;              /* the pinned block may still be read by the copy of the last set */
  pixgrid_launches_t launches; /* what run and run_box launch the last set with */
  uint64_t tiles_bytes;        /* the slab of the last set */
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

const char *asciichat_pixgrid_last_error(void) { return g_error; }

int asciichat_pixgrid_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

static asciichat_pixgrid_t *pixgrid_of(const asciichat_pixgrid_t *g) {
  return g && g->magic == PIXGRID_MAGIC ? (asciichat_pixgrid_t *)g : NULL;
}

static void pixgrid_free(asciichat_pixgrid_t *h) {
  (void)hipFree(h->dev);
  if (h->pinned)
    (void)hipHostFree(h->pinned);
  free(h->comps);
  free(h->masks);
  h->magic = 0;
  free(h);
}

int asciichat_pixgrid_create(asciichat_pixgrid_t **g, int max_tiles) {
  if (!g)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pixgrid_create: no handle");
  *g = NULL;
  if (max_tiles < 1 || max_tiles > PIXGRID_MAX_TILES)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pixgrid_create: max_tiles %d outside 1..%d", max_tiles, PIXGRID_MAX_TILES);
  if (asciichat_pixgrid_device_count() <= 0)
    return fail(ASCIICHAT_PIX_ERR_NO_DEVICE, "pixgrid_create: no HIP device");
  asciichat_pixgrid_t *h = (asciichat_pixgrid_t *)calloc(1, sizeof(*h));
  achip_composite_t *comps = (achip_composite_t *)calloc((size_t)max_tiles, sizeof(achip_composite_t));
  uint16_t *masks = (uint16_t *)calloc((size_t)max_tiles, sizeof(uint16_t));
  if (!h || !comps || !masks) {
    free(h);
    free(comps);
    free(masks);
    return fail(ASCIICHAT_PIX_ERR_MEMORY, "pixgrid_create: out of memory");
  }
  h->magic = PIXGRID_MAGIC;
  h->max_tiles = max_tiles;
  h->comps = comps;
  h->masks = masks;
  const size_t bytes = (size_t)max_tiles * sizeof(pixgrid_item_t);
  int rc = hip_check(hipGetDevice(&h->device), "hipGetDevice");
  if (!rc)
    rc = hip_check(hipMalloc((void **)&h->dev, bytes), "hipMalloc(pixgrid set)");
  if (!rc)
    rc = hip_check(hipHostMalloc((void **)&h->pinned, bytes, hipHostMallocDefault), "hipHostMalloc(pixgrid set)");
  if (rc) {
    pixgrid_free(h);
    return rc;
  }
  *g = h;
  return 0;
}

int asciichat_pixgrid_set(asciichat_pixgrid_t *g, const achip_composite_t *const *comps_host, const asciichat_pix_source_t *const *sources,
                          int n_comps, void *stream) {
  asciichat_pixgrid_t *h = pixgrid_of(g);
  if (!h)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pixgrid_set: not a handle");
  int bad_comp = -1, bad_slot = -1, n_tiles = 0;
  const char *why = pixgrid_set_check(comps_host, sources, n_comps, h->max_tiles, PIXGRID_SEG_COLS, &bad_comp, &bad_slot, &n_tiles);
  if (why) {
    if (bad_comp >= 0 && bad_slot >= 0)
      return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pixgrid_set: composite %d slot %d: %s", bad_comp, bad_slot, why);
    if (bad_comp >= 0)
      return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pixgrid_set: composite %d: %s", bad_comp, why);
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pixgrid_set: %s", why);
  }
  /* the pinned block may still be in flight from the set before, on this stream (a handle's calls are ordered on one): wait
   * before it is overwritten, and before anything of the handle changes */
  if (h->dma_queued) {
    const int rc = hip_check(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
    if (rc)
      return rc;
  }
  h->dma_queued = 0;
  h->n_comps = 0; /* (should the copy fail, nothing is set) */
  pixgrid_launches_t launches;
  const uint64_t tiles_bytes = pixgrid_fill(comps_host, sources, n_comps, PIXGRID_SEG_COLS, (pixgrid_item_t *)h->pinned, h->masks, &launches);
  for (int c = 0; c < n_comps; c++)
    h->comps[c] = *comps_host[c];
  if (n_tiles) {
    const int rc = hip_check(hipMemcpyAsync(h->dev, h->pinned, (size_t)n_tiles * sizeof(pixgrid_item_t), hipMemcpyHostToDevice, (hipStream_t)stream),
                             "hipMemcpyAsync(pixgrid set)");
    if (rc)
      return rc;
    h->dma_queued = 1;
  }
  h->n_comps = n_comps;
  h->n_tiles = n_tiles;
  h->launches = launches;
  h->tiles_bytes = tiles_bytes;
  return 0;
}

size_t asciichat_pixgrid_tiles_bytes(const asciichat_pixgrid_t *g) {
  const asciichat_pixgrid_t *h = pixgrid_of(g);
  return h && h->n_comps ? (size_t)h->tiles_bytes : 0;
}

/* what run, run_box and composites ask of a handle and of the slab's place */
static int slab_ok(const asciichat_pixgrid_t *h, const uint8_t *tiles_dev, const char *what) {
  if (!h)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "%s: not a handle", what);
  if (!h->n_comps)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "%s: nothing is set (asciichat_pixgrid_set)", what);
  if (h->n_tiles && (!tiles_dev || ((uintptr_t)tiles_dev & 15u)))
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "%s: a tile slab at a multiple of 16 is required", what);
  return 0;
}

int asciichat_pixgrid_run(asciichat_pixgrid_t *g, uint8_t *tiles_dev, void *stream) {
  asciichat_pixgrid_t *h = pixgrid_of(g);
  const int rc = slab_ok(h, tiles_dev, "pixgrid_run");
  if (rc)
    return rc;
  if (!h->n_tiles)
    return 0; /* nothing to sample: nothing is launched */
  return hip_check((hipError_t)pixgrid_launch_tiles((const pixgrid_item_t *)h->dev, h->n_tiles, h->launches.max_pixels, tiles_dev, stream),
                   "pixgrid tile launch");
}

int asciichat_pixgrid_run_box(asciichat_pixgrid_t *g, uint8_t *tiles_dev, void *stream) {
  asciichat_pixgrid_t *h = pixgrid_of(g);
  const int rc = slab_ok(h, tiles_dev, "pixgrid_run_box");
  if (rc)
    return rc;
  if (!h->n_tiles)
    return 0; /* nothing to average: nothing is launched */
  if (!h->launches.boxable)
    return fail(ASCIICHAT_PIX_ERR_NOT_SUPPORTED, "pixgrid_run_box: a source of the set is larger than %d x %d (asciichat_pixgrid_run serves it)",
                PIX_BOX_MAX_SRC_W, PIX_BOX_MAX_SRC_H);
  return hip_check((hipError_t)pixgrid_launch_box((const pixgrid_item_t *)h->dev, h->n_tiles, h->launches.workgroups, h->launches.stage_cols,
                                                  tiles_dev, stream),
                   "pixgrid averaged tile launch");
}

int asciichat_pixgrid_composites(const asciichat_pixgrid_t *g, const uint8_t *tiles_dev, achip_composite_t *comps_out) {
  const asciichat_pixgrid_t *h = pixgrid_of(g);
  const int rc = slab_ok(h, tiles_dev, "pixgrid_composites");
  if (rc)
    return rc;
  if (!comps_out)
    return fail(ASCIICHAT_PIX_ERR_INVALID_PARAM, "pixgrid_composites: no descriptors to write");
  uint64_t at = 0;
  for (int c = 0; c < h->n_comps; c++)
    yuvgrid_rewrite(&h->comps[c], h->masks[c], tiles_dev, &at, &comps_out[c]);
  return 0;
}

void asciichat_pixgrid_destroy(asciichat_pixgrid_t *g) {
  asciichat_pixgrid_t *h = pixgrid_of(g);
  if (!h)
    return;
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(h->device);
  pixgrid_free(h);
  (void)hipSetDevice(cur);
}
