/*
 * yuvboxgrid.c -- the host side of libasciichat_yuvboxgrid.so (include/asciichat_yuvboxgrid.h): a set of composites and their YUV
 * sources is checked on the host (yuvboxgrid.h) before anything of the handle changes, then staged as items -- the workgroup
 * table in them -- through the one pinned block the handle owns and copied by one asynchronous transfer on the caller's stream;
 * run() only launches (yuvboxgrid.hip), composites() only rewrites the descriptors the set came with (yuvgrid_math.h's
 * rewrite).  Both blocks are allocated by create(); nothing allocates afterwards.  Nothing here comes from the other five
 * libraries.
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "asciichat_yuvboxgrid.h"
#include "yuvboxgrid.h"

#define YUVBOXGRID_MAGIC 0x5955564258475231ull

struct asciichat_yuvboxgrid {
  uint64_t magic;
  int device, max_tiles;
  uint8_t *dev, *pinned;    /* one block each, max_tiles items */
  achip_composite_t *comps; /* the descriptors of the last set as given (host): composites() rewrites these */
  uint16_t *masks;          /* per composite of the last set: bit k, slot k is a YUV slot */
  int n_comps;              /* composites of the last set, 0 before any */
  int n_tiles;              /* its YUV slots */
  int dma_queued;           /* the pinned block may still be read by the copy of the last set */
  yuvgrid_item_t *layout;   /* max_tiles of yuvgrid_math.h's items (host): the slab's layout is yuvgrid_fill's own */
  uint32_t workgroups;      /* of the last set's launch */
  uint32_t stage_cols;      /* the widest LDS stage among its tiles, in columns */
  uint64_t tiles_bytes;     /* the slab of the last set */
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

const char *asciichat_yuvboxgrid_last_error(void) { return g_error; }

int asciichat_yuvboxgrid_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

static asciichat_yuvboxgrid_t *boxgrid_of(const asciichat_yuvboxgrid_t *g) {
  return g && g->magic == YUVBOXGRID_MAGIC ? (asciichat_yuvboxgrid_t *)g : NULL;
}

static void boxgrid_free(asciichat_yuvboxgrid_t *h) {
  (void)hipFree(h->dev);
  if (h->pinned)
    (void)hipHostFree(h->pinned);
  free(h->comps);
  free(h->masks);
  free(h->layout);
  h->magic = 0;
  free(h);
}

int asciichat_yuvboxgrid_create(asciichat_yuvboxgrid_t **g, int max_tiles) {
  if (!g)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuvboxgrid_create: no handle");
  *g = NULL;
  if (max_tiles < 1 || max_tiles > YUVGRID_MAX_TILES)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuvboxgrid_create: max_tiles %d outside 1..%d", max_tiles, YUVGRID_MAX_TILES);
  if (asciichat_yuvboxgrid_device_count() <= 0)
    return fail(ASCIICHAT_YUV_ERR_NO_DEVICE, "yuvboxgrid_create: no HIP device");
  asciichat_yuvboxgrid_t *h = (asciichat_yuvboxgrid_t *)calloc(1, sizeof(*h));
  achip_composite_t *comps = (achip_composite_t *)calloc((size_t)max_tiles, sizeof(achip_composite_t));
  uint16_t *masks = (uint16_t *)calloc((size_t)max_tiles, sizeof(uint16_t));
  yuvgrid_item_t *layout = (yuvgrid_item_t *)calloc((size_t)max_tiles, sizeof(yuvgrid_item_t));
  if (!h || !comps || !masks || !layout) {
    free(h);
    free(comps);
    free(masks);
    free(layout);
    return fail(ASCIICHAT_YUV_ERR_MEMORY, "yuvboxgrid_create: out of memory");
  }
  h->magic = YUVBOXGRID_MAGIC;
  h->max_tiles = max_tiles;
  h->comps = comps;
  h->masks = masks;
  h->layout = layout;
  const size_t bytes = (size_t)max_tiles * sizeof(yuvboxgrid_item_t);
  int rc = hip_check(hipGetDevice(&h->device), "hipGetDevice");
  if (!rc)
    rc = hip_check(hipMalloc((void **)&h->dev, bytes), "hipMalloc(yuvboxgrid set)");
  if (!rc)
    rc = hip_check(hipHostMalloc((void **)&h->pinned, bytes, hipHostMallocDefault), "hipHostMalloc(yuvboxgrid set)");
  if (rc) {
    boxgrid_free(h);
    return rc;
  }
  *g = h;
  return 0;
}

int asciichat_yuvboxgrid_set(asciichat_yuvboxgrid_t *g, const achip_composite_t *const *comps_host, const asciichat_yuv_source_t *const *sources,
                          int n_comps, void *stream) {
  asciichat_yuvboxgrid_t *h = boxgrid_of(g);
  if (!h)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuvboxgrid_set: not a handle");
  int bad_comp = -1, bad_slot = -1, n_tiles = 0;
  const char *why = yuvboxgrid_set_check(comps_host, sources, n_comps, h->max_tiles, YUVBOXGRID_SEG_COLS, &bad_comp, &bad_slot, &n_tiles);
  if (why) {
    if (bad_comp >= 0 && bad_slot >= 0)
      return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuvboxgrid_set: composite %d slot %d: %s", bad_comp, bad_slot, why);
    if (bad_comp >= 0)
      return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuvboxgrid_set: composite %d: %s", bad_comp, why);
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuvboxgrid_set: %s", why);
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
  uint32_t workgroups = 0u, stage_cols = 0u;
  const uint64_t tiles_bytes = yuvboxgrid_fill(comps_host, sources, n_comps, YUVBOXGRID_SEG_COLS, h->layout, (yuvboxgrid_item_t *)h->pinned, h->masks,
                                               &workgroups, &stage_cols);
  for (int c = 0; c < n_comps; c++)
    h->comps[c] = *comps_host[c];
  if (n_tiles) {
    const int rc = hip_check(hipMemcpyAsync(h->dev, h->pinned, (size_t)n_tiles * sizeof(yuvboxgrid_item_t), hipMemcpyHostToDevice, (hipStream_t)stream),
                             "hipMemcpyAsync(yuvboxgrid set)");
    if (rc)
      return rc;
    h->dma_queued = 1;
  }
  h->n_comps = n_comps;
  h->n_tiles = n_tiles;
  h->workgroups = workgroups;
  h->stage_cols = stage_cols;
  h->tiles_bytes = tiles_bytes;
  return 0;
}

size_t asciichat_yuvboxgrid_tiles_bytes(const asciichat_yuvboxgrid_t *g) {
  const asciichat_yuvboxgrid_t *h = boxgrid_of(g);
  return h && h->n_comps ? (size_t)h->tiles_bytes : 0;
}

/* what run and composites ask of a handle and of the slab's place */
static int slab_ok(const asciichat_yuvboxgrid_t *h, const uint8_t *tiles_dev, const char *what) {
  if (!h)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "%s: not a handle", what);
  if (!h->n_comps)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "%s: nothing is set (asciichat_yuvboxgrid_set)", what);
  if (h->n_tiles && (!tiles_dev || ((uintptr_t)tiles_dev & 15u)))
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "%s: a tile slab at a multiple of 16 is required", what);
  return 0;
}

int asciichat_yuvboxgrid_run(asciichat_yuvboxgrid_t *g, uint8_t *tiles_dev, void *stream) {
  asciichat_yuvboxgrid_t *h = boxgrid_of(g);
  const int rc = slab_ok(h, tiles_dev, "yuvboxgrid_run");
  if (rc)
    return rc;
  if (!h->n_tiles)
    return 0; /* nothing to average: nothing is launched */
  return hip_check((hipError_t)yuvboxgrid_launch((const yuvboxgrid_item_t *)h->dev, h->n_tiles, h->workgroups, h->stage_cols, tiles_dev, stream),
                   "yuvboxgrid tile launch");
}

int asciichat_yuvboxgrid_composites(const asciichat_yuvboxgrid_t *g, const uint8_t *tiles_dev, achip_composite_t *comps_out) {
  const asciichat_yuvboxgrid_t *h = boxgrid_of(g);
  const int rc = slab_ok(h, tiles_dev, "yuvboxgrid_composites");
  if (rc)
    return rc;
  if (!comps_out)
    return fail(ASCIICHAT_YUV_ERR_INVALID_PARAM, "yuvboxgrid_composites: no descriptors to write");
  uint64_t at = 0;
  for (int c = 0; c < h->n_comps; c++)
    yuvgrid_rewrite(&h->comps[c], h->masks[c], tiles_dev, &at, &comps_out[c]);
  return 0;
}

void asciichat_yuvboxgrid_destroy(asciichat_yuvboxgrid_t *g) {
  asciichat_yuvboxgrid_t *h = boxgrid_of(g);
  if (!h)
    return;
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(h->device);
  boxgrid_free(h);
  (void)hipSetDevice(cur);
}
