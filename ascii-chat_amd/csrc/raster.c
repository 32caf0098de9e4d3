/*
 * raster.c -- the host side of libasciichat_raster.so (include/asciichat_raster.h): a handle checks its font and grid before
 * it needs a device (raster.h), uploads the atlas and the lookup tables once and owns every byte of scratch a run uses --
 * cells, row starts and row records for max_frames frames --, so that run() only launches (raster.hip) on the caller's
 * stream.  The cells may also come straight from frame descriptors (images_set and the entries behind it, raster_images.h): a
 * set is checked on the host and staged through one pinned block of the handle's.  Nothing here comes from
 * libasciichat_hip.so.
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "asciichat_raster.h"
#include "raster.h"
#include "raster_images.h"

#define RASTER_MAGIC 0x5241535445523031ull

struct asciichat_raster {
  uint64_t magic;
  int device, max_frames;
  raster_params_t p;
  uint8_t *tables; /* one allocation: codepoints, glyphs, lut, coverage */
  uint32_t *starts;
  raster_rowrec_t *recs;
  raster_cell_t *cells;
  /* cells from images (raster_images.h): the atlas' codepoints for the slot table, the last set and where it is staged */
  uint32_t *codepoints_host;
  uint8_t *img_dev, *img_pinned; /* one block each: the table, then max_frames descriptors; allocated by the first images_set */
  raster_img_args_t img;
  int img_n;          /* frames of the last set, 0 before any */
  int img_comp;       /* some frame of the last set carries a composite: the kernel form with the staged sampler */
  int img_dma_queued; /* the pinned block may still be read by the copy of the last set */
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
  return fail(e == hipErrorOutOfMemory ? ASCIICHAT_RASTER_ERR_MEMORY : ASCIICHAT_RASTER_ERR_NO_DEVICE, "%s: %s", what, hipGetErrorString(e));
}

const char *asciichat_raster_last_error(void) { return g_error; }

int asciichat_raster_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

static asciichat_raster_t *raster_of(const asciichat_raster_t *r) { return r && r->magic == RASTER_MAGIC ? (asciichat_raster_t *)r : NULL; }

static void raster_free(asciichat_raster_t *h) {
  (void)hipFree(h->cells);
  (void)hipFree(h->recs);
  (void)hipFree(h->starts);
  (void)hipFree(h->tables);
  (void)hipFree(h->img_dev);
  if (h->img_pinned)
    (void)hipHostFree(h->img_pinned);
  free(h->codepoints_host);
  h->magic = 0;
  free(h);
}

static size_t round16(size_t v) { return (v + 15u) & ~(size_t)15u; }

int asciichat_raster_create(asciichat_raster_t **r, const asciichat_raster_font_t *font, int cols, int rows, int max_frames) {
  if (!r)
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "raster_create: no handle");
  *r = NULL;
  const char *why = raster_check(font, cols, rows, max_frames);
  if (why)
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "raster_create: %s", why);
  if (asciichat_raster_device_count() <= 0)
    return fail(ASCIICHAT_RASTER_ERR_NO_DEVICE, "raster_create: no HIP device");
  asciichat_raster_t *h = (asciichat_raster_t *)calloc(1, sizeof(*h));
  /* the tables as one host block, laid out as on the device */
  const size_t ng = (size_t)font->n_glyphs;
  const size_t at_glyphs = round16(4u * ng), at_lut = at_glyphs + sizeof(raster_glyph_t) * ng, at_cov = at_lut + 4u * 512u;
  const size_t bytes = at_cov + round16(font->coverage_bytes) + 16u;
  uint8_t *host = (uint8_t *)calloc(1, bytes);
  uint32_t *cps = (uint32_t *)calloc(ng + 1u, sizeof(uint32_t));
  if (!h || !host || !cps) {
    free(h);
    free(host);
    free(cps);
    return fail(ASCIICHAT_RASTER_ERR_MEMORY, "raster_create: out of memory");
  }
  raster_tables(font, (uint32_t *)host, (raster_glyph_t *)(host + at_glyphs), (uint32_t *)(host + at_lut));
  memcpy(cps, host, 4u * ng);
  h->codepoints_host = cps;
  if (font->coverage_bytes)
    memcpy(host + at_cov, font->coverage, font->coverage_bytes);
  h->magic = RASTER_MAGIC;
  h->max_frames = max_frames;
  const size_t n = (size_t)max_frames, nr = (size_t)rows, nc = (size_t)cols;
  int rc = hip_check(hipGetDevice(&h->device), "hipGetDevice");
  if (!rc)
    rc = hip_check(hipMalloc((void **)&h->tables, bytes), "hipMalloc(raster tables)");
  if (!rc)
    rc = hip_check(hipMalloc((void **)&h->starts, 4u * n * (nr + 2u)), "hipMalloc(raster row starts)");
  if (!rc)
    rc = hip_check(hipMalloc((void **)&h->recs, sizeof(raster_rowrec_t) * n * (nr + 1u)), "hipMalloc(raster row records)");
  if (!rc)
    rc = hip_check(hipMalloc((void **)&h->cells, sizeof(raster_cell_t) * n * nr * nc), "hipMalloc(raster cells)");
  if (!rc)
    rc = hip_check(hipMemcpy(h->tables, host, bytes, hipMemcpyHostToDevice), "hipMemcpy(raster tables)"); /* landed on return */
  free(host);
  if (rc) {
    raster_free(h);
    return rc;
  }
  raster_params_t *p = &h->p;
  p->cols = cols, p->rows = rows, p->cell_w = font->cell_w, p->cell_h = font->cell_h;
  p->n_glyphs = font->n_glyphs, p->matrix_map = font->matrix_map != 0;
  p->default_fg = font->default_fg & 0xFFFFFFu, p->default_bg = font->default_bg & 0xFFFFFFu;
  p->codepoints = (const uint32_t *)h->tables;
  p->glyphs = (const raster_glyph_t *)(h->tables + at_glyphs);
  p->lut = (const uint32_t *)(h->tables + at_lut);
  p->coverage = h->tables + at_cov;
  p->coverage_bytes = (uint32_t)font->coverage_bytes;
  p->atlas_in_lds = font->coverage_bytes <= RASTER_ATLAS_LDS;
  *r = h;
  return 0;
}

int asciichat_raster_width_px(const asciichat_raster_t *r) {
  const asciichat_raster_t *h = raster_of(r);
  return h ? h->p.cols * h->p.cell_w : 0;
}

int asciichat_raster_height_px(const asciichat_raster_t *r) {
  const asciichat_raster_t *h = raster_of(r);
  return h ? h->p.rows * h->p.cell_h : 0;
}

size_t asciichat_raster_image_pitch(const asciichat_raster_t *r) {
  return 4u * (size_t)asciichat_raster_width_px(r) * (size_t)asciichat_raster_height_px(r);
}

static int frames_ok(const asciichat_raster_t *h, int n, const char *what) {
  if (!h)
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "%s: not a rasteriser", what);
  if (n < 1 || n > h->max_frames)
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "%s: %d frames for a rasteriser of 1..%d", what, n, h->max_frames);
  return 0;
}

int asciichat_raster_parse(asciichat_raster_t *r, const uint8_t *frames_dev, size_t frame_stride, const uint32_t *len_dev, int n,
                           uint32_t *status_dev, void *stream) {
  asciichat_raster_t *h = raster_of(r);
  const int rc = frames_ok(h, n, "raster_parse");
  if (rc)
    return rc;
  if (!frames_dev || !len_dev || !status_dev)
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "raster_parse: frames, lengths and a status array are required");
  if (frame_stride > 0x7FFFFFFFu) /* (byte positions in a frame are 32-bit) */
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "raster_parse: frame stride %zu beyond 2^31 - 1", frame_stride);
  return hip_check((hipError_t)raster_launch_parse(&h->p, frames_dev, (uint64_t)frame_stride, len_dev, n, h->starts, h->recs, h->cells,
                                                   status_dev, stream),
                   "raster parse launch");
}

int asciichat_raster_draw(asciichat_raster_t *r, int n, uint8_t *pixels_dev, size_t image_pitch, void *stream) {
  asciichat_raster_t *h = raster_of(r);
  const int rc = frames_ok(h, n, "raster_draw");
  if (rc)
    return rc;
  if (!pixels_dev || ((uintptr_t)pixels_dev & 3u) || (image_pitch & 3u))
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "raster_draw: 4-byte aligned pixels and image pitch are required");
  if (image_pitch < asciichat_raster_image_pitch(h))
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "raster_draw: pitch %zu below an image's %zu bytes", image_pitch,
                asciichat_raster_image_pitch(h));
  return hip_check((hipError_t)raster_launch_draw(&h->p, h->cells, n, pixels_dev, (uint64_t)image_pitch, stream), "raster draw launch");
}

int asciichat_raster_run(asciichat_raster_t *r, const uint8_t *frames_dev, size_t frame_stride, const uint32_t *len_dev, int n,
                         uint8_t *pixels_dev, size_t image_pitch, uint32_t *status_dev, void *stream) {
  asciichat_raster_t *h = raster_of(r);
  int rc = frames_ok(h, n, "raster_run");
  if (rc)
    return rc;
  /* nothing is launched unless both stages take their arguments */
  if (!pixels_dev || ((uintptr_t)pixels_dev & 3u) || (image_pitch & 3u) || image_pitch < asciichat_raster_image_pitch(h))
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "raster_run: 4-byte aligned pixels and an image pitch of at least %zu are required",
                asciichat_raster_image_pitch(h));
  rc = asciichat_raster_parse(r, frames_dev, frame_stride, len_dev, n, status_dev, stream);
  return rc ? rc : asciichat_raster_draw(r, n, pixels_dev, image_pitch, stream);
}

size_t asciichat_raster_yuv420_bytes(int width_px, int height_px) {
  if (width_px < 2 || height_px < 2 || (width_px & 1) || (height_px & 1))
    return 0;
  return (size_t)width_px * (size_t)height_px / 2u * 3u;
}

size_t asciichat_raster_yuv420_pitch(const asciichat_raster_t *r) {
  return asciichat_raster_yuv420_bytes(asciichat_raster_width_px(r), asciichat_raster_height_px(r));
}

/* what both YUV entries ask of their output; nothing is launched unless it holds */
static int yuv_ok(const asciichat_raster_t *h, int n, const uint8_t *yuv_dev, size_t image_pitch, int layout, const char *what) {
  const int rc = frames_ok(h, n, what);
  if (rc)
    return rc;
  const size_t need = asciichat_raster_yuv420_pitch(h);
  if (!need)
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "%s: a %d x %d image has no 4:2:0 planes: both must be even", what,
                asciichat_raster_width_px(h), asciichat_raster_height_px(h));
  if (layout != ASCIICHAT_RASTER_YUV_I420 && layout != ASCIICHAT_RASTER_YUV_NV12)
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "%s: layout %d is neither I420 nor NV12", what, layout);
  if (!yuv_dev || ((uintptr_t)yuv_dev & 3u) || (image_pitch & 3u))
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "%s: 4-byte aligned planes and image pitch are required", what);
  if (image_pitch < need)
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "%s: pitch %zu below an image's %zu bytes", what, image_pitch, need);
  return 0;
}

int asciichat_raster_draw_yuv420(asciichat_raster_t *r, int n, uint8_t *yuv_dev, size_t image_pitch, int layout, void *stream) {
  asciichat_raster_t *h = raster_of(r);
  const int rc = yuv_ok(h, n, yuv_dev, image_pitch, layout, "raster_draw_yuv420");
  if (rc)
    return rc;
  return hip_check((hipError_t)raster_launch_draw_yuv(&h->p, h->cells, n, yuv_dev, (uint64_t)image_pitch, layout, stream),
                   "raster yuv draw launch");
}

int asciichat_raster_run_yuv420(asciichat_raster_t *r, const uint8_t *frames_dev, size_t frame_stride, const uint32_t *len_dev, int n,
                                uint8_t *yuv_dev, size_t image_pitch, int layout, uint32_t *status_dev, void *stream) {
  int rc = yuv_ok(raster_of(r), n, yuv_dev, image_pitch, layout, "raster_run_yuv420");
  if (rc)
    return rc;
  rc = asciichat_raster_parse(r, frames_dev, frame_stride, len_dev, n, status_dev, stream);
  return rc ? rc : asciichat_raster_draw_yuv420(r, n, yuv_dev, image_pitch, layout, stream);
}

/* ---- cells straight from frame descriptors (raster_images.h) ---- */

/* a checked set (composites: how many of its frames carry comp) becomes the handle's */
static int images_stage(asciichat_raster_t *h, int mode, const char *palette_chars, const achip_frame_t *frames, int n, int composites,
                        void *stream) {
  int rc = 0;
  if (!h->img_dev) { /* the first set of this handle: both blocks, sized by max_frames; later sets allocate nothing */
    const size_t bytes = raster_images_bytes(h->max_frames);
    uint8_t *dev = NULL, *pinned = NULL;
    rc = hip_check(hipMalloc((void **)&dev, bytes), "hipMalloc(raster images)");
    if (!rc)
      rc = hip_check(hipHostMalloc((void **)&pinned, bytes, hipHostMallocDefault), "hipHostMalloc(raster images)");
    if (rc) {
      (void)hipFree(dev);
      return rc;
    }
    h->img_dev = dev;
    h->img_pinned = pinned;
  }
  /* the pinned block may still be in flight from the set before, on this stream (a handle's calls are ordered on one):
   * wait before it is overwritten, and before anything of the handle changes */
  if (h->img_dma_queued)
    rc = hip_check(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
  if (rc)
    return rc;
  h->img_dma_queued = 0;
  raster_img_tables_t *t = (raster_img_tables_t *)h->img_pinned;
  uint32_t mixed = 0u;
  if (mode == ACHIP_MODE_16_DITHER_BG) /* (images_set_dithered alone comes here with this mode) */
    raster_images_dither_tables(palette_chars, h->codepoints_host, h->p.n_glyphs, h->p.matrix_map, t);
  else
    mixed = raster_images_tables(mode, palette_chars, h->codepoints_host, h->p.n_glyphs, h->p.matrix_map, t);
  memcpy(h->img_pinned + raster_images_at_frames(), frames, (size_t)n * sizeof(achip_frame_t));
  h->img_n = 0; /* (should the copy fail, nothing is set) */
  rc = hip_check(hipMemcpyAsync(h->img_dev, h->img_pinned, raster_images_bytes(n), hipMemcpyHostToDevice, (hipStream_t)stream),
                 "hipMemcpyAsync(raster images)");
  if (rc)
    return rc;
  h->img_dma_queued = 1;
  h->img.mode = mode;
  h->img.mixed = mixed;
  h->img.tables = (const raster_img_tables_t *)h->img_dev;
  h->img.frames = (const achip_frame_t *)(h->img_dev + raster_images_at_frames());
  h->img_comp = composites > 0;
  h->img_n = n;
  return 0;
}

static int images_refused(const char *what, int bad, const char *why) {
  return bad >= 0 ? fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "%s: frame %d: %s", what, bad, why)
                  : fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "%s: %s", what, why);
}

int asciichat_raster_images_set(asciichat_raster_t *r, int mode, const char *palette_chars, const achip_frame_t *frames, int n,
                                void *stream) {
  asciichat_raster_t *h = raster_of(r);
  if (!h)
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "raster_images_set: not a rasteriser");
  int bad = -1;
  const char *why = raster_images_check(mode, palette_chars, frames, n, h->max_frames, &bad);
  return why ? images_refused("raster_images_set", bad, why) : images_stage(h, mode, palette_chars, frames, n, 0, stream);
}

int asciichat_raster_images_set_composites(asciichat_raster_t *r, int mode, const char *palette_chars, const achip_frame_t *frames,
                                           int n, void *stream) {
  asciichat_raster_t *h = raster_of(r);
  if (!h)
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "raster_images_set_composites: not a rasteriser");
  int bad = -1, composites = 0;
  const char *why = raster_images_composites_check(mode, palette_chars, frames, n, h->max_frames, &bad, &composites);
  return why ? images_refused("raster_images_set_composites", bad, why)
             : images_stage(h, mode, palette_chars, frames, n, composites, stream);
}

int asciichat_raster_images_set_dithered(asciichat_raster_t *r, const char *palette_chars, const achip_frame_t *frames, int n, void *stream) {
  asciichat_raster_t *h = raster_of(r);
  if (!h)
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "raster_images_set_dithered: not a rasteriser");
  int bad = -1, composites = 0;
  const char *why = raster_images_dithered_check(palette_chars, frames, n, h->max_frames, &bad, &composites);
  return why ? images_refused("raster_images_set_dithered", bad, why)
             : images_stage(h, ACHIP_MODE_16_DITHER_BG, palette_chars, frames, n, composites, stream);
}

/* what cells_from_images asks of its arguments; nothing is launched unless it holds */
static int images_ok(const asciichat_raster_t *h, int n, const uint32_t *status_dev, const char *what) {
  if (!h)
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "%s: not a rasteriser", what);
  if (h->img_n < 1)
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "%s: no images are set (asciichat_raster_images_set)", what);
  if (n < 1 || n > h->img_n)
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "%s: %d frames of the %d that are set", what, n, h->img_n);
  if (!status_dev)
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "%s: a status array is required", what);
  return 0;
}

int asciichat_raster_cells_from_images(asciichat_raster_t *r, int n, uint32_t *status_dev, void *stream) {
  asciichat_raster_t *h = raster_of(r);
  const int rc = images_ok(h, n, status_dev, "raster_cells_from_images");
  if (rc)
    return rc;
  if (h->img.mode == ACHIP_MODE_16_DITHER_BG) /* the current set's kind: made by images_set_dithered */
    return hip_check((hipError_t)raster_launch_cells_dither(&h->p, &h->img, h->img_comp, n, h->cells, status_dev, stream), "raster dither launch");
  return hip_check((hipError_t)raster_launch_cells_images(&h->p, &h->img, h->img_comp, n, h->cells, status_dev, stream), "raster images launch");
}

int asciichat_raster_run_images(asciichat_raster_t *r, int n, uint8_t *pixels_dev, size_t image_pitch, uint32_t *status_dev,
                                void *stream) {
  asciichat_raster_t *h = raster_of(r);
  int rc = images_ok(h, n, status_dev, "raster_run_images");
  if (rc)
    return rc;
  /* nothing is launched unless both stages take their arguments */
  if (!pixels_dev || ((uintptr_t)pixels_dev & 3u) || (image_pitch & 3u) || image_pitch < asciichat_raster_image_pitch(h))
    return fail(ASCIICHAT_RASTER_ERR_INVALID_PARAM, "raster_run_images: 4-byte aligned pixels and an image pitch of at least %zu are required",
                asciichat_raster_image_pitch(h));
  rc = asciichat_raster_cells_from_images(r, n, status_dev, stream);
  return rc ? rc : asciichat_raster_draw(r, n, pixels_dev, image_pitch, stream);
}

int asciichat_raster_run_images_yuv420(asciichat_raster_t *r, int n, uint8_t *yuv_dev, size_t image_pitch, int layout,
                                       uint32_t *status_dev, void *stream) {
  asciichat_raster_t *h = raster_of(r);
  int rc = images_ok(h, n, status_dev, "raster_run_images_yuv420");
  if (!rc)
    rc = yuv_ok(h, n, yuv_dev, image_pitch, layout, "raster_run_images_yuv420");
  if (rc)
    return rc;
  rc = asciichat_raster_cells_from_images(r, n, status_dev, stream);
  return rc ? rc : asciichat_raster_draw_yuv420(r, n, yuv_dev, image_pitch, layout, stream);
}

void asciichat_raster_destroy(asciichat_raster_t *r) {
  asciichat_raster_t *h = raster_of(r);
  if (!h)
    return;
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(h->device);
  raster_free(h);
  (void)hipSetDevice(cur);
}
