/*
 * rain.c -- the digital rain effect (lib/video/anim/digital_rain.c): the reference's context with its exact layout, its
 * eight entry points, and the batch form asciichat_hip_rain_apply_batch; the pass itself is rain_kernels.hpp.
 *
 * A context is the public digital_rain_t followed by a private tail (magic-tagged) that holds the device copy of the
 * per-column constants and of the previous-brightness grid.  The device state is created at a context's first apply, from
 * the host arrays as they stand then.  Every apply reads the public parameters afresh (callers write them directly), and
 * advances time, the rainbow colour and first_frame on the host when it is ISSUED.  The drop-in apply waits for its frame
 * and copies the grid back into previous_brightness; the batch form leaves the grid on the device.
 *
 * Per-frame descriptors travel in a ring of mapped pinned segments: a segment is reused only after the launch that read it
 * has finished (its event), so a batch call never waits on the GPU unless 16 earlier calls are all still in flight.
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <math.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "achip_host.h"
#include "asciichat_hip.h"
#include "asciichat_render.h"
#include "internal.h"
#include "rain.h"

#define RAIN_MAGIC 0x52414e4449474954ull
#define RAIN_RING_SEGS 16
#define RAIN_SEG_FRAMES 1024

typedef struct {
  digital_rain_t pub; /* first: a digital_rain_t * is a rain_ctx_t * */
  uint64_t magic;
  int cols, rows;     /* as allocated */
  int device;         /* -1 until the device state exists */
  float *state_dev;   /* cols * rows previous brightness, then as many of backup */
  float *cols_dev;    /* cols x {time_offset, speed_multiplier} */
  int seg;            /* ring segment of the last launch that read this context, -1 for none */
  uint64_t seg_gen;
  hipStream_t stream; /* the drop-in's own */
  uint8_t *io_dev;    /* drop-in: [length, padded to 16][input][output] */
  size_t io_cap;
} rain_ctx_t;

static rain_ctx_t *ctx_of(digital_rain_t *rain) {
  rain_ctx_t *c = (rain_ctx_t *)rain;
  return c && c->magic == RAIN_MAGIC ? c : NULL;
}

/* ---- descriptor ring ---- */
static struct {
  pthread_mutex_t lock;
  achip_rain_desc_t *host, *dev;
  hipEvent_t ev[RAIN_RING_SEGS];
  uint64_t gen[RAIN_RING_SEGS]; /* launches recorded on the segment's event */
  int next;
  int ready;
} g_ring = {PTHREAD_MUTEX_INITIALIZER, NULL, NULL, {0}, {0}, 0, 0};

static int ring_init_locked(void) {
  if (g_ring.ready)
    return 0;
  void *h = NULL, *d = NULL;
  int rc = achip_hip_check((int)hipHostMalloc(&h, sizeof(achip_rain_desc_t) * RAIN_RING_SEGS * RAIN_SEG_FRAMES,
                                              hipHostMallocMapped | hipHostMallocPortable),
                           "hipHostMalloc(rain descriptors)");
  if (!rc)
    rc = achip_hip_check((int)hipHostGetDevicePointer(&d, h, 0), "hipHostGetDevicePointer(rain descriptors)");
  for (int s = 0; !rc && s < RAIN_RING_SEGS; s++)
    rc = achip_hip_check((int)hipEventCreateWithFlags(&g_ring.ev[s], hipEventDisableTiming), "hipEventCreate");
  if (rc)
    return rc;
  g_ring.host = (achip_rain_desc_t *)h;
  g_ring.dev = (achip_rain_desc_t *)d;
  g_ring.ready = 1;
  return 0;
}

/* waits until no launch that read context c can still be running */
static int ctx_wait(rain_ctx_t *c) {
  int rc = 0;
  pthread_mutex_lock(&g_ring.lock);
  if (c->seg >= 0 && g_ring.gen[c->seg] == c->seg_gen) /* (a newer generation means the segment was waited for) */
    rc = achip_hip_check((int)hipEventSynchronize(g_ring.ev[c->seg]), "hipEventSynchronize(rain)");
  c->seg = -1;
  pthread_mutex_unlock(&g_ring.lock);
  return rc;
}

/* ---- the reference's per-column constants (digital_rain.c:31-36, 120-125), on the host with its sinf ---- */
static float random_float(float x, float y) {
  float dt = x * 12.9898f + y * 78.233f;
  float sn = fmodf(dt, (float)M_PI);
  return fmodf(sinf(sn) * 43758.5453f, 1.0f);
}

digital_rain_t *digital_rain_init(int num_columns, int num_rows) {
  if (num_columns <= 0 || num_rows <= 0) {
    achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "digital_rain_init: invalid dimensions %dx%d", num_columns, num_rows);
    return NULL;
  }
  rain_ctx_t *c = (rain_ctx_t *)calloc(1, sizeof(rain_ctx_t));
  digital_rain_column_t *cols = (digital_rain_column_t *)calloc((size_t)num_columns, sizeof(digital_rain_column_t));
  float *prev = (float *)calloc((size_t)num_columns * (size_t)num_rows, sizeof(float));
  if (!c || !cols || !prev) {
    free(c);
    free(cols);
    free(prev);
    achip_fail(ASCIICHAT_HIP_ERR_MEMORY, "digital_rain_init: out of memory");
    return NULL;
  }
  for (int k = 0; k < num_columns; k++) {
    cols[k].time_offset = random_float((float)k, 0.0f) * 1000.0f;
    cols[k].speed_multiplier = random_float((float)k + 0.1f, 0.0f) * 0.5f + 0.5f;
    cols[k].phase_offset = random_float((float)k + 0.2f, 0.0f) * (float)M_PI * 2.0f;
  }
  digital_rain_t *r = &c->pub;
  r->columns = cols;
  r->num_columns = num_columns;
  r->num_rows = num_rows;
  r->fall_speed = 3.0f;
  r->raindrop_length = 12.0f;
  r->brightness_decay = 0.1f;
  r->animation_speed = 1.0f;
  r->color_r = 0;
  r->color_g = 255;
  r->color_b = 80;
  r->cursor_brightness = 2.0f;
  r->rainbow_mode = false;
  r->first_frame = true;
  r->time = 0.0f;
  r->previous_brightness = prev;
  c->magic = RAIN_MAGIC;
  c->cols = num_columns;
  c->rows = num_rows;
  c->device = -1;
  c->seg = -1;
  return r;
}

void digital_rain_destroy(digital_rain_t *rain) {
  rain_ctx_t *c = ctx_of(rain);
  if (!c)
    return;
  (void)ctx_wait(c);
  if (c->device >= 0) {
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(c->device);
    if (c->stream)
      (void)hipStreamSynchronize(c->stream);
    (void)hipFree(c->state_dev);
    (void)hipFree(c->cols_dev);
    (void)hipFree(c->io_dev);
    if (c->stream)
      (void)hipStreamDestroy(c->stream);
    (void)hipSetDevice(cur);
  }
  c->magic = 0;
  free(c->pub.columns);
  free(c->pub.previous_brightness);
  free(c);
}

void digital_rain_reset(digital_rain_t *rain) {
  rain_ctx_t *c = ctx_of(rain);
  if (!c)
    return;
  rain->time = 0.0f;
  rain->first_frame = true;
  memset(rain->previous_brightness, 0, (size_t)c->cols * (size_t)c->rows * sizeof(float));
  if (c->device >= 0 && !ctx_wait(c))
    (void)achip_hip_check((int)hipMemset(c->state_dev, 0, (size_t)c->cols * (size_t)c->rows * sizeof(float)), "hipMemset(rain state)");
}

void digital_rain_set_fall_speed(digital_rain_t *rain, float speed) {
  if (rain)
    rain->fall_speed = speed;
}

void digital_rain_set_raindrop_length(digital_rain_t *rain, float length) {
  if (rain)
    rain->raindrop_length = length;
}

void digital_rain_set_color(digital_rain_t *rain, uint8_t r, uint8_t g, uint8_t b) {
  if (rain) {
    rain->color_r = r;
    rain->color_g = g;
    rain->color_b = b;
  }
}

void digital_rain_set_color_from_filter(digital_rain_t *rain, color_filter_t filter) {
  if (!rain)
    return;
  if (filter == COLOR_FILTER_NONE) {
    rain->rainbow_mode = false;
    digital_rain_set_color(rain, 0, 255, 80);
    return;
  }
  if (filter == COLOR_FILTER_RAINBOW) {
    rain->rainbow_mode = true;
    digital_rain_set_color(rain, 255, 0, 0);
    return;
  }
  rain->rainbow_mode = false;
  achip_frame_t f;
  memset(&f, 0, sizeof(f));
  if (achip_frame_set_display_ops(&f, false, false, (int)filter) == 0) { /* the filter's tint (color_filter.c:24-150) */
    const uint32_t tint = f.ops >> ACHIP_OP_TINT_SHIFT;
    digital_rain_set_color(rain, (uint8_t)tint, (uint8_t)(tint >> 8), (uint8_t)(tint >> 16));
  }
}

/* the device state, created on the current device from the host arrays */
static int ctx_device(rain_ctx_t *c) {
  int dev = 0;
  int rc = achip_require_device();
  if (!rc)
    rc = achip_hip_check((int)hipGetDevice(&dev), "hipGetDevice");
  if (rc)
    return rc;
  if (c->device >= 0)
    return c->device == dev ? 0 : achip_fail(ASCIICHAT_HIP_ERR_INVALID_STATE, "rain: context lives on device %d, not %d", c->device, dev);
  const size_t cells = (size_t)c->cols * (size_t)c->rows;
  float *cols = (float *)malloc((size_t)c->cols * 2 * sizeof(float));
  if (!cols)
    return achip_fail(ASCIICHAT_HIP_ERR_MEMORY, "rain: out of memory");
  for (int k = 0; k < c->cols; k++) {
    cols[2 * k] = c->pub.columns[k].time_offset;
    cols[2 * k + 1] = c->pub.columns[k].speed_multiplier;
  }
  rc = achip_hip_check((int)hipMalloc((void **)&c->state_dev, 2 * cells * sizeof(float)), "hipMalloc(rain state)");
  if (!rc)
    rc = achip_hip_check((int)hipMalloc((void **)&c->cols_dev, (size_t)c->cols * 2 * sizeof(float)), "hipMalloc(rain columns)");
  if (!rc)
    rc = achip_hip_check((int)hipMemcpy(c->cols_dev, cols, (size_t)c->cols * 2 * sizeof(float), hipMemcpyHostToDevice),
                         "hipMemcpy(rain columns)");
  if (!rc)
    rc = achip_hip_check((int)hipMemcpy(c->state_dev, c->pub.previous_brightness, cells * sizeof(float), hipMemcpyHostToDevice),
                         "hipMemcpy(rain state)");
  free(cols);
  if (rc) {
    (void)hipFree(c->state_dev);
    (void)hipFree(c->cols_dev);
    c->state_dev = NULL;
    c->cols_dev = NULL;
    return rc;
  }
  c->device = dev;
  return 0;
}

size_t asciichat_hip_rain_out_stride(size_t src_stride, size_t max_chars_per_frame) {
  return (src_stride + 19u * max_chars_per_frame + 1u + 127u) & ~(size_t)127u;
}

float *asciichat_hip_rain_state_dev(digital_rain_t *rain) {
  rain_ctx_t *c = ctx_of(rain);
  if (!c) {
    achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "rain_state_dev: not a digital rain context");
    return NULL;
  }
  return ctx_device(c) ? NULL : c->state_dev;
}

int asciichat_hip_rain_apply_batch(digital_rain_t *const *rains, const float *dt, int n, const uint8_t *src_dev, size_t src_stride,
                                   const uint32_t *src_len_dev, uint8_t *dst_dev, size_t dst_stride, uint32_t *dst_len_dev,
                                   void *stream) {
  if (!rains || !dt || n <= 0 || !src_dev || !src_len_dev || !dst_dev || !dst_len_dev || dst_stride == 0)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "rain_apply_batch: bad arguments");
  for (int i = 0; i < n; i++) {
    rain_ctx_t *c = ctx_of(rains[i]);
    if (!c)
      return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "rain_apply_batch: frame %d has no digital rain context", i);
    if (c->pub.num_columns <= 0 || c->pub.num_rows <= 0 || c->pub.num_columns > c->cols || c->pub.num_rows > c->rows)
      return achip_fail(ASCIICHAT_HIP_ERR_INVALID_STATE, "rain_apply_batch: frame %d: grid %dx%d outside the context's %dx%d", i,
                        c->pub.num_columns, c->pub.num_rows, c->cols, c->rows);
    for (int j = 0; j < i; j++)
      if (rains[j] == rains[i])
        return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "rain_apply_batch: context of frame %d appears again at frame %d", j, i);
  }
  for (int i = 0; i < n; i++) {
    const int rc = ctx_device((rain_ctx_t *)rains[i]);
    if (rc)
      return rc;
  }
  pthread_mutex_lock(&g_ring.lock);
  int rc = ring_init_locked();
  /* a context's frames follow its earlier launches, whichever stream those went to (no host wait) */
  uint32_t waited = 0;
  for (int i = 0; !rc && i < n; i++) {
    const rain_ctx_t *c = (const rain_ctx_t *)rains[i];
    if (c->seg >= 0 && g_ring.gen[c->seg] == c->seg_gen && !(waited & (1u << c->seg))) {
      waited |= 1u << c->seg;
      rc = achip_hip_check((int)hipStreamWaitEvent((hipStream_t)stream, g_ring.ev[c->seg], 0), "hipStreamWaitEvent(rain)");
    }
  }
  for (int first = 0; !rc && first < n; first += RAIN_SEG_FRAMES) {
    const int m = n - first < RAIN_SEG_FRAMES ? n - first : RAIN_SEG_FRAMES;
    const int s = g_ring.next;
    if (g_ring.gen[s] != 0) /* the launch that read this segment last must be done before it is rewritten */
      rc = achip_hip_check((int)hipEventSynchronize(g_ring.ev[s]), "hipEventSynchronize(rain ring)");
    if (rc)
      break;
    achip_rain_desc_t *d = g_ring.host + (size_t)s * RAIN_SEG_FRAMES;
    int table = 0;
    for (int i = 0; i < m; i++) {
      rain_ctx_t *c = (rain_ctx_t *)rains[first + i];
      digital_rain_t *r = &c->pub;
      r->time += dt[first + i] * r->animation_speed; /* digital_rain.c:375-381 */
      if (r->rainbow_mode)
        color_filter_calculate_rainbow(r->time, &r->color_r, &r->color_g, &r->color_b);
      d[i].state = c->state_dev;
      d[i].cols = c->cols_dev;
      d[i].t = r->time;
      d[i].fall_speed = r->fall_speed;
      d[i].raindrop_length = r->raindrop_length;
      d[i].decay = r->brightness_decay;
      d[i].color = (uint32_t)r->color_r | ((uint32_t)r->color_g << 8) | ((uint32_t)r->color_b << 16) |
                   ((uint32_t)(r->first_frame ? 1 : 0) << 24);
      d[i].num_columns = r->num_columns;
      d[i].num_rows = r->num_rows;
      d[i].backup = (uint32_t)((size_t)c->cols * (size_t)c->rows);
      r->first_frame = false;
      const long entries = (long)r->num_columns * (long)(r->num_rows + 1);
      if (entries <= ACHIP_RAIN_TABLE_MAX && entries > table)
        table = (int)entries;
    }
    rc = achip_hip_check(achip_launch_rain(g_ring.dev + (size_t)s * RAIN_SEG_FRAMES, m, table, src_dev + (size_t)first * src_stride,
                                           (uint64_t)src_stride, src_len_dev + first, dst_dev + (size_t)first * dst_stride,
                                           (uint64_t)dst_stride, dst_len_dev + first, stream),
                         "rain launch");
    if (!rc)
      rc = achip_hip_check((int)hipEventRecord(g_ring.ev[s], (hipStream_t)stream), "hipEventRecord(rain)");
    if (rc)
      break;
    g_ring.gen[s]++;
    for (int i = 0; i < m; i++) {
      rain_ctx_t *c = (rain_ctx_t *)rains[first + i];
      c->seg = s;
      c->seg_gen = g_ring.gen[s];
    }
    g_ring.next = (s + 1) % RAIN_RING_SEGS;
  }
  pthread_mutex_unlock(&g_ring.lock);
  return rc;
}

char *digital_rain_apply(digital_rain_t *rain, const char *frame, float delta_time) {
  rain_ctx_t *c = ctx_of(rain);
  if (!c || !frame) {
    achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "digital_rain_apply: NULL parameter");
    return NULL;
  }
  const size_t len = strlen(frame);
  if (len > 0x7FFFFFFu) {
    achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "digital_rain_apply: frame of %zu bytes", len);
    return NULL;
  }
  int rc = ctx_device(c);
  const size_t in_bytes = (len + 15u) & ~(size_t)15u, out_stride = (20u * len + 1u + 15u) & ~(size_t)15u; /* never overflows */
  const size_t need = 16u + in_bytes + out_stride;
  if (!rc && !c->stream)
    rc = achip_hip_check((int)hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), "hipStreamCreate(rain)");
  if (!rc && c->io_cap < need) {
    (void)hipFree(c->io_dev);
    c->io_dev = NULL;
    c->io_cap = 0;
    rc = achip_hip_check((int)hipMalloc((void **)&c->io_dev, need + need / 4), "hipMalloc(rain staging)");
    if (!rc)
      c->io_cap = need + need / 4;
  }
  if (rc)
    return NULL;
  uint32_t *len_dev = (uint32_t *)c->io_dev;
  uint8_t *in_dev = c->io_dev + 16, *out_dev = c->io_dev + 16 + in_bytes;
  const uint32_t len32 = (uint32_t)len;
  uint32_t out_len = 0;
  const size_t cells = (size_t)c->cols * (size_t)c->rows;
  rc = achip_hip_check((int)hipMemcpyAsync(len_dev, &len32, 4, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync(rain length)");
  if (!rc && len)
    rc = achip_hip_check((int)hipMemcpyAsync(in_dev, frame, len, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync(rain frame)");
  if (!rc)
    rc = asciichat_hip_rain_apply_batch(&rain, &delta_time, 1, in_dev, in_bytes ? in_bytes : 16u, len_dev, out_dev, out_stride,
                                        len_dev + 1, c->stream);
  if (!rc)
    rc = achip_hip_check((int)hipMemcpyAsync(&out_len, len_dev + 1, 4, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync(rain length)");
  if (!rc)
    rc = achip_hip_check((int)hipMemcpyAsync(rain->previous_brightness, c->state_dev, cells * sizeof(float), hipMemcpyDeviceToHost,
                                             c->stream),
                         "hipMemcpyAsync(rain state)");
  if (!rc)
    rc = achip_hip_check((int)hipStreamSynchronize(c->stream), "hipStreamSynchronize(rain)");
  if (rc)
    return NULL;
  if (out_len > out_stride) {
    achip_fail(ASCIICHAT_HIP_ERR_BUFFER, "digital_rain_apply: output length %u", out_len);
    return NULL;
  }
  char *s = (char *)malloc((size_t)out_len + 1u);
  if (!s) {
    achip_fail(ASCIICHAT_HIP_ERR_MEMORY, "digital_rain_apply: out of memory");
    return NULL;
  }
  if (out_len)
    rc = achip_hip_check((int)hipMemcpy(s, out_dev, out_len, hipMemcpyDeviceToHost), "hipMemcpy(rain output)");
  if (rc) {
    free(s);
    return NULL;
  }
  s[out_len] = '\0';
  return s;
}
