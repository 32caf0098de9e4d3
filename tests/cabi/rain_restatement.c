/*
 * rain_restatement.c -- the digital rain contract (digital_rain_apply and friends) restated sequentially from its
 * description, for the tests: one pass over the string, one token at a time.  The context has the public layout of
 * digital_rain_t (include/asciichat_render.h), so the tests poke the same fields on both.  The wobble's sine is binary32
 * sine taken as (float)sin((double)x); the per-column constants use the platform's sinf, as the contract says.
 * Built by the tests with gcc -O2 -ffp-contract=off (no fast-math, no -march), linked with csrc/achip_host.c.
 */
#include <math.h>
#include <stdbool.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
  float time_offset, speed_multiplier, phase_offset;
} rs_column_t;
typedef struct {
  rs_column_t *columns;
  int num_columns, num_rows;
  float time, fall_speed, raindrop_length, brightness_decay, animation_speed;
  uint8_t color_r, color_g, color_b;
  float cursor_brightness;
  bool rainbow_mode, first_frame;
  float *previous_brightness;
} rs_rain_t;

_Static_assert(sizeof(rs_rain_t) == 56, "layout");

static float rf(float x, float y) {
  float d = x * 12.9898f + y * 78.233f;
  float s = fmodf(d, (float)M_PI);
  return fmodf(sinf(s) * 43758.5453f, 1.0f);
}

rs_rain_t *rs_init(int cols, int rows) {
  if (cols <= 0 || rows <= 0)
    return NULL;
  rs_rain_t *r = calloc(1, sizeof(*r));
  r->columns = calloc((size_t)cols, sizeof(rs_column_t));
  r->previous_brightness = calloc((size_t)cols * (size_t)rows, sizeof(float));
  for (int c = 0; c < cols; c++) {
    r->columns[c].time_offset = rf((float)c, 0.0f) * 1000.0f;
    r->columns[c].speed_multiplier = rf((float)c + 0.1f, 0.0f) * 0.5f + 0.5f;
    r->columns[c].phase_offset = rf((float)c + 0.2f, 0.0f) * (float)M_PI * 2.0f;
  }
  r->num_columns = cols;
  r->num_rows = rows;
  r->fall_speed = 3.0f;
  r->raindrop_length = 12.0f;
  r->brightness_decay = 0.1f;
  r->animation_speed = 1.0f;
  r->color_g = 255;
  r->color_b = 80;
  r->cursor_brightness = 2.0f;
  r->first_frame = true;
  return r;
}

void rs_destroy(rs_rain_t *r) {
  if (!r)
    return;
  free(r->columns);
  free(r->previous_brightness);
  free(r);
}

void rs_reset(rs_rain_t *r) {
  r->time = 0.0f;
  r->first_frame = true;
  memset(r->previous_brightness, 0, (size_t)r->num_columns * (size_t)r->num_rows * sizeof(float));
}

/* color_filter_calculate_rainbow's HSV walk: the product's host helper (csrc/achip_host.c, linked in by the tests) */
void achip_rainbow_color(float time_seconds, uint8_t *r, uint8_t *g, uint8_t *b);

/* digital_rain_set_color_from_filter: default green, rainbow, or the filter's tint (color_filter.c's registry) */
void rs_set_color_from_filter(rs_rain_t *r, int filter) {
  static const uint8_t tint[12][3] = {{0, 0, 0},     {0, 0, 0},     {255, 255, 255}, {0, 255, 65},    {255, 0, 255},  {255, 0, 170},
                                      {255, 136, 0}, {0, 221, 221}, {0, 255, 255},   {255, 182, 193}, {255, 51, 51}, {255, 235, 153}};
  if (filter == 0 || filter == 12) {
    r->rainbow_mode = filter == 12;
    r->color_r = filter ? 255 : 0;
    r->color_g = filter ? 0 : 255;
    r->color_b = filter ? 0 : 80;
    return;
  }
  r->rainbow_mode = false;
  if (filter > 0 && filter < 12) {
    r->color_r = tint[filter][0];
    r->color_g = tint[filter][1];
    r->color_b = tint[filter][2];
  }
}

static float bright(const rs_rain_t *r, int col, int row, float t) {
  if (col >= r->num_columns)
    return 0.0f;
  float ct = r->columns[col].time_offset + t * r->fall_speed * r->columns[col].speed_multiplier;
  float x = (ct - (float)row) / r->raindrop_length;
  float w = x + 0.3f * (float)sin((double)(1.41421354f * x)) + 0.2f * (float)sin((double)(2.23606801f * x));
  return 1.0f - (w - floorf(w));
}

static int chan(int v, float b) {
  float f = (float)v * b;
  int x = (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : (int)0x80000000u; /* x86's conversion of the rest */
  return x < 0 ? 0 : x > 255 ? 255 : x;
}

static size_t put_sgr(char *o, bool fg, int r, int g, int b, float bright_v, bool cursor) {
  if (cursor)
    bright_v *= 2.0f;
  if (bright_v < 0.0f)
    bright_v = 0.0f;
  if (bright_v > 1.0f)
    bright_v = 1.0f;
  int v[3] = {chan(r, bright_v), chan(g, bright_v), chan(b, bright_v)};
  size_t n = 0;
  o[n++] = 27;
  o[n++] = '[';
  o[n++] = fg ? '3' : '4';
  o[n++] = '8';
  o[n++] = ';';
  o[n++] = '2';
  for (int q = 0; q < 3; q++) {
    o[n++] = ';';
    if (v[q] >= 100)
      o[n++] = (char)('0' + v[q] / 100);
    if (v[q] >= 10)
      o[n++] = (char)('0' + v[q] / 10 % 10);
    o[n++] = (char)('0' + v[q] % 10);
  }
  o[n++] = 'm';
  return n;
}

static int u8len(const uint8_t *s) {
  if (s[0] < 0x80)
    return 1;
  if ((s[0] & 0xE0) == 0xC0)
    return (s[1] & 0xC0) == 0x80 ? 2 : 1;
  if ((s[0] & 0xF0) == 0xE0)
    return (s[1] & 0xC0) == 0x80 && (s[2] & 0xC0) == 0x80 ? 3 : 1;
  if ((s[0] & 0xF8) == 0xF0)
    return (s[1] & 0xC0) == 0x80 && (s[2] & 0xC0) == 0x80 && (s[3] & 0xC0) == 0x80 ? 4 : 1;
  return 1;
}

/* ESC [ 3|4 8 ; 2 ; digits ; digits ; digits m at s: its length, or 0 */
static size_t color_event(const uint8_t *s, bool *fg, int *rgb) {
  if (!((s[2] == '3' || s[2] == '4') && s[3] == '8' && s[4] == ';' && s[5] == '2' && s[6] == ';'))
    return 0;
  *fg = s[2] == '3';
  size_t p = 7;
  for (int q = 0; q < 3; q++) {
    unsigned v = 0;
    while (s[p] >= '0' && s[p] <= '9')
      v = v * 10u + (unsigned)(s[p++] - '0');
    rgb[q] = (int)v;
    if (s[p++] != (q < 2 ? ';' : 'm'))
      return 0;
  }
  return p;
}

/* one event at (col, row): the brightness it shows (blended, state updated) and whether it is a cursor */
static float event(rs_rain_t *r, int col, int row, float t, bool *cursor) {
  float b = bright(r, col, row, t);
  *cursor = b > bright(r, col, row + 1, t);
  if (row < r->num_rows && col < r->num_columns) {
    float *p = &r->previous_brightness[(size_t)row * (size_t)r->num_columns + (size_t)col];
    if (!r->first_frame)
      b = *p + (b - *p) * r->brightness_decay;
    *p = b;
  }
  return b;
}

char *rs_apply(rs_rain_t *r, const char *frame, float dt, size_t *out_len) {
  r->time += dt * r->animation_speed;
  const float t = r->time;
  if (r->rainbow_mode)
    achip_rainbow_color(t, &r->color_r, &r->color_g, &r->color_b);
  const uint8_t *s = (const uint8_t *)frame;
  const size_t len = strlen(frame);
  char *out = malloc(len * 20 + 64), *o = out;
  int col = 0, row = 0;
  size_t i = 0;
  while (s[i]) {
    if (s[i] == 27) {
      bool fg, cursor;
      int rgb[3];
      size_t n = s[i + 1] == '[' ? color_event(s + i, &fg, rgb) : 0;
      if (n) {
        float b = event(r, col, row, t, &cursor);
        o += put_sgr(o, fg, rgb[0], rgb[1], rgb[2], b, cursor);
        i += n;
        continue;
      }
      size_t j = i + 1;
      if (s[j] == '[') {
        j++;
        while (s[j] && !(s[j] >= 0x40 && s[j] <= 0x7E))
          j++;
        if (s[j])
          j++;
      }
      memcpy(o, s + i, j - i);
      o += j - i;
      i = j;
      continue;
    }
    if (s[i] == '\n') {
      *o++ = '\n';
      i++;
      row++;
      col = 0;
      continue;
    }
    bool cursor;
    float b = event(r, col, row, t, &cursor);
    o += put_sgr(o, true, r->color_r, r->color_g, r->color_b, b, cursor);
    int n = u8len(s + i);
    memcpy(o, s + i, (size_t)n);
    o += n;
    i += (size_t)n;
    col++;
  }
  *o = 0;
  r->first_frame = false;
  if (out_len)
    *out_len = (size_t)(o - out);
  return out;
}
