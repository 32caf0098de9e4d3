/* achip_desc.h -- the three pure-C rules both libraries apply to a caller's palette and frame descriptors: the glyph tables of
 * a palette and the two descriptor checks.  libasciichat_hip.so exports them as achip_lut_build, achip_frame_extent_ok and
 * achip_frame_ratios_ok (achip_host.c); libasciichat_raster.so, which links nothing of that library, uses them as they stand
 * here (raster_images.h).  One text, two users.  Not installed. */
#ifndef ACHIP_DESC_H
#define ACHIP_DESC_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "achip_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* UTF-8 sequence length from the lead byte -- the palette parser's rule (common.c:397-410) */
static inline int achip_desc_utf8_seq_len(unsigned char c) {
  if ((c & 0xE0) == 0xC0)
    return 2;
  if ((c & 0xF0) == 0xE0)
    return 3;
  if ((c & 0xF8) == 0xF0)
    return 4;
  return 1;
}

static inline int achip_desc_lut_build(const char *palette_chars, achip_lut_t *lut) {
  if (!palette_chars || !lut || palette_chars[0] == '\0')
    return -1;
  memset(lut, 0, sizeof(*lut));
  uint32_t packed[256];
  int count = 0;
  size_t len = strlen(palette_chars), pos = 0;
  while (pos < len && count < 255) {
    int n = achip_desc_utf8_seq_len((unsigned char)palette_chars[pos]);
    uint32_t g = 0;
    for (int k = 0; k < n && pos + (size_t)k < len; k++)
      g |= (uint32_t)(unsigned char)palette_chars[pos + (size_t)k] << (8 * k);
    packed[count++] = g;
    pos += (size_t)n;
  }
  for (int i = 0; i < 256; i++) {
    int ci = count > 1 ? (i * (count - 1) + 127) / 255 : 0;
    if (ci >= count)
      ci = count - 1;
    lut->glyph[i] = packed[ci];
  }
  for (int i = 0; i < 64; i++) {
    int ci = count > 1 ? (i * (count - 1) + 31) / 63 : 0;
    if (ci >= count)
      ci = count - 1;
    lut->ramp[i] = (uint8_t)ci;
    lut->glyph64[i] = packed[ci];
  }
  for (int i = 0; i < 256; i++) /* the kernels take a one-byte-per-glyph fast path when nothing is multi-byte */
    if ((lut->glyph[i] & 0xFFu) >= 128u || (lut->glyph64[i & 63] & 0xFFu) >= 128u)
      lut->flags |= ACHIP_LUT_MULTIBYTE;
  return 0;
}

/* The kernels address a source with 32-bit byte offsets (a frame is at most tens of MB): a descriptor whose last pixel
 * lies 4 GiB or more behind its first -- only possible with an absurd explicit row stride -- is refused on the host. */
static inline bool achip_desc_extent_ok(const achip_frame_t *f) {
  if (!f || f->comp)
    return true; /* composites carry their own (tile-sized) sources */
  const uint64_t stride = f->src_stride > 0 ? (uint64_t)f->src_stride : 3ull * (uint64_t)(f->src_w > 0 ? f->src_w : 0);
  if (f->src_stride < 0)
    return false;
  const uint64_t extent = (uint64_t)(f->src_h > 0 ? f->src_h - 1 : 0) * stride + 3ull * (uint64_t)(f->src_w > 0 ? f->src_w : 0);
  return extent < 0xFFFFFFF0ull && stride < (1ull << 24);
}

/* The kernels compute a sample's column as (x * x_ratio) >> 16 in 32 bits (the reference's own arithmetic, image.c:315):
 * a descriptor whose last column or row would wrap that product is refused on the host, so that every kernel form samples
 * exactly what the rule in achip_types.h says.  Descriptors of sources of at most 10 000 pixels never come near it. */
static inline bool achip_desc_ratios_ok(const achip_frame_t *f) {
  if (!f || f->out_w <= 0 || f->out_h <= 0)
    return false;
  return (uint64_t)(f->out_w - 1) * f->x_ratio < (1ull << 32) && (uint64_t)(f->out_h - 1) * f->y_ratio < (1ull << 32);
}

#ifdef __cplusplus
}
#endif
#endif
