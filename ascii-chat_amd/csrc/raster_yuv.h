/* raster_yuv.h -- the RGB -> YUV 4:2:0 arithmetic of the rasteriser's plane output (include/asciichat_raster.h), one text for
 * the kernel (raster_yuv_kernels.hpp), the emulator driver and host code: the reference's h265_encoder_ascii_to_yuv420
 * (lib/video/h265/encoder.c:247-289), pure integer.
 *
 * The reference clamps U and V to 0..255 (:282, :286).  Over all 2^24 inputs Y lies in 16..235 and U, V in 16..240, so the
 * clamp never fires and is not coded; tests/test_raster_yuv_emulated.py walks every input and pins the ranges.  Not installed. */
#ifndef ASCIICHAT_RASTER_YUV_PRIV_H
#define ASCIICHAT_RASTER_YUV_PRIV_H

#include <stdint.h>

#if defined(__HIPCC__)
#define RASTER_YUV_FN __host__ __device__ static inline
#else
#define RASTER_YUV_FN static inline
#endif

/* :264, per pixel */
RASTER_YUV_FN uint32_t raster_yuv_y(uint32_t r, uint32_t g, uint32_t b) { return ((66u * r + 129u * g + 25u * b + 128u) >> 8) + 16u; }
/* :276-278, one channel of a 2x2 block: the sum of its four pixels (0..1020), truncating */
RASTER_YUV_FN uint32_t raster_yuv_avg(uint32_t sum4) { return sum4 / 4u; }
/* :281 and :285, over the block's averages; the shift of a negative sum is arithmetic, as the reference's is */
RASTER_YUV_FN uint32_t raster_yuv_u(uint32_t r, uint32_t g, uint32_t b) {
  return (uint32_t)(((-38 * (int32_t)r - 74 * (int32_t)g + 112 * (int32_t)b + 128) >> 8) + 128);
}
RASTER_YUV_FN uint32_t raster_yuv_v(uint32_t r, uint32_t g, uint32_t b) {
  return (uint32_t)(((112 * (int32_t)r - 94 * (int32_t)g - 18 * (int32_t)b + 128) >> 8) + 128);
}

#endif
