/* rain.h -- the digital rain pass: the per-frame descriptor shared by the host C (rain.c) and the kernel (rain_kernels.hpp),
 * and the launcher between them (rain.hip).  Not installed. */
#ifndef ACHIP_RAIN_H
#define ACHIP_RAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* one frame of a rain batch: the context's device state and its parameters as they stood at issue time */
typedef struct {
  float *state;       /* num_columns * num_rows previous brightness values (row-major), and the backup half at [backup] */
  const float *cols;  /* num_columns x {time_offset, speed_multiplier} */
  float t;            /* time after this call's advance */
  float fall_speed, raindrop_length, decay;
  uint32_t color;     /* r | g << 8 | b << 16 | first_frame << 24 */
  int32_t num_columns, num_rows;
  uint32_t backup;    /* cells of the grid as allocated: a grid written smaller keeps its backup behind all of them;
                         0, or anything less than the grid as written: directly behind the grid as written */
} achip_rain_desc_t;

#define ACHIP_RAIN_BLOCK 256       /* threads per workgroup: one workgroup per frame */
#define ACHIP_RAIN_SEG 16          /* input bytes per thread and chunk */
#define ACHIP_RAIN_TABLE_MAX 12288 /* brightness table entries in LDS (48 KB): 200 x 61 fits, larger grids compute on demand */

/* frames i < n: desc_dev[i] (device-readable), input at src + i * src_stride (src_len_dev[i] bytes, up to the first NUL),
 * output at dst + i * dst_stride with its length in dst_len_dev[i] (ACHIP_LEN_OVERFLOW when it does not fit with its NUL) */
int achip_launch_rain(const achip_rain_desc_t *desc_dev, int n, int table_entries, const uint8_t *src, uint64_t src_stride,
                      const uint32_t *src_len_dev, uint8_t *dst, uint64_t dst_stride, uint32_t *dst_len_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif
