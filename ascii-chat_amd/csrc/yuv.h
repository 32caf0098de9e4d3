/* yuv.h -- what the host side of libasciichat_yuv.so (yuv.c) and its launchers (yuv.hip, kernels in yuv_kernels.hpp) share.
 * Not installed. */
#ifndef ASCIICHAT_YUV_PRIV_H
#define ASCIICHAT_YUV_PRIV_H

#include "yuv_math.h"

#ifdef __cplusplus
extern "C" {
#endif

#define YUV_WHOLE_LANES_X 64 /* a workgroup of the whole conversion: 64 x 4 lanes, one block of pixels each */
#define YUV_WHOLE_LANES_Y (YUV_BLOCK / YUV_WHOLE_LANES_X)

/* a whole conversion, by value in the kernel arguments */
typedef struct {
  const asciichat_yuv_source_t *sources; /* device, resolved, one per image; NULL: `one` is the only source */
  asciichat_yuv_source_t one;            /* resolved */
  uint8_t *rgb;                          /* image i at rgb + i * pitch */
  uint64_t pitch;
  int32_t rgb_stride; /* bytes per image row; 0: tight, 3 * width of each source */
  int32_t _pad;
} yuv_whole_args_t;

/* the launchers (yuv.hip); each returns a hipError_t.  Arguments are the host's to check: nothing is checked again there but
 * what keeps a grid legal.
 * sample: image i of n from sources[i] under frames[i]; max_pixels: the largest out_w * out_h among them */
int yuv_launch_sample(const asciichat_yuv_source_t *sources, const achip_frame_t *frames, int n, uint32_t max_pixels, uint8_t *images,
                      uint64_t pitch, void *stream);
/* whole: n images; max_w, max_h: the largest width and height among the sources; formats: bit f set when some source has format
 * f -- one launch per format present, whose workgroups leave the images of the others alone */
int yuv_launch_whole(const yuv_whole_args_t *a, int n, int max_w, int max_h, unsigned formats, void *stream);

#ifdef __cplusplus
}
#endif
#endif
