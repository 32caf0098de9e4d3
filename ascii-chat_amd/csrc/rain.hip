/* rain.hip -- the launcher of the digital rain pass (rain_kernels.hpp); the host side is rain.c. */
#include <hip/hip_runtime.h>

#include "rain.h"
#include "rain_kernels.hpp"

extern "C" int achip_launch_rain(const achip_rain_desc_t *desc_dev, int n, int table_entries, const uint8_t *src, uint64_t src_stride,
                                 const uint32_t *src_len_dev, uint8_t *dst, uint64_t dst_stride, uint32_t *dst_len_dev, void *stream) {
  if (n <= 0)
    return (int)hipSuccess;
  if (table_entries < 0 || table_entries > ACHIP_RAIN_TABLE_MAX)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(achip::rain::rain_kernel, dim3((unsigned)n), dim3(ACHIP_RAIN_BLOCK), achip::rain::lds_bytes(table_entries),
                     static_cast<hipStream_t>(stream), desc_dev, table_entries, src, src_stride, src_len_dev, dst, dst_stride,
                     dst_len_dev);
  return (int)hipGetLastError();
}
