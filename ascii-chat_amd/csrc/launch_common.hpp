/*
 * launch_common.hpp -- what every launcher between hip_launch.h's entry points and hipLaunchKernelGGL needs once
 * (hip_launch.hip, render_inst.hip, render_stream_inst.hip, render_rows_inst.hip).  Host code only.
 */
#ifndef ACHIP_LAUNCH_COMMON_HPP
#define ACHIP_LAUNCH_COMMON_HPP

#include <hip/hip_runtime.h>

#include <mutex>

#include "achip_types.h"

namespace achip {

/* The launch's uniform descriptor as the kernels take it by value: all zero unless the caller enabled it (composite
 * batches too: achip_frames_uniform), but the launch-wide facts of `flags` always travel -- also when the descriptors
 * come from the device array.  (The phase kernel never reads the flags.) */
inline achip_uniform_t launch_uniform(const achip_uniform_t *uniform) {
  achip_uniform_t uni = {};
  if (uniform && uniform->enabled)
    uni = *uniform;
  if (uniform)
    uni.flags = uniform->flags;
  return uni;
}

/* A kernel that may be launched with more than 48 KB of dynamic LDS says so to the runtime first, once per
 * instantiation (one flag per KERN; benign race: the call is idempotent). */
template <auto KERN> hipError_t ensure_dynamic_lds(int bytes) {
  static bool attr_set = false;
  if (!attr_set) {
    if (bytes > 48 * 1024) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
      if (e != hipSuccess)
        return e;
    }
    attr_set = true;
  }
  return hipSuccess;
}

/* A constant table the kernels read: BYTES of device memory filled by INIT (one 256-thread workgroup with INIT_LDS bytes of
 * dynamic LDS), one image per device of the process, built at the first call on that device and read-only from then on.
 * Building allocates, launches on the null stream and synchronises the device -- launches on every stream may read the
 * image afterwards --, none of which a stream capture allows: see achip_launch_warm_crc_tables. */
template <void (*INIT)(uint32_t *), size_t BYTES, size_t INIT_LDS> hipError_t device_table(const uint4 **out) {
  constexpr int MAX_DEVICES = 16;
  static std::mutex mu;
  static uint32_t *tab[MAX_DEVICES] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess)
    return e;
  if (dev < 0 || dev >= MAX_DEVICES)
    return hipErrorInvalidDevice;
  std::lock_guard<std::mutex> lock(mu);
  if (!tab[dev]) {
    uint32_t *t = nullptr;
    e = hipMalloc(reinterpret_cast<void **>(&t), BYTES);
    if (e != hipSuccess)
      return e;
    hipLaunchKernelGGL(INIT, dim3(1), dim3(256), INIT_LDS, nullptr, t);
    e = hipGetLastError();
    if (e == hipSuccess)
      e = hipDeviceSynchronize();
    if (e != hipSuccess) {
      (void)hipFree(t);
      return e;
    }
    tab[dev] = t;
  }
  *out = reinterpret_cast<const uint4 *>(tab[dev]);
  return hipSuccess;
}

} // namespace achip

/* The checksum kernels' prebuilt tables (crc_math.hpp: crc_frame_tables_init_kernel<block>, block = 1024 or 256; defined in
 * hip_launch.hip): ONE image per device and block for the whole library -- the stream kernel's PACK + wire launches read the
 * same one as the stand-alone pass --, which achip_launch_warm_crc_tables builds.  Returns a hipError_t. */
extern "C" int achipk_frame_crc_tables(int block, const uint4 **out);
#endif
