/*
 * nodevice_hip.c -- TEST INFRASTRUCTURE, never part of the product.
 *
 * The four HIP runtime entry points buffer_pool.c calls, answering as the runtime does on a host without a GPU: no pinned
 * memory, so every block comes from the host fallback.  Linked instead of libamdhip64 into the sanitizer builds of
 * tests/cabi/buffer_pool_test_port.c, so that those runs exercise the host blocks only, and the same ones, whether or not the
 * machine has a GPU.
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <stddef.h>

hipError_t hipHostMalloc(void **ptr, size_t size, unsigned int flags) {
  (void)size;
  (void)flags;
  if (ptr)
    *ptr = NULL;
  return hipErrorNoDevice;
}

hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned int flags) {
  (void)host;
  (void)flags;
  if (dev)
    *dev = NULL;
  return hipErrorNoDevice;
}

hipError_t hipHostFree(void *ptr) { return ptr ? hipErrorInvalidValue : hipSuccess; }

hipError_t hipGetLastError(void) { return hipSuccess; }
