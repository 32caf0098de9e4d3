/* ops_probe.hip -- the device build of the machine-ops probe: ops_probe_kernels.hpp against the product's gfx950_ops.hpp, one
 * extern "C" entry per family (ascii-chat_amd/Makefile: libachip_opsprobe.so).  Every entry queues its launches on `stream` and
 * returns the HIP error code of the last one (0 = queued), or -1 for a grid beyond PROBE_MAX_GRID.  TESTS ONLY. */
#include "ops_probe_kernels.hpp"

using namespace opsprobe;

#define PROBE_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

__global__ __launch_bounds__(PROBE_BLOCK) void k_lane_arith(const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t n, uint32_t *out) {
  lane_arith_kernel(a, b, c, n, out);
}
__global__ __launch_bounds__(PROBE_BLOCK) void k_lane_const(const uint32_t *a, const uint32_t *b, uint32_t n, uint32_t *out) {
  lane_const_kernel(a, b, n, out);
}
__global__ __launch_bounds__(PROBE_BLOCK) void k_wave(const uint32_t *val, const uint32_t *idx, const uint32_t *sel, const uint32_t *wdist, const uint32_t *widx,
                                                      const uint32_t *wfirst, const uint32_t *wval, const uint32_t *wmask, uint32_t *out) {
  wave_kernel(val, idx, sel, wdist, widx, wfirst, wval, wmask, out);
}
template <int OFF, bool HI>
__global__ __launch_bounds__(PROBE_BLOCK) void k_lds_byte(const uint32_t *pat, const uint32_t *phase, const uint32_t *v, uint32_t *out) {
  lds_byte_kernel<OFF, HI>(pat, phase, v, out);
}
__global__ __launch_bounds__(PROBE_BLOCK) void k_lds_or(const uint32_t *init, const uint32_t *at, const uint32_t *plain, const uint32_t *off0,
                                                        const uint32_t *off4, const uint32_t *off8, uint32_t *out) {
  lds_or_kernel(init, at, plain, off0, off4, off8, out);
}
__global__ __launch_bounds__(PROBE_BLOCK) void k_gmem_store(uint8_t *buf, const uint32_t *vals) { gmem_store_kernel(buf, vals); }
__global__ __launch_bounds__(PROBE_BLOCK) void k_gmem_load(const uint8_t *src, uint32_t *out) { gmem_load_kernel(src, out); }
__global__ __launch_bounds__(PROBE_BLOCK) void k_atomics(const uint32_t *wg_in, const uint32_t *xv, uint32_t *old, uint32_t *wg_out,
                                                         unsigned long long *counter, unsigned long long inc, unsigned long long *old64,
                                                         const unsigned long long *wg64, unsigned long long *slot64, unsigned long long *back64) {
  atomics_kernel(wg_in, xv, old, wg_out, counter, inc, old64, wg64, slot64, back64);
}
__global__ __launch_bounds__(PROBE_BLOCK) void k_arrival(const uint32_t *word, uint32_t *data, uint32_t *arrivals, uint32_t *res) {
  arrival_kernel(word, data, arrivals, res);
}

inline bool grid_ok(int grid) { return grid >= 1 && grid <= PROBE_MAX_GRID; }

template <int OFF, bool HI>
void lds_byte_launch(int grid, const uint32_t *pat, const uint32_t *phase, const uint32_t *v, uint32_t *out, hipStream_t s) {
  hipLaunchKernelGGL((k_lds_byte<OFF, HI>), dim3(grid), dim3(PROBE_BLOCK), LDS_BYTES, s, pat, phase, v, out);
}

} // namespace

/* the compile-time (offset, width) pairs and shifts of the folded kernel, for the tests' own table to be held against:
 * table[0 .. 2 * CONST_BFE) then [.. + CONST_ALIGN), then kConstV, kConstLo; returns the number of words */
PROBE_EXPORT int opsprobe_const_table(uint32_t *table) {
  int k = 0;
  for (int i = 0; i < CONST_BFE; i++) {
    table[k++] = kConstBfe[i][0];
    table[k++] = kConstBfe[i][1];
  }
  for (int i = 0; i < CONST_ALIGN; i++)
    table[k++] = kConstAlign[i];
  table[k++] = kConstV;
  table[k++] = kConstLo;
  return k;
}

PROBE_EXPORT int opsprobe_lane_arith(int grid, const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t n, uint32_t *out, void *stream) {
  if (!grid_ok(grid))
    return -1;
  hipLaunchKernelGGL(k_lane_arith, dim3(grid), dim3(PROBE_BLOCK), 0, (hipStream_t)stream, a, b, c, n, out);
  return (int)hipGetLastError();
}

PROBE_EXPORT int opsprobe_lane_const(int grid, const uint32_t *a, const uint32_t *b, uint32_t n, uint32_t *out, void *stream) {
  if (!grid_ok(grid))
    return -1;
  hipLaunchKernelGGL(k_lane_const, dim3(grid), dim3(PROBE_BLOCK), 0, (hipStream_t)stream, a, b, n, out);
  return (int)hipGetLastError();
}

PROBE_EXPORT int opsprobe_wave(int grid, const uint32_t *val, const uint32_t *idx, const uint32_t *sel, const uint32_t *wdist, const uint32_t *widx,
                               const uint32_t *wfirst, const uint32_t *wval, const uint32_t *wmask, uint32_t *out, void *stream) {
  if (!grid_ok(grid))
    return -1;
  hipLaunchKernelGGL(k_wave, dim3(grid), dim3(PROBE_BLOCK), 0, (hipStream_t)stream, val, idx, sel, wdist, widx, wfirst, wval, wmask, out);
  return (int)hipGetLastError();
}

/* ten launches: (OFF, HI) = (0, 1, 2, 3, 7) x (false, true) in that order, launch j writing out + j * 4 * grid * 256 words */
PROBE_EXPORT int opsprobe_lds_bytes(int grid, const uint32_t *pat, const uint32_t *phase, const uint32_t *v, uint32_t *out, void *stream) {
  if (!grid_ok(grid))
    return -1;
  hipStream_t s = (hipStream_t)stream;
  const size_t per = (size_t)4 * (size_t)grid * PROBE_BLOCK;
  lds_byte_launch<0, false>(grid, pat, phase, v, out + 0 * per, s);
  lds_byte_launch<0, true>(grid, pat, phase, v, out + 1 * per, s);
  lds_byte_launch<1, false>(grid, pat, phase, v, out + 2 * per, s);
  lds_byte_launch<1, true>(grid, pat, phase, v, out + 3 * per, s);
  lds_byte_launch<2, false>(grid, pat, phase, v, out + 4 * per, s);
  lds_byte_launch<2, true>(grid, pat, phase, v, out + 5 * per, s);
  lds_byte_launch<3, false>(grid, pat, phase, v, out + 6 * per, s);
  lds_byte_launch<3, true>(grid, pat, phase, v, out + 7 * per, s);
  lds_byte_launch<7, false>(grid, pat, phase, v, out + 8 * per, s);
  lds_byte_launch<7, true>(grid, pat, phase, v, out + 9 * per, s);
  return (int)hipGetLastError();
}

PROBE_EXPORT int opsprobe_lds_or(int grid, const uint32_t *init, const uint32_t *at, const uint32_t *plain, const uint32_t *off0,
                                 const uint32_t *off4, const uint32_t *off8, uint32_t *out, void *stream) {
  if (!grid_ok(grid))
    return -1;
  hipLaunchKernelGGL(k_lds_or, dim3(grid), dim3(PROBE_BLOCK), PROBE_BLOCK * 4, (hipStream_t)stream, init, at, plain, off0, off4, off8, out);
  return (int)hipGetLastError();
}

PROBE_EXPORT int opsprobe_gmem(uint8_t *store_buf, const uint32_t *vals, const uint8_t *load_src, uint32_t *load_out, void *stream) {
  hipLaunchKernelGGL(k_gmem_store, dim3(1), dim3(PROBE_BLOCK), 0, (hipStream_t)stream, store_buf, vals);
  hipLaunchKernelGGL(k_gmem_load, dim3(1), dim3(PROBE_BLOCK), 0, (hipStream_t)stream, load_src, load_out);
  return (int)hipGetLastError();
}

PROBE_EXPORT int opsprobe_atomics(int grid, const uint32_t *wg_in, const uint32_t *xv, uint32_t *old, uint32_t *wg_out,
                                  unsigned long long *counter, unsigned long long inc, unsigned long long *old64,
                                  const unsigned long long *wg64, unsigned long long *slot64, unsigned long long *back64, void *stream) {
  if (!grid_ok(grid))
    return -1;
  hipLaunchKernelGGL(k_atomics, dim3(grid), dim3(PROBE_BLOCK), 8, (hipStream_t)stream, wg_in, xv, old, wg_out, counter, inc, old64, wg64,
                     slot64, back64);
  return (int)hipGetLastError();
}

/* always PROBE_MAX_GRID = 64 workgroups: the collector reads a word per lane */
PROBE_EXPORT int opsprobe_arrival(const uint32_t *word, uint32_t *data, uint32_t *arrivals, uint32_t *res, void *stream) {
  hipLaunchKernelGGL(k_arrival, dim3(PROBE_MAX_GRID), dim3(PROBE_BLOCK), 0, (hipStream_t)stream, word, data, arrivals, res);
  return (int)hipGetLastError();
}
