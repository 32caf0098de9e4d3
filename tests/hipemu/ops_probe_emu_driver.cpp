/* ops_probe_emu_driver.cpp -- the machine-ops probe (tests/opsprobe/ops_probe_kernels.hpp) under the fiber emulator, against the
 * emulator's twin of gfx950_ops.hpp: the entries of tests/opsprobe/ops_probe.hip by name and signature, every launch with the
 * grid, block and LDS size the device launcher gives it.  `stream` is ignored.  TESTS ONLY. */
#include "../opsprobe/ops_probe_kernels.hpp"

using namespace opsprobe;

static inline bool grid_ok(int grid) { return grid >= 1 && grid <= PROBE_MAX_GRID; }

extern "C" int opsprobe_const_table(uint32_t *table) {
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

extern "C" int opsprobe_lane_arith(int grid, const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t n, uint32_t *out, void *) {
  if (!grid_ok(grid))
    return -1;
  hipemu::launch(dim3((unsigned)grid), dim3(PROBE_BLOCK), 0, [&] { lane_arith_kernel(a, b, c, n, out); });
  return 0;
}

extern "C" int opsprobe_lane_const(int grid, const uint32_t *a, const uint32_t *b, uint32_t n, uint32_t *out, void *) {
  if (!grid_ok(grid))
    return -1;
  hipemu::launch(dim3((unsigned)grid), dim3(PROBE_BLOCK), 0, [&] { lane_const_kernel(a, b, n, out); });
  return 0;
}

extern "C" int opsprobe_wave(int grid, const uint32_t *val, const uint32_t *idx, const uint32_t *sel, const uint32_t *wdist, const uint32_t *widx,
                             const uint32_t *wfirst, const uint32_t *wval, const uint32_t *wmask, uint32_t *out, void *) {
  if (!grid_ok(grid))
    return -1;
  hipemu::launch(dim3((unsigned)grid), dim3(PROBE_BLOCK), 0, [&] { wave_kernel(val, idx, sel, wdist, widx, wfirst, wval, wmask, out); });
  return 0;
}

template <int OFF, bool HI> static void lds_byte_launch(int grid, const uint32_t *pat, const uint32_t *phase, const uint32_t *v, uint32_t *out) {
  hipemu::launch(dim3((unsigned)grid), dim3(PROBE_BLOCK), LDS_BYTES, [&] { lds_byte_kernel<OFF, HI>(pat, phase, v, out); });
}

extern "C" int opsprobe_lds_bytes(int grid, const uint32_t *pat, const uint32_t *phase, const uint32_t *v, uint32_t *out, void *) {
  if (!grid_ok(grid))
    return -1;
  const size_t per = (size_t)4 * (size_t)grid * PROBE_BLOCK;
  lds_byte_launch<0, false>(grid, pat, phase, v, out + 0 * per);
  lds_byte_launch<0, true>(grid, pat, phase, v, out + 1 * per);
  lds_byte_launch<1, false>(grid, pat, phase, v, out + 2 * per);
  lds_byte_launch<1, true>(grid, pat, phase, v, out + 3 * per);
  lds_byte_launch<2, false>(grid, pat, phase, v, out + 4 * per);
  lds_byte_launch<2, true>(grid, pat, phase, v, out + 5 * per);
  lds_byte_launch<3, false>(grid, pat, phase, v, out + 6 * per);
  lds_byte_launch<3, true>(grid, pat, phase, v, out + 7 * per);
  lds_byte_launch<7, false>(grid, pat, phase, v, out + 8 * per);
  lds_byte_launch<7, true>(grid, pat, phase, v, out + 9 * per);
  return 0;
}

extern "C" int opsprobe_lds_or(int grid, const uint32_t *init, const uint32_t *at, const uint32_t *plain, const uint32_t *off0,
                               const uint32_t *off4, const uint32_t *off8, uint32_t *out, void *) {
  if (!grid_ok(grid))
    return -1;
  hipemu::launch(dim3((unsigned)grid), dim3(PROBE_BLOCK), PROBE_BLOCK * 4, [&] { lds_or_kernel(init, at, plain, off0, off4, off8, out); });
  return 0;
}

extern "C" int opsprobe_gmem(uint8_t *store_buf, const uint32_t *vals, const uint8_t *load_src, uint32_t *load_out, void *) {
  hipemu::launch(dim3(1), dim3(PROBE_BLOCK), 0, [&] { gmem_store_kernel(store_buf, vals); });
  hipemu::launch(dim3(1), dim3(PROBE_BLOCK), 0, [&] { gmem_load_kernel(load_src, load_out); });
  return 0;
}

extern "C" int opsprobe_atomics(int grid, const uint32_t *wg_in, const uint32_t *xv, uint32_t *old, uint32_t *wg_out, unsigned long long *counter,
                                unsigned long long inc, unsigned long long *old64, const unsigned long long *wg64, unsigned long long *slot64,
                                unsigned long long *back64, void *) {
  if (!grid_ok(grid))
    return -1;
  hipemu::launch(dim3((unsigned)grid), dim3(PROBE_BLOCK), 8,
                 [&] { atomics_kernel(wg_in, xv, old, wg_out, counter, inc, old64, wg64, slot64, back64); });
  return 0;
}

extern "C" int opsprobe_arrival(const uint32_t *word, uint32_t *data, uint32_t *arrivals, uint32_t *res, void *) {
  hipemu::launch(dim3(PROBE_MAX_GRID), dim3(PROBE_BLOCK), 0, [&] { arrival_kernel(word, data, arrivals, res); });
  return 0;
}

/* EMULATOR ONLY: one wave operation with an argument outside its domain, which the twin must refuse by aborting the process.
 * which = 0: wave_read_lane of lane 64; 1: of a lane select that differs between the lanes; 2: wave_shfl_up by 64; 3: by -1.
 * Returns (0) only if nothing refused. */
extern "C" int opsprobe_emu_out_of_domain(int which) {
  hipemu::launch(dim3(1), dim3(PROBE_BLOCK), 0, [&] {
    const uint32_t v = threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    if (which == 0)
      (void)wave_read_lane(v, 64);
    else if (which == 1)
      (void)wave_read_lane(v, 63 - lane);
    else if (which == 2)
      (void)wave_shfl_up(v, 64);
    else
      (void)wave_shfl_up(v, -1);
  });
  return 0;
}
