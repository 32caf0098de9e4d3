/*
 * ops_probe_kernels.hpp -- one small kernel per family of <gfx950_ops.hpp>, each op called directly on inputs a test chooses
 * and its result written out untouched.  Plain HIP plus <gfx950_ops.hpp>, no conditional compilation: hipcc compiles this text
 * against the product header (tests/opsprobe/ops_probe.hip -> libachip_opsprobe.so), g++ against the emulator's twin
 * (tests/hipemu/ops_probe_emu_driver.cpp), and tests/ops_ref.py says what either must give.  TESTS ONLY.
 *
 * Every kernel runs in workgroups of PROBE_BLOCK = 256 threads (four waves), at most PROBE_MAX_GRID of them.  Every wave
 * operation is called by all 64 lanes of every wave, outside divergent control flow.  No thread waits for another workgroup.
 */
#pragma once

#include <gfx950_ops.hpp>
#include <stdint.h>

namespace opsprobe {

using namespace achip;

constexpr int PROBE_BLOCK = 256;
constexpr int PROBE_MAX_GRID = 64;

/* ---- lane arithmetic: out[op * n + i] = op(a[i], b[i], c[i]) -------------------------------------------------------------- */
enum { AR_ALIGNBIT = 0, AR_DOT4, AR_BFE, AR_MAD_I24, AR_MUL_U24, AR_BITREVERSE, AR_OPAQUE, AR_OPS };

__device__ inline void lane_arith_kernel(const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t n, uint32_t *out) {
  for (uint32_t i = blockIdx.x * (uint32_t)PROBE_BLOCK + threadIdx.x; i < n; i += gridDim.x * (uint32_t)PROBE_BLOCK) {
    const uint32_t x = a[i], y = b[i], z = c[i];
    out[AR_ALIGNBIT * n + i] = alignbit(x, y, z);
    out[AR_DOT4 * n + i] = dot4_u8(x, y, z);
    out[AR_BFE * n + i] = bfe_u32(x, y, z);
    out[AR_MAD_I24 * n + i] = (uint32_t)mad_i24((int32_t)x, (int32_t)y, (int32_t)z);
    out[AR_MUL_U24 * n + i] = mul_u24(x, y);
    out[AR_BITREVERSE * n + i] = bitreverse32(x);
    out[AR_OPAQUE * n + i] = opaque(x);
  }
}

/* the same two instructions with the offset, width and shift as compile-time constants (what the compiler folds them to), on a
 * value from memory and on a constant value */
constexpr int CONST_BFE = 16, CONST_ALIGN = 10;
constexpr uint32_t kConstBfe[CONST_BFE][2] = {{0, 0},  {0, 32}, {0, 24}, {0, 31},  {0, 1},   {8, 8},   {24, 8},  {24, 24},
                                              {31, 1}, {31, 31}, {31, 32}, {32, 8}, {16, 0}, {0, 33}, {40, 63}, {255, 255}};
constexpr uint32_t kConstAlign[CONST_ALIGN] = {0, 1, 8, 24, 31, 32, 33, 40, 63, 255};
constexpr uint32_t kConstV = 0x89ABCDEFu, kConstLo = 0x01234567u;
constexpr int CONST_OUTS = 2 * (CONST_BFE + CONST_ALIGN);

template <int K> __device__ inline void const_bfe_one(uint32_t v, uint32_t n, uint32_t i, uint32_t *out) {
  constexpr uint32_t off = kConstBfe[K][0], width = kConstBfe[K][1];
  out[(uint32_t)K * n + i] = bfe_u32(v, off, width);
  out[(uint32_t)(CONST_BFE + CONST_ALIGN + K) * n + i] = bfe_u32(kConstV, off, width);
  if constexpr (K + 1 < CONST_BFE)
    const_bfe_one<K + 1>(v, n, i, out);
}
template <int K> __device__ inline void const_align_one(uint32_t hi, uint32_t lo, uint32_t n, uint32_t i, uint32_t *out) {
  constexpr uint32_t sh = kConstAlign[K];
  out[(uint32_t)(CONST_BFE + K) * n + i] = alignbit(hi, lo, sh);
  out[(uint32_t)(2 * CONST_BFE + CONST_ALIGN + K) * n + i] = alignbit(kConstV, kConstLo, sh);
  if constexpr (K + 1 < CONST_ALIGN)
    const_align_one<K + 1>(hi, lo, n, i, out);
}
__device__ inline void lane_const_kernel(const uint32_t *a, const uint32_t *b, uint32_t n, uint32_t *out) {
  for (uint32_t i = blockIdx.x * (uint32_t)PROBE_BLOCK + threadIdx.x; i < n; i += gridDim.x * (uint32_t)PROBE_BLOCK) {
    const_bfe_one<0>(a[i], n, i, out);
    const_align_one<0>(a[i], b[i], n, i, out);
  }
}

/* ---- wave operations: thread g = blockIdx.x * 256 + threadIdx.x, wave w = g / 64; out[op * n + g], n = gridDim.x * 256 -------
 * per thread: val[g], idx[g] (a lane, 0..63), sel[g] (the SAME word in every lane of a wave: a lane select that the compiler
 * sees in a vector register, computed per lane, as the zseq state walk and the rasteriser's parser have it); per wave: wdist[w]
 * (0..63), widx[w] (0..63), wfirst[w], wval[w], wmask[2w..] */
enum {
  WV_BALLOT_LO = 0, WV_BALLOT_HI, WV_LANE_BIT_BALLOT, WV_LANE_BIT_MEM, WV_SHFL, WV_SHFL_UP, WV_SHFL_UP_1, WV_READ_0, WV_READ_1,
  WV_READ_63, WV_READ_UNIFORM, WV_READ_VGPR, WV_UNIFORM, WV_SCAN, WV_XOR_LAST, WV_SHIFT_UP1, WV_OPS
};

__device__ inline void wave_kernel(const uint32_t *val, const uint32_t *idx, const uint32_t *sel, const uint32_t *wdist, const uint32_t *widx,
                                   const uint32_t *wfirst, const uint32_t *wval, const uint32_t *wmask, uint32_t *out) {
  const uint32_t g = blockIdx.x * (uint32_t)PROBE_BLOCK + threadIdx.x, w = g >> 6, n = gridDim.x * (uint32_t)PROBE_BLOCK;
  const uint32_t v = val[g];
  const uint64_t bal = wave_ballot((v & 1u) != 0u);
  out[WV_BALLOT_LO * n + g] = (uint32_t)bal;
  out[WV_BALLOT_HI * n + g] = (uint32_t)(bal >> 32);
  out[WV_LANE_BIT_BALLOT * n + g] = lane_bit(wave_ballot((v & 2u) != 0u) >> 1) ? 1u : 0u;
  out[WV_LANE_BIT_MEM * n + g] = lane_bit((uint64_t)wmask[2u * w] | ((uint64_t)wmask[2u * w + 1u] << 32)) ? 1u : 0u;
  out[WV_SHFL * n + g] = wave_shfl(v, (int)idx[g]);
  out[WV_SHFL_UP * n + g] = wave_shfl_up(v, (int)wdist[w]);
  out[WV_SHFL_UP_1 * n + g] = wave_shfl_up(v, 1);
  out[WV_READ_0 * n + g] = wave_read_lane(v, 0);
  out[WV_READ_1 * n + g] = wave_read_lane(v, 1);
  out[WV_READ_63 * n + g] = wave_read_lane(v, 63);
  out[WV_READ_UNIFORM * n + g] = wave_read_lane(v, (int)widx[w]);
  out[WV_READ_VGPR * n + g] = wave_read_lane(v, (int)(sel[g] >> 4) + (int)(sel[g] & 15u));
  out[WV_UNIFORM * n + g] = (uint32_t)wave_uniform((int)wval[w]);
  out[WV_SCAN * n + g] = wave_inclusive_scan(v);
  out[WV_XOR_LAST * n + g] = wave_xor_to_last(v); /* (valid in lane 63) */
  out[WV_SHIFT_UP1 * n + g] = wave_shift_up1(v, wfirst[w]);
}

/* ---- LDS ------------------------------------------------------------------------------------------------------------------
 * byte stores: every lane owns the 16 bytes at lds_base_addr() + 16 * tid, fills them with pat[4g..4g+3], stores ONE byte of
 * v[g] at phase[g] + OFF (phase + OFF <= 15) and reads the slot back behind the fence and a barrier: out[4g..4g+3] */
constexpr uint32_t LDS_SLOT = 16;
constexpr uint32_t LDS_BYTES = PROBE_BLOCK * LDS_SLOT;

template <int OFF, bool HI>
__device__ inline void lds_byte_kernel(const uint32_t *pat, const uint32_t *phase, const uint32_t *v, uint32_t *out) {
  const uint32_t tid = threadIdx.x, g = blockIdx.x * (uint32_t)PROBE_BLOCK + tid;
  uint32_t *slot = reinterpret_cast<uint32_t *>(ACHIP_SMEM + LDS_SLOT * tid);
  for (int j = 0; j < 4; j++)
    slot[j] = pat[4u * g + (uint32_t)j];
  __syncthreads();
  ds_store_byte<OFF, HI>(lds_base_addr() + LDS_SLOT * tid + phase[g], v[g]);
  lds_store_fence();
  __syncthreads();
  for (int j = 0; j < 4; j++)
    out[4u * g + (uint32_t)j] = slot[j];
}

/* ORs: the workgroup's LDS holds 256 words, word t = init[256 * blockIdx.x + t].  Thread g ORs plain[g] into word at[2g] with
 * ds_or_u32, and off0/off4/off8[g] into the words at byte 16 * at[2g + 1] + 0 / 4 / 8 with ds_or_u32_at (at[2g + 1] < 64). */
__device__ inline void lds_or_kernel(const uint32_t *init, const uint32_t *at, const uint32_t *plain, const uint32_t *off0,
                                     const uint32_t *off4, const uint32_t *off8, uint32_t *out) {
  const uint32_t tid = threadIdx.x, g = blockIdx.x * (uint32_t)PROBE_BLOCK + tid;
  uint32_t *words = reinterpret_cast<uint32_t *>(ACHIP_SMEM);
  words[tid] = init[g];
  __syncthreads();
  const uint32_t base = lds_base_addr();
  ds_or_u32(base + 4u * at[2u * g], plain[g]);
  const uint32_t grp = base + 16u * at[2u * g + 1u];
  ds_or_u32_at<0>(grp, off0[g]);
  ds_or_u32_at<4>(grp, off4[g]);
  ds_or_u32_at<8>(grp, off8[g]);
  lds_store_fence();
  __syncthreads();
  out[g] = words[tid];
}

/* ---- global memory ----------------------------------------------------------------------------------------------------------
 * stores: thread t < GM_OFFSETS of region k writes at byte offset t of its own 256-byte slot, buf + (k * GM_OFFSETS + t) * 256:
 * region 0 two bytes, 1 four, 2 eight, 3 sixteen (unaligned), 4 sixteen non-temporal (threads with t % 16 == 0 only) */
constexpr uint32_t GM_OFFSETS = 144, GM_SLOT = 256, GM_REGIONS = 5;

__device__ inline void gmem_store_kernel(uint8_t *buf, const uint32_t *vals) {
  const uint32_t t = threadIdx.x;
  if (blockIdx.x != 0u || t >= GM_OFFSETS)
    return;
  const uint32_t a = vals[4u * t], b = vals[4u * t + 1u], c = vals[4u * t + 2u], d = vals[4u * t + 3u];
  store_u16_unaligned(buf + (0u * GM_OFFSETS + t) * GM_SLOT + t, (uint16_t)a);
  store_u1_unaligned(buf + (1u * GM_OFFSETS + t) * GM_SLOT + t, a);
  store_u2_unaligned(buf + (2u * GM_OFFSETS + t) * GM_SLOT + t, a, b);
  store_u4_unaligned(buf + (3u * GM_OFFSETS + t) * GM_SLOT + t, make_uint4(a, b, c, d));
  if (t % 16u == 0u)
    store_u4_nt(buf + (4u * GM_OFFSETS + t) * GM_SLOT + t, make_uint4(a, b, c, d));
}
/* loads: out[t] = the four bytes at src + t, t < GM_OFFSETS (the caller owns src[0 .. GM_OFFSETS + 3]) */
__device__ inline void gmem_load_kernel(const uint8_t *src, uint32_t *out) {
  const uint32_t t = threadIdx.x;
  if (blockIdx.x != 0u || t >= GM_OFFSETS)
    return;
  out[t] = load_u32_unaligned_nt(src + t);
}

/* ---- scoped atomics ---------------------------------------------------------------------------------------------------------
 * workgroup scope, two LDS words: every thread adds wg_in[4b + 1] to a word that starts at wg_in[4b] and xors xv[g] into one
 * that starts at wg_in[4b + 2]; old[g] = what its add returned, wg_out[2b], [2b + 1] = the words afterwards.
 * agent scope: every thread of the launch adds inc to *counter (old64[g] = what it got); thread 0 of workgroup b stores
 * wg64[b] into slot64[b] and loads it back into back64[b]. */
__device__ inline void atomics_kernel(const uint32_t *wg_in, const uint32_t *xv, uint32_t *old, uint32_t *wg_out,
                                      unsigned long long *counter, unsigned long long inc, unsigned long long *old64,
                                      const unsigned long long *wg64, unsigned long long *slot64, unsigned long long *back64) {
  const uint32_t tid = threadIdx.x, b = blockIdx.x, g = b * (uint32_t)PROBE_BLOCK + tid;
  uint32_t *words = reinterpret_cast<uint32_t *>(ACHIP_SMEM);
  if (tid == 0u) {
    wg_store_u32(&words[0], wg_in[4u * b]);
    wg_store_u32(&words[1], wg_in[4u * b + 2u]);
  }
  __syncthreads();
  old[g] = wg_fetch_add_u32(&words[0], wg_in[4u * b + 1u]);
  wg_xor_u32(&words[1], xv[g]);
  old64[g] = agent_fetch_add_u64(counter, inc);
  __syncthreads();
  if (tid == 0u) {
    wg_out[2u * b] = wg_load_u32(&words[0]);
    wg_out[2u * b + 1u] = wg_load_u32(&words[1]);
    agent_store_u64(&slot64[b], wg64[b]);
    back64[b] = agent_load_u64(&slot64[b]);
  }
}

/* the arrival hand-off of the span checksum: lane 0 of every workgroup's wave 0 publishes word[b] into data[b] and arrives at
 * *arrivals; the ONE workgroup that is handed gridDim.x - 1 (gridDim.x == 64: a word per lane) reads all the words and writes
 * res[0] = their sum, res[1] = its own index and bumps res[2], the number of collectors.  Nobody waits for anybody. */
__device__ inline void arrival_kernel(const uint32_t *word, uint32_t *data, uint32_t *arrivals, uint32_t *res) {
  const uint32_t tid = threadIdx.x, b = blockIdx.x;
  if (tid >= 64u)
    return;
  uint32_t arrived = 0u;
  if (tid == 0u) {
    agent_store_u32(&data[b], word[b]);
    arrived = agent_arrive_u32(arrivals);
  }
  arrived = wave_read_lane(arrived, 0);
  if (arrived != gridDim.x - 1u)
    return;
  const uint32_t sum = wave_read_lane(wave_inclusive_scan(agent_load_u32(&data[tid])), 63);
  if (tid == 0u) {
    res[0] = sum;
    res[1] = b;
    (void)agent_arrive_u32(&res[2]);
  }
}

} // namespace opsprobe
