/*
 * hip_emu.h -- a tiny single-threaded fiber emulator of the HIP execution model, for TESTS ONLY.
 *
 * Purpose: the render kernels (ascii-chat_amd/csrc/render_kernels.hpp) are plain HIP C++.  Compiled
 * with -DACHIP_HIPEMU under g++ they run here, one workgroup at a time, every work-item a ucontext
 * fiber, so that block barriers, wave64 ballots/shuffles and LDS indexing are exercised bit-exactly
 * against the oracle in the CPU test suite -- GPU minutes are scarce, logic bugs should die here.
 *
 * This is not a fallback and is never linked into the product library: libasciichat_hip.so contains
 * only hipcc-compiled gfx950 code and fails loudly without a GPU.
 *
 * SCHEDULES.  A workgroup runs in sweeps; the unit of scheduling is the WAVE: a wave picked in a sweep runs each of its
 * runnable lanes once, lanes ascending, up to the lane's next barrier / wave operation / exit, and wave barriers are
 * released after the sweep.  Which waves a sweep picks, and in which order, is the wave policy (hipemu_set_schedule):
 *   ASC            every runnable wave, 0 .. W-1: the default, and the only schedule this emulator had before
 *   DESC           every runnable wave, W-1 .. 0
 *   RANDOM(seed)   every runnable wave with probability 1/2 (one of them if none came up), in a fresh random permutation;
 *                  the generator is seeded from (seed, linear workgroup index) alone, so a failure replays from its seed
 *   LATE(w, k)     wave w % W is not picked in the first k sweeps of each workgroup: the late-arriving predecessor.
 *                  LATE(w, k, after=B) starts the k sweeps when the workgroup's B-th block barrier is released: a kernel
 *                  whose prologue ends in a barrier makes EVERY wave wait there for a wave that is late from the start, and
 *                  nobody in the hand-off behind it
 * and the order of the workgroups, which still run ONE AT A TIME TO COMPLETION, is ASC, DESC or SHUFFLE(seed) -- legal
 * only for launches whose workgroups never wait for one another.
 * Blind spots that remain: the order of the lanes INSIDE a wave never varies (on the machine a wave's lanes run in
 * lockstep, and the twin models lds_store_fence as a wave barrier), workgroups are never co-resident, and memory is
 * sequentially consistent (no store is ever seen late or out of order).
 */
#pragma once
#include <ucontext.h>

#include <algorithm>
#include <cassert>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(...)
#define __restrict__

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct uint4 {
  uint32_t x, y, z, w;
};
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
struct uint2 {
  uint32_t x, y;
};
static inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }

namespace hipemu {

struct idx3 {
  unsigned x, y, z;
};
inline idx3 g_threadIdx, g_blockIdx;
inline dim3 g_blockDim, g_gridDim;
inline std::vector<unsigned char> g_smem;
inline size_t g_smem_limit = 160 * 1024;

enum { RUN = 0, WAIT_BLOCK = 1, WAIT_WAVE = 2, DONE = 3 };
struct Fiber {
  ucontext_t ctx;
  void *stack = nullptr;
  int state = RUN;
};
inline std::vector<Fiber> g_fibers;
inline ucontext_t g_sched;
inline int g_cur = -1;
inline std::function<void()> g_body;
inline uint32_t g_wave_slots[64][64]; /* [wave][lane] exchange slots (block <= 4096 threads) */

/* ---- the schedule (see the head of this file) ------------------------------------------------------------------- */
enum { WAVES_ASC = 0, WAVES_DESC = 1, WAVES_RANDOM = 2, WAVES_LATE = 3 };
enum { WG_ASC = 0, WG_DESC = 1, WG_SHUFFLE = 2 };
struct Schedule {
  int waves = WAVES_ASC;
  uint64_t seed = 0;       /* RANDOM */
  int late_wave = 0;       /* LATE: the wave held back (modulo the block's waves) ... */
  uint64_t late_sweeps = 0; /* ... during this many sweeps of each workgroup ... */
  unsigned late_after = 0;  /* ... counted from the release of this many block barriers (0: from the workgroup's start) */
  int wg_order = WG_ASC;
  uint64_t wg_seed = 0; /* SHUFFLE */
};
inline Schedule g_schedule;
inline uint64_t g_naps = 0; /* calls of the twin's spin_nap: a lane found nothing and waits */
enum { PICK_LOG_CAP = 1 << 16 };
inline uint8_t g_pick_log[PICK_LOG_CAP]; /* the waves visited, in order, over every launch since the last reset */
inline uint64_t g_picks = 0;             /* ... and how many there were (the log keeps the first PICK_LOG_CAP) */

/* splitmix64: small, and good enough from consecutive seeds */
struct Rng {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  unsigned below(unsigned n) { return (unsigned)(next() % n); } /* n <= 4096: the bias is far below what matters here */
  template <class T> void shuffle(T *v, unsigned n) {
    for (unsigned i = n; i > 1; i--)
      std::swap(v[i - 1], v[below(i)]);
  }
};
inline Rng rng_for(uint64_t seed, uint64_t stream) {
  Rng r{seed * 0xD1342543DE82EF95ull + stream};
  r.next();
  return r;
}

inline void yield_as(int state) {
  g_fibers[g_cur].state = state;
  swapcontext(&g_fibers[g_cur].ctx, &g_sched);
}
inline void trampoline() {
  g_body();
  yield_as(DONE);
}
inline void block_barrier() { yield_as(WAIT_BLOCK); }
inline void wave_barrier() { yield_as(WAIT_WAVE); }

inline int lane() { return (int)(g_threadIdx.x & 63u); }
inline int wave() { return (int)(g_threadIdx.x >> 6); }

inline uint64_t ballot(int pred) {
  const int w = wave(), l = lane();
  g_wave_slots[w][l] = pred ? 1u : 0u;
  wave_barrier();
  uint64_t m = 0;
  const int nl = std::min<int>(64, (int)g_blockDim.x - w * 64);
  for (int i = 0; i < nl; i++)
    m |= (uint64_t)g_wave_slots[w][i] << i;
  wave_barrier();
  return m;
}
inline uint32_t shfl_from(uint32_t v, int src) {
  const int w = wave(), l = lane();
  g_wave_slots[w][l] = v;
  wave_barrier();
  uint32_t r = (src >= 0 && src < 64) ? g_wave_slots[w][src] : v;
  wave_barrier();
  return r;
}

template <class F> void launch(dim3 grid, dim3 block, size_t smem_bytes, F body) {
  if (smem_bytes > g_smem_limit) {
    fprintf(stderr, "hipemu: dynamic LDS request %zu exceeds %zu\n", smem_bytes, g_smem_limit);
    abort();
  }
  assert(block.y == 1 && block.z == 1 && block.x % 64 == 0 && block.x <= 4096);
  const size_t stack_bytes = 256 * 1024;
  const Schedule sch = g_schedule;
  g_blockDim = block;
  g_gridDim = grid;
  g_smem.assign(smem_bytes + 64, 0xCD); /* poison: kernels must initialise what they read */
  g_fibers.resize(block.x);
  for (auto &f : g_fibers)
    if (!f.stack)
      f.stack = malloc(stack_bytes);
  g_body = body;
  const unsigned nwg = grid.x * grid.y * grid.z, nwaves = block.x / 64;
  std::vector<unsigned> wg_at; /* the workgroup that runs at each position; empty = ascending */
  if (sch.wg_order != WG_ASC) {
    wg_at.resize(nwg);
    for (unsigned i = 0; i < nwg; i++)
      wg_at[i] = sch.wg_order == WG_DESC ? nwg - 1 - i : i;
    if (sch.wg_order == WG_SHUFFLE) {
      Rng r = rng_for(sch.wg_seed, 0x5746ull);
      r.shuffle(wg_at.data(), nwg);
    }
  }
  for (unsigned at = 0; at < nwg; at++) { /* workgroups one at a time, x fastest */
    const unsigned bb = wg_at.empty() ? at : wg_at[at];
    const unsigned b = bb % grid.x;
    g_blockIdx = idx3{b, (bb / grid.x) % grid.y, bb / (grid.x * grid.y)};
    std::fill(g_smem.begin(), g_smem.end(), 0xCD);
    for (unsigned t = 0; t < block.x; t++) {
      Fiber &f = g_fibers[t];
      getcontext(&f.ctx);
      f.ctx.uc_stack.ss_sp = f.stack;
      f.ctx.uc_stack.ss_size = stack_bytes;
      f.ctx.uc_link = nullptr;
      makecontext(&f.ctx, (void (*)())trampoline, 0);
      f.state = RUN;
    }
    Rng rng = rng_for(sch.seed, bb);
    const unsigned held = sch.waves == WAVES_LATE ? (unsigned)sch.late_wave % nwaves : ~0u;
    unsigned picked[64], barriers = 0;
    uint64_t hold_from = 0; /* the sweep at which the hold began, once `barriers` has reached late_after */
    for (uint64_t sweep = 0;; sweep++) {
      bool ran = false;
      const bool holding = barriers >= sch.late_after && sweep - hold_from < sch.late_sweeps;
      /* the waves of this sweep: those with a runnable lane, thinned and ordered by the policy */
      unsigned np = 0;
      for (unsigned w = 0; w < nwaves; w++) {
        bool runnable = false;
        for (unsigned t = w * 64; t < w * 64 + 64 && !runnable; t++)
          runnable = g_fibers[t].state == RUN;
        if (!runnable)
          continue;
        if (w == held && holding) {
          ran = true; /* waiting for the held wave is progress, not a deadlock: it runs after late_sweeps sweeps */
          continue;
        }
        picked[np++] = w;
      }
      if (sch.waves == WAVES_DESC) {
        std::reverse(picked, picked + np);
      } else if (sch.waves == WAVES_RANDOM && np) {
        unsigned nk = 0, keep[64];
        for (unsigned i = 0; i < np; i++)
          if (rng.next() >> 63)
            keep[nk++] = picked[i];
        if (!nk)
          keep[nk++] = picked[rng.below(np)];
        rng.shuffle(keep, nk);
        std::copy(keep, keep + nk, picked);
        np = nk;
      }
      for (unsigned i = 0; i < np; i++) {
        if (g_picks < PICK_LOG_CAP)
          g_pick_log[g_picks] = (uint8_t)picked[i];
        g_picks++;
        for (unsigned t = picked[i] * 64; t < picked[i] * 64 + 64; t++) {
          if (g_fibers[t].state != RUN)
            continue;
          g_cur = (int)t;
          g_threadIdx = idx3{t, 0, 0};
          swapcontext(&g_sched, &g_fibers[t].ctx);
          ran = true;
        }
      }
      /* release wave barriers */
      unsigned done = 0, at_block = 0;
      for (unsigned w0 = 0; w0 < block.x; w0 += 64) {
        unsigned nwait = 0, ndone = 0, n = std::min(64u, block.x - w0);
        for (unsigned t = w0; t < w0 + n; t++) {
          nwait += g_fibers[t].state == WAIT_WAVE;
          ndone += g_fibers[t].state == DONE;
        }
        if (nwait && nwait + ndone == n) {
          if (ndone) {
            fprintf(stderr, "hipemu: wave op with exited lanes (wave %u)\n", w0 / 64);
            abort();
          }
          for (unsigned t = w0; t < w0 + n; t++)
            g_fibers[t].state = RUN;
          ran = true;
        }
      }
      for (unsigned t = 0; t < block.x; t++) {
        done += g_fibers[t].state == DONE;
        at_block += g_fibers[t].state == WAIT_BLOCK;
      }
      if (done == block.x)
        break;
      if (at_block && at_block + done == block.x) {
        if (done) {
          fprintf(stderr, "hipemu: __syncthreads with exited threads\n");
          abort();
        }
        for (auto &f : g_fibers)
          f.state = RUN;
        ran = true;
        if (++barriers == sch.late_after)
          hold_from = sweep + 1;
      }
      if (!ran) {
        fprintf(stderr, "hipemu: deadlock (divergent barrier?) block %u\n", b);
        abort();
      }
    }
  }
}

} // namespace hipemu

/* ---- what every driver library exports of the schedule (tests/emu_schedule.py) ----------------------------------- */
/* the schedule of every later launch; also clears the nap counter and the pick log.  All zeros = the default */
extern "C" __attribute__((used, visibility("default"))) inline void hipemu_set_schedule(int waves, uint64_t seed, int late_wave,
                                                                                       uint64_t late_sweeps, int late_after,
                                                                                       int wg_order, uint64_t wg_seed) {
  hipemu::g_schedule.waves = waves;
  hipemu::g_schedule.seed = seed;
  hipemu::g_schedule.late_wave = late_wave < 0 ? 0 : late_wave;
  hipemu::g_schedule.late_sweeps = late_sweeps;
  hipemu::g_schedule.late_after = late_after < 0 ? 0u : (unsigned)late_after;
  hipemu::g_schedule.wg_order = wg_order;
  hipemu::g_schedule.wg_seed = wg_seed;
  hipemu::g_naps = 0;
  hipemu::g_picks = 0;
}
/* spin_nap calls since the last reset */
extern "C" __attribute__((used, visibility("default"))) inline uint64_t hipemu_naps(int reset) {
  const uint64_t n = hipemu::g_naps;
  if (reset)
    hipemu::g_naps = 0;
  return n;
}
/* the waves visited since the last reset: copies the first min(cap, PICK_LOG_CAP, picks) into out, returns the picks */
extern "C" __attribute__((used, visibility("default"))) inline uint64_t hipemu_pick_log(uint8_t *out, uint64_t cap, int reset) {
  const uint64_t n = hipemu::g_picks, have = std::min<uint64_t>(n, hipemu::PICK_LOG_CAP);
  if (out)
    memcpy(out, hipemu::g_pick_log, (size_t)std::min(cap, have));
  if (reset)
    hipemu::g_picks = 0;
  return n;
}

#define threadIdx hipemu::g_threadIdx
#define blockIdx hipemu::g_blockIdx
#define blockDim hipemu::g_blockDim
#define gridDim hipemu::g_gridDim

static inline void __syncthreads() { hipemu::block_barrier(); }
static inline uint32_t __umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
static inline uint32_t __umul24(uint32_t a, uint32_t b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); } /* low 32 bits */
static inline int __popcll(uint64_t v) { return __builtin_popcountll(v); }
static inline int __ffsll(unsigned long long v) { return __builtin_ffsll((long long)v); }
static inline int __clzll(long long v) { return v ? __builtin_clzll(v) : 64; }
static inline int __ffs(int v) { return __builtin_ffs(v); }
static inline int __clz(int v) { return v ? __builtin_clz((unsigned)v) : 32; }
using std::max;
using std::min;
static inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { /* fibers run one at a time */
  const uint32_t old = *p;
  *p = old + v;
  return old;
}
