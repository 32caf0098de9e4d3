/*
 * sched_probe_emu_driver.cpp -- tiny kernels that probe hip_emu.h's SCHEDULES (tests/test_emu_schedules.py).  TESTS ONLY, and
 * emulator only: some of them are wrong on purpose (a read with no barrier in front of it, a divergent barrier), to show that a
 * schedule tells, so none of this is ever compiled for the device.
 */
#include <gfx950_ops.hpp>

using namespace achip;

namespace {

constexpr uint32_t MAGIC = 0x600DF00Du;

/* lane 0 of wave 0 writes an LDS word, every thread reads it: with the barrier between this is legal code, without it the
 * readers of the other waves see the word only if wave 0 happened to run first */
void word_for_all(uint32_t *out, bool barrier) {
  uint32_t *w = reinterpret_cast<uint32_t *>(ACHIP_SMEM);
  if (threadIdx.x == 0)
    wg_store_u32(w, MAGIC + blockIdx.x);
  if (barrier)
    __syncthreads();
  out[blockIdx.x * blockDim.x + threadIdx.x] = wg_load_u32(w);
}

/* a flag hand-off through a polling loop with a wave operation in it (the shape of render_rows.hpp's rows_seg_wait): the
 * waiting wave takes one word from the wave below it and one from the wave above it; a producer publishes after `work` wave
 * operations of its own.  The words are zeroed by the host: a barrier in front of the loop would make every wave wait for a late
 * one there, and nobody in the loop.  Every wave but the producers and the waiter only exits.  The polls are bounded as the kernels' are. */
void flag_handoff(uint32_t *out, uint32_t *flags, int waiter, int work) { /* flags: [0] from below, [1] from above, zeroed */
  const int w = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
  if (w == waiter - 1 || w == waiter + 1) {
    uint32_t v = 0;
    for (int i = 0; i < work; i++)
      v += (uint32_t)__popcll(wave_ballot(((lane + i) & 1) != 0));
    if (lane == 0)
      wg_store_u32(&flags[w < waiter ? 0 : 1], 1000u * (uint32_t)(w + 1) + v);
  } else if (w == waiter) {
    uint32_t got[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
    for (int k = 0; k < 2; k++)
      for (int spin = 0; spin < (1 << 21); spin++) {
        const uint32_t v = wg_load_u32(&flags[k]);
        if (wave_ballot(v != 0u) == ~0ull) {
          got[k] = v;
          break;
        }
        spin_nap<1>();
      }
    out[2 * lane] = got[0];
    out[2 * lane + 1] = got[1];
  }
}

/* every workgroup appends its linear index to a list */
void append_index(uint32_t *list) {
  if (threadIdx.x == 0) {
    const uint32_t at = agent_arrive_u32(&list[0]);
    list[1 + at] = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  }
}

/* `steps` wave operations in every wave, nothing else: what the pick log of a schedule looks like */
void only_steps(uint32_t *out, int steps) {
  uint32_t v = 0;
  for (int i = 0; i < steps; i++)
    v += (uint32_t)__popcll(wave_ballot((threadIdx.x & 1u) != 0u));
  out[threadIdx.x] = v;
}

/* a barrier that half of wave 0 never reaches: those lanes sit in a wave operation for ever */
void divergent_barrier() {
  if (threadIdx.x < 32)
    (void)wave_ballot(true);
  __syncthreads();
}
/* a wave operation after half of the wave has left */
void ballot_after_exit() {
  if ((threadIdx.x & 63u) >= 32u)
    return;
  (void)wave_ballot(true);
}

} // namespace

extern "C" {
void probe_word_for_all(int blocks, int waves, int barrier, uint32_t *out) {
  hipemu::launch(dim3(blocks), dim3(64 * waves), 64, [=] { word_for_all(out, barrier != 0); });
}
void probe_flag_handoff(int waves, int waiter, int work, uint32_t *out) { /* out: 128 results, then the two flag words */
  out[128] = out[129] = 0u;
  hipemu::launch(dim3(1), dim3(64 * waves), 64, [=] { flag_handoff(out, out + 128, waiter, work); });
}
void probe_append_index(int gx, int gy, int gz, uint32_t *list) {
  hipemu::launch(dim3(gx, gy, gz), dim3(64), 0, [=] { append_index(list); });
}
void probe_only_steps(int blocks, int waves, int steps, uint32_t *out) {
  hipemu::launch(dim3(blocks), dim3(64 * waves), 0, [=] { only_steps(out, steps); });
}
void probe_divergent_barrier(int waves) {
  hipemu::launch(dim3(1), dim3(64 * waves), 0, [] { divergent_barrier(); });
}
void probe_ballot_after_exit(int waves) {
  hipemu::launch(dim3(1), dim3(64 * waves), 0, [] { ballot_after_exit(); });
}
}
