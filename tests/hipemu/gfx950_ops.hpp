/*
 * gfx950_ops.hpp (emulator twin) -- the interface of ascii-chat_amd/csrc/gfx950_ops.hpp on top of hip_emu.h's fibers, so
 * that the kernel sources compile unchanged under g++ and run on the CPU test box.  TESTS ONLY: found ahead of the
 * product header because the emulator build lists this directory first on the include path.
 *
 * Each operation states its DOMAIN as the product header does.  Inside it the two files give the same answer: the probe of
 * tests/opsprobe/ runs op by op against both and against tests/ops_ref.py (tests/test_ops_emulated.py here, tests/test_gpu_ops.py
 * on the device).  Outside it this file aborts where it can tell, so that every emulated suite polices the domain.
 */
#pragma once
#include <string.h>

#include "hip_emu.h"

/* an argument outside an operation's domain: say which, and stop (as hip_emu.h does for a wave op with exited lanes) */
#define ACHIP_EMU_DOMAIN(ok, op, arg)                                                                        \
  do {                                                                                                       \
    if (!(ok)) {                                                                                             \
      fprintf(stderr, "hipemu: %s outside its domain (%d; lane %d of wave %d)\n", op, (int)(arg), hipemu::lane(), hipemu::wave()); \
      abort();                                                                                               \
    }                                                                                                        \
  } while (0)

#define ACHIP_SMEM (hipemu::g_smem.data())
#define ACHIP_GLOBAL
#define ACHIP_EMULATED 1
#define ACHIP_DEVICE_ONLY(...)
#define ACHIP_WAVES_PER_EU(n)

namespace achip {

/* domain: addr + OFF any byte of the workgroup's LDS; HI takes bits 23..16 of v, else bits 7..0 */
template <int OFF, bool HI> inline void ds_store_byte(uint32_t addr, uint32_t v) {
  ACHIP_SMEM[addr + OFF] = (unsigned char)(HI ? v >> 16 : v);
}
/* domain: addr (+ OFF) a multiple of 4 */
inline void ds_or_u32(uint32_t addr, uint32_t v) { *reinterpret_cast<uint32_t *>(ACHIP_SMEM + addr) |= v; }
template <int OFF> inline void ds_or_u32_at(uint32_t addr, uint32_t v) { *reinterpret_cast<uint32_t *>(ACHIP_SMEM + addr + OFF) |= v; }
/* domain: any sh, of which bits 4..0 count */
inline uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (sh & 31u)); }
/* domain: any three words; the sum wraps mod 2^32 */
inline uint32_t dot4_u8(uint32_t a, uint32_t b, uint32_t c) {
  return (a & 0xFFu) * (b & 0xFFu) + ((a >> 8) & 0xFFu) * ((b >> 8) & 0xFFu) + ((a >> 16) & 0xFFu) * ((b >> 16) & 0xFFu) +
         (a >> 24) * (b >> 24) + c;
}
/* domain: any off and width, of each bits 4..0 count (a width of 32 is a width of 0) */
inline uint32_t bfe_u32(uint32_t v, uint32_t off, uint32_t width) { /* v_bfe_u32: offset and width modulo 32 */
  off &= 31u;
  width &= 31u;
  return width ? (v >> off) & ((1u << width) - 1u) : 0u;
}
/* domain (both 24-bit multiplies): any 32-bit patterns, bits 31..24 of a and b dropped */
inline int32_t mad_i24(int32_t a, int32_t b, int32_t c) { /* operands sign-extended from 24 bits, low 32 bits of the product */
  const int64_t sa = ((int32_t)((uint32_t)a << 8)) >> 8, sb = ((int32_t)((uint32_t)b << 8)) >> 8;
  return (int32_t)((uint32_t)(sa * sb) + (uint32_t)c);
}
inline uint32_t mul_u24(uint32_t a, uint32_t b) { return (uint32_t)((uint64_t)(a & 0xFFFFFFu) * (uint64_t)(b & 0xFFFFFFu)); }
inline void keep_alive(uint32_t, uint32_t) {}
inline uint32_t lds_base_addr() { return 0u; }
/* a wave's lanes run in lockstep on the GPU: every lane's stores precede the reads behind the fence.
 * domain: every lane of the wave gets here */
inline void lds_store_fence() { hipemu::wave_barrier(); }
inline void wave_lockstep() { hipemu::wave_barrier(); }
inline void wait_vmem_all() {}

/* fibers of one OS thread: no switch inside a plain read-modify-write.  domain (agent_*, wg_*): a naturally aligned word */
inline void agent_store_u64(unsigned long long *p, unsigned long long w) { *reinterpret_cast<volatile unsigned long long *>(p) = w; }
inline unsigned long long agent_load_u64(const unsigned long long *p) {
  return *reinterpret_cast<const volatile unsigned long long *>(p);
}
inline unsigned long long agent_fetch_add_u64(unsigned long long *p, unsigned long long v) {
  const unsigned long long old = *reinterpret_cast<volatile unsigned long long *>(p);
  *reinterpret_cast<volatile unsigned long long *>(p) = old + v;
  return old;
}
inline void agent_store_u32(uint32_t *p, uint32_t w) { *reinterpret_cast<volatile uint32_t *>(p) = w; }
inline uint32_t agent_load_u32(const uint32_t *p) { return *reinterpret_cast<const volatile uint32_t *>(p); }
inline uint32_t agent_arrive_u32(uint32_t *p) {
  const uint32_t old = *reinterpret_cast<volatile uint32_t *>(p);
  *reinterpret_cast<volatile uint32_t *>(p) = old + 1u;
  return old;
}
/* a lane that polled, found nothing and waits: counted, so that a test can tell whether a wait path ran (hip_emu.h) */
template <int N> inline void spin_nap() { hipemu::g_naps++; }
inline void wg_store_u32(uint32_t *p, uint32_t v) { *reinterpret_cast<volatile uint32_t *>(p) = v; }
inline uint32_t wg_load_u32(const uint32_t *p) { return *reinterpret_cast<const volatile uint32_t *>(p); }
inline uint32_t wg_fetch_add_u32(uint32_t *p, uint32_t v) {
  const uint32_t old = *reinterpret_cast<volatile uint32_t *>(p);
  *reinterpret_cast<volatile uint32_t *>(p) = old + v;
  return old;
}
inline void wg_xor_u32(uint32_t *p, uint32_t v) {
  *reinterpret_cast<volatile uint32_t *>(p) = *reinterpret_cast<volatile uint32_t *>(p) ^ v;
}

/* domain (every wave operation below): all 64 lanes alive, outside divergent control flow -- hip_emu.h aborts otherwise */
inline uint64_t wave_ballot(bool p) { return hipemu::ballot(p); }
/* domain: the same mask in every lane */
inline bool lane_bit(uint64_t wave_uniform_mask) { return ((wave_uniform_mask >> hipemu::lane()) & 1ull) != 0ull; }
/* domain: 0 <= d < 64 (the machine would wrap another d: refused here) */
inline uint32_t wave_shfl_up(uint32_t v, int d) {
  ACHIP_EMU_DOMAIN(d >= 0 && d < 64, "wave_shfl_up: distance", d);
  return hipemu::shfl_from(v, hipemu::lane() - d); /* src < 0 -> own value, like __shfl_up */
}
/* domain: lane in 0..63 and the same in every lane of the wave.  v_readlane_b32 takes ONE lane select for the wave: of an index
 * that differs between the lanes the compiler keeps the first lane's, and another lane number wraps -- both refused here */
inline uint32_t wave_read_lane(uint32_t v, int lane) {
  static uint32_t select[64][64]; /* [wave][lane], beside hipemu::g_wave_slots: one exchange for the value and the select */
  const int w = hipemu::wave(), l = hipemu::lane();
  ACHIP_EMU_DOMAIN(lane >= 0 && lane < 64, "wave_read_lane: lane", lane);
  hipemu::g_wave_slots[w][l] = v;
  select[w][l] = (uint32_t)lane;
  hipemu::wave_barrier();
  ACHIP_EMU_DOMAIN(select[w][0] == (uint32_t)lane, "wave_read_lane: a lane select that differs from lane 0's", lane);
  const uint32_t r = hipemu::g_wave_slots[w][lane];
  hipemu::wave_barrier();
  return r;
}
/* domain: src in 0..63 */
inline uint32_t wave_shfl(uint32_t v, int src) { return hipemu::shfl_from(v, src & 63); }
/* domain: a wave-uniform value.  NOT a wave operation here: it is legal in divergent code on the machine */
inline int wave_uniform(int v) { return v; }
inline uint32_t wave_inclusive_scan(uint32_t v) {
  const int l = hipemu::lane();
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = hipemu::shfl_from(v, l - d);
    if (l >= d)
      v += t;
  }
  return v;
}
/* the result is valid in lane 63 */
inline uint32_t wave_xor_to_last(uint32_t v) {
  const int l = hipemu::lane();
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = hipemu::shfl_from(v, l - d);
    if (l >= d)
      v ^= t;
  }
  return v;
}
/* domain: any v; `first` is read in lane 0 only */
inline uint32_t wave_shift_up1(uint32_t v, uint32_t first) {
  const int l = hipemu::lane();
  const uint32_t t = hipemu::shfl_from(v, l - 1);
  return l == 0 ? first : t;
}
/* domain: any word */
inline uint32_t bitreverse32(uint32_t v) {
  uint32_t r = 0;
  for (int i = 0; i < 32; i++)
    r |= ((v >> i) & 1u) << (31 - i);
  return r;
}

struct __attribute__((packed)) unaligned_u32 {
  uint32_t v;
};
/* domain: p any byte address with p[0..3] inside memory the caller owns */
inline uint32_t load_u32_unaligned_nt(const uint8_t *p) { return reinterpret_cast<const unaligned_u32 *>(p)->v; }
inline uint32_t opaque(uint32_t v) { return v; }
/* domain: p a multiple of 16 */
inline void store_u4_nt(uint8_t *p, uint4 v) { *reinterpret_cast<uint4 *>(p) = v; }
/* domain: any p; exactly the 16 / 8 / 4 / 2 bytes from p are written */
inline void store_u4_unaligned(uint8_t *p, uint4 v) { memcpy(p, &v, 16); }
inline void store_u2_unaligned(uint8_t *p, uint32_t a, uint32_t b) {
  memcpy(p, &a, 4);
  memcpy(p + 4, &b, 4);
}
inline void store_u1_unaligned(uint8_t *p, uint32_t a) { memcpy(p, &a, 4); }
inline void store_u16_unaligned(uint8_t *p, uint16_t a) { memcpy(p, &a, 2); }

inline unsigned long long cycle_now() { return 0ull; }
inline unsigned long long wall_now() { return 0ull; }

} // namespace achip
