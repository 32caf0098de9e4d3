"""What every operation of <gfx950_ops.hpp> must give, restated from the documented meaning of the instruction (the CDNA3/CDNA4
instruction set reference, HIP's programming guide for the shuffles, C++ for the atomics) and from neither header.  NumPy in 64-bit
integers, masked to 32 bits only where the instruction says so; nothing here wraps by accident.  TESTS ONLY."""
import numpy as np

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1


def _u(x):
    a = np.asarray(x)
    assert a.dtype.kind in "ui"
    a = a.astype(np.uint64)
    assert (a <= M32).all()
    return a


def _out(x):
    return (np.asarray(x, dtype=np.uint64) & np.uint64(M32)).astype(np.uint32)


# ---- lane arithmetic ----------------------------------------------------------------------------------------------------------
def alignbit(hi, lo, sh):
    """V_ALIGNBIT_B32: D = ({S0, S1} >> S2[4:0]) & 0xFFFFFFFF -- S0 the high dword, five bits of the shift count"""
    hi, lo, sh = _u(hi), _u(lo), _u(sh)
    return _out(((hi << np.uint64(32)) | lo) >> (sh & np.uint64(31)))


def dot4_u8(a, b, c):
    """V_DOT4_U32_U8 (no clamp): D = S0.u8[0] * S1.u8[0] + S0.u8[1] * S1.u8[1] + S0.u8[2] * S1.u8[2] + S0.u8[3] * S1.u8[3] + S2,
    the low 32 bits"""
    a, b, c = _u(a), _u(b), _u(c)
    s = c.copy()  # at most 2^32 - 1 + 4 * 255 * 255 < 2^33
    for k in range(4):
        s += ((a >> np.uint64(8 * k)) & np.uint64(0xFF)) * ((b >> np.uint64(8 * k)) & np.uint64(0xFF))
    return _out(s)


def bfe_u32(v, off, width):
    """V_BFE_U32: D = (S0 >> S1[4:0]) & ((1 << S2[4:0]) - 1) -- five bits of the offset and five of the width: 32 is 0 and yields 0"""
    v, off, width = _u(v), _u(off), _u(width)
    return _out((v >> (off & np.uint64(31))) & ((np.uint64(1) << (width & np.uint64(31))) - np.uint64(1)))


def _i24(x):
    """bits 23..0 as a signed number"""
    x = (_u(x) & np.uint64(0xFFFFFF)).astype(np.int64)
    return x - ((x >> 23) << 24)


def mad_i24(a, b, c):
    """V_MAD_I32_I24 (or V_MUL_I32_I24 and an add): D = S0.i24 * S1.i24 + S2.i32, the low 32 bits; .i24 is bits 23..0 sign-extended"""
    p = _i24(a) * _i24(b)  # |p| < 2^46
    return _out((p + _u(c).astype(np.int64)).astype(np.uint64))  # two's complement: the low 32 bits are those of the signed sum


def mul_u24(a, b):
    """V_MUL_U32_U24: D = S0.u24 * S1.u24, the low 32 bits; .u24 is bits 23..0"""
    return _out((_u(a) & np.uint64(0xFFFFFF)) * (_u(b) & np.uint64(0xFFFFFF)))  # < 2^48


def bitreverse32(v):
    """V_BFREV_B32: D[31 - i] = S0[i]"""
    v = _u(v)
    r = np.zeros_like(v)
    for i in range(32):
        r |= ((v >> np.uint64(i)) & np.uint64(1)) << np.uint64(31 - i)
    return _out(r)


def opaque(v):
    """the value itself"""
    return _out(_u(v))


# ---- wave operations: arrays of shape (waves, 64) ----------------------------------------------------------------------------
def _waves(x):
    a = _u(x)
    assert a.ndim == 2 and a.shape[1] == 64
    return a


def wave_ballot(pred):
    """ballot: bit l of the result is lane l's predicate, the same 64-bit word in every lane -> (waves,) uint64"""
    p = np.asarray(pred).astype(bool)
    assert p.ndim == 2 and p.shape[1] == 64
    return (p.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)  # (disjoint bits: a sum is an OR)


def lane_bit(mask):
    """inverse ballot: lane l's predicate is bit l of the wave's mask; mask (waves,) uint64 -> (waves, 64) of 0 / 1"""
    m = np.asarray(mask, dtype=np.uint64).reshape(-1, 1)
    return ((m >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(np.uint32)


def wave_shfl(v, src):
    """__shfl at width 64 (DS_BPERMUTE_B32): lane l gets lane src[l]'s value, src in 0..63"""
    v, src = _waves(v), np.asarray(src, dtype=np.int64)
    assert ((src >= 0) & (src < 64)).all()
    return _out(np.take_along_axis(v, src, axis=1))


def wave_shfl_up(v, d):
    """__shfl_up at width 64: lane l gets lane l - d's value, a lane below d keeps its own; d (waves,) in 0..63"""
    v, d = _waves(v), np.asarray(d, dtype=np.int64).reshape(-1, 1)
    assert ((d >= 0) & (d < 64)).all()
    lanes = np.arange(64, dtype=np.int64)[None, :]
    return _out(np.take_along_axis(v, np.where(lanes >= d, lanes - d, lanes), axis=1))


def wave_read_lane(v, lane):
    """V_READLANE_B32: one lane select per wave; every lane gets that lane's value; lane (waves,) in 0..63"""
    v, lane = _waves(v), np.asarray(lane, dtype=np.int64).reshape(-1, 1)
    assert ((lane >= 0) & (lane < 64)).all()
    return _out(np.repeat(np.take_along_axis(v, lane, axis=1), 64, axis=1))


def wave_uniform(x):
    """V_READFIRSTLANE_B32 of a value that is the same in every lane: the value"""
    return _out(_u(x))


def wave_inclusive_scan(v):
    """lane l gets v[0] + ... + v[l], mod 2^32"""
    return _out(np.cumsum(_waves(v), axis=1, dtype=np.uint64))  # < 64 * 2^32


def wave_xor_to_last(v):
    """lane 63 gets v[0] ^ ... ^ v[63]; -> (waves,)"""
    return _out(np.bitwise_xor.reduce(_waves(v), axis=1))


def wave_shift_up1(v, first):
    """lane l gets lane l - 1's value, lane 0 gets the wave's `first`; first (waves,)"""
    v = _waves(v)
    return _out(np.concatenate([_u(first).reshape(-1, 1), v[:, :63]], axis=1))


# ---- LDS ----------------------------------------------------------------------------------------------------------------------
def ds_store_byte(slot_bytes, at, v, hi):
    """DS_WRITE_B8 / DS_WRITE_B8_D16_HI: ONE byte, data[7:0] resp. data[23:16], at byte `at` of the slot; slot_bytes (n, 16) uint8"""
    out = np.array(slot_bytes, dtype=np.uint8, copy=True)
    byte = (_u(v) >> np.uint64(16 if hi else 0)) & np.uint64(0xFF)
    out[np.arange(out.shape[0]), np.asarray(at, dtype=np.int64)] = byte.astype(np.uint8)
    return out


def ds_or(words, targets, values):
    """DS_OR_B32 without return: words[t] |= v for every (t, v), in any order (an OR commutes)"""
    out = _u(words).copy()
    np.bitwise_or.at(out, np.asarray(targets, dtype=np.int64), _u(values))
    return _out(out)


# ---- global memory --------------------------------------------------------------------------------------------------------------
def le_bytes(words, nbytes):
    """little-endian bytes of consecutive 32-bit words (the first word lowest), the first nbytes of them"""
    return np.frombuffer(np.asarray(words, dtype="<u4").tobytes(), dtype=np.uint8)[:nbytes].copy()


def load_u32(buf, at):
    """four bytes at any byte offset, little-endian"""
    b = np.asarray(buf, dtype=np.uint8)
    return int(b[at]) | int(b[at + 1]) << 8 | int(b[at + 2]) << 16 | int(b[at + 3]) << 24


# ---- atomics --------------------------------------------------------------------------------------------------------------------
def fetch_add_progression(start, inc, count, bits):
    """what `count` fetch-adds of inc return, as a sorted list of Python integers: start + k * inc mod 2^bits"""
    return sorted((int(start) + k * int(inc)) & ((1 << bits) - 1) for k in range(count))


def fetch_add_final(start, inc, count, bits):
    return (int(start) + count * int(inc)) & ((1 << bits) - 1)


def xor_all(start, values):
    r = int(start)
    for v in np.asarray(values).reshape(-1).tolist():
        r ^= int(v)
    return r
