"""The machine-ops probe's inputs and checks, shared by the emulated suite (tests/test_ops_emulated.py: the emulator's twin of
gfx950_ops.hpp) and the GPU suite (tests/test_gpu_ops.py: the product header through libachip_opsprobe.so).  Inputs are seeded and
built once; what a case is there for is asserted with the reference (tests/ops_ref.py) before anything runs.  A backend only has
to place bytes at a 256-byte aligned address and read them back; every buffer lies between guards that are checked afterwards.
TESTS ONLY."""
import ctypes as C
import itertools

import numpy as np

import ops_ref as R

BLOCK = 256
MAX_GRID = 64
GUARD = 0xA5
GUARD_BYTES = 256
M32 = 0xFFFFFFFF

# the order of the probe's outputs (tests/opsprobe/ops_probe_kernels.hpp)
ARITH_OPS = ("alignbit", "dot4_u8", "bfe_u32", "mad_i24", "mul_u24", "bitreverse32", "opaque")
WAVE_OUTS = ("ballot_lo", "ballot_hi", "lane_bit_ballot", "lane_bit_mem", "shfl", "shfl_up", "shfl_up_1", "read_0", "read_1", "read_63",
             "read_uniform", "read_vgpr", "uniform", "scan", "xor_last", "shift_up1")
LDS_BYTE_FORMS = tuple((off, hi) for off in (0, 1, 2, 3, 7) for hi in (False, True))
GM_OFFSETS, GM_SLOT, GM_REGIONS = 144, 256, 5
GM_STORES = (("store_u16_unaligned", 2), ("store_u1_unaligned", 4), ("store_u2_unaligned", 8), ("store_u4_unaligned", 16), ("store_u4_nt", 16))
# the compile-time arguments of the folded kernel: held against the table the probe library itself reports
CONST_BFE = ((0, 0), (0, 32), (0, 24), (0, 31), (0, 1), (8, 8), (24, 8), (24, 24), (31, 1), (31, 31), (31, 32), (32, 8), (16, 0), (0, 33),
             (40, 63), (255, 255))
CONST_ALIGN = (0, 1, 8, 24, 31, 32, 33, 40, 63, 255)
CONST_V, CONST_LO = 0x89ABCDEF, 0x01234567

EDGES = (0, 1, 2, 0xFF, 0x100, 0x7FFFFF, 0x800000, 0xFFFFFF, 0x1000000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)
COUNTS = tuple(range(41)) + (63, 64, 255)  # shifts, offsets, widths


def declare(lib):
    """argument types of the probe's entries (the device library and the emulator's driver have the same)"""
    p, i, u, q = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64
    for name, args in (("opsprobe_const_table", [p]), ("opsprobe_lane_arith", [i, p, p, p, u, p, p]), ("opsprobe_lane_const", [i, p, p, u, p, p]),
                       ("opsprobe_wave", [i] + [p] * 10), ("opsprobe_lds_bytes", [i, p, p, p, p, p]), ("opsprobe_lds_or", [i] + [p] * 8),
                       ("opsprobe_gmem", [p] * 5), ("opsprobe_atomics", [i, p, p, p, p, p, q, p, p, p, p, p]), ("opsprobe_arrival", [p] * 5)):
        f = getattr(lib, name)
        f.restype, f.argtypes = C.c_int, args
    return lib


class HostBackend:
    """buffers in this process's memory (the emulator)"""
    stream = None

    class _Placed:
        def __init__(self, data):
            self.raw = np.empty(data.size + 256, dtype=np.uint8)
            start = (-self.raw.ctypes.data) % 256
            self.view = self.raw[start:start + data.size]
            self.view[:] = data
            self.addr = self.view.ctypes.data

        def read(self):
            return self.view.copy()

    def place(self, data):
        return self._Placed(data)

    def sync(self):
        pass


class Buf:
    """payload bytes between two guards, at a 256-byte aligned address"""

    def __init__(self, be, payload):
        payload = np.ascontiguousarray(payload)
        self.dtype, self.n = payload.dtype, payload.size
        raw = payload.view(np.uint8).reshape(-1)
        self.nbytes = raw.size
        self.placed = be.place(np.concatenate([np.full(GUARD_BYTES, GUARD, np.uint8), raw, np.full(GUARD_BYTES, GUARD, np.uint8)]))
        assert self.placed.addr % 256 == 0, "a buffer's base address must be a multiple of 256"
        self.addr = self.placed.addr + GUARD_BYTES

    def read(self, what):
        got = self.placed.read()
        assert (got[:GUARD_BYTES] == GUARD).all(), f"{what}: a store in front of the buffer"
        assert (got[GUARD_BYTES + self.nbytes:] == GUARD).all(), f"{what}: a store behind the buffer"
        return got[GUARD_BYTES:GUARD_BYTES + self.nbytes].view(self.dtype).copy()


def _out(be, count, dtype=np.uint32):
    """an output buffer: guard-filled throughout"""
    return Buf(be, np.full(count * np.dtype(dtype).itemsize, GUARD, np.uint8).view(dtype))


def _u32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64).astype(np.uint32))


_cache = {}


def _once(fn):
    def wrapped():
        if fn.__name__ not in _cache:
            v = fn()
            for a in (v.values() if isinstance(v, dict) else v):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            _cache[fn.__name__] = v
        return _cache[fn.__name__]
    return wrapped


def _first_bad(got, want):
    bad = np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))
    return int(bad[0]), bad.size


# ==== lane arithmetic ==============================================================================================================
@_once
def arith_inputs():
    second = sorted(set(EDGES) | set(COUNTS))
    t = np.array(list(itertools.product(EDGES, second, second)), dtype=np.uint64)
    rng = np.random.default_rng(9501)
    rnd = rng.integers(0, 1 << 32, size=(4096, 3), dtype=np.uint64)
    rnd[1024:2048, 2] &= 63  # shifts and widths that are not all masked to noise
    rnd[2048:3072, 1] &= 63
    rnd[3072:, 1:] &= 63
    t = np.concatenate([t, rnd])
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    # what the table is there for
    assert ((b == 0) & (c == 0)).any() and ((c == 32)).any() and (c == 0).any(), "bfe_u32: widths 0 and 32"
    assert (c >= 32).any() and set(COUNTS) <= set(c.tolist()) and set(COUNTS) <= set(b.tolist()), "alignbit / bfe_u32: every count, shifts of 32 and more"
    assert ((a >> 24 != 0) & (b >> 24 != 0)).any(), "24-bit multiplies: bits above bit 23 in both operands"
    assert (((a >> 23) & 1 == 1) & ((b >> 23) & 1 == 0) & (b & 0xFFFFFF != 0)).any(), "mad_i24: a negative times a positive operand"
    assert (((a & 0xFFFFFF) * (b & 0xFFFFFF)) >> 32 != 0).any(), "mul_u24: a product that passes 2^32"
    assert ((a >> 24 != 0) & (b >> 24 != 0) & (c == M32)).any(), "dot4_u8: byte 3 set in both, a sum that wraps"
    want = {"alignbit": R.alignbit(a, b, c), "dot4_u8": R.dot4_u8(a, b, c), "bfe_u32": R.bfe_u32(a, b, c), "mad_i24": R.mad_i24(a, b, c),
            "mul_u24": R.mul_u24(a, b), "bitreverse32": R.bitreverse32(a), "opaque": R.opaque(a)}
    assert (want["bfe_u32"][(c & 31) == 0] == 0).all()
    assert (want["alignbit"][(c & 31) == 0] == b[(c & 31) == 0]).all()
    return {"a": _u32(a), "b": _u32(b), "c": _u32(c), "want": want}


def run_lane_arith(lib, be):
    ci = arith_inputs()
    n = ci["a"].size
    a, b, c = Buf(be, ci["a"]), Buf(be, ci["b"]), Buf(be, ci["c"])
    out = _out(be, len(ARITH_OPS) * n)
    assert lib.opsprobe_lane_arith(MAX_GRID, a.addr, b.addr, c.addr, n, out.addr, be.stream) == 0
    be.sync()
    got = out.read("lane arithmetic").reshape(len(ARITH_OPS), n)
    for buf, name in ((a, "a"), (b, "b"), (c, "c")):
        assert np.array_equal(buf.read(name), ci[name]), f"lane arithmetic: input {name} was written"
    for k, op in enumerate(ARITH_OPS):
        if not np.array_equal(got[k], ci["want"][op]):
            i, nbad = _first_bad(got[k], ci["want"][op])
            raise AssertionError(f"{op}(0x{ci['a'][i]:08X}, 0x{ci['b'][i]:08X}, 0x{ci['c'][i]:08X}) = 0x{got[k][i]:08X}, want "
                                 f"0x{ci['want'][op][i]:08X} (triple {i}, thread {i % (MAX_GRID * BLOCK)}; {nbad} of {n} differ)")


@_once
def const_inputs():
    rng = np.random.default_rng(9502)
    pairs = np.array(list(itertools.product(EDGES, EDGES)), dtype=np.uint64)
    t = np.concatenate([pairs, rng.integers(0, 1 << 32, size=(512 - len(pairs), 2), dtype=np.uint64)])
    a, b = t[:, 0], t[:, 1]
    n = a.size
    assert {(0, 0), (0, 32), (0, 24), (0, 31)} <= set(CONST_BFE) and {0, 24, 31, 32} <= set(CONST_ALIGN)
    cv, cl = np.full(n, CONST_V, np.uint64), np.full(n, CONST_LO, np.uint64)
    rows = [R.bfe_u32(a, np.full(n, o), np.full(n, w)) for o, w in CONST_BFE] + [R.alignbit(a, b, np.full(n, s)) for s in CONST_ALIGN]
    rows += [R.bfe_u32(cv, np.full(n, o), np.full(n, w)) for o, w in CONST_BFE] + [R.alignbit(cv, cl, np.full(n, s)) for s in CONST_ALIGN]
    names = [f"bfe_u32(v, {o}, {w})" for o, w in CONST_BFE] + [f"alignbit(hi, lo, {s})" for s in CONST_ALIGN]
    names += [f"bfe_u32(0x{CONST_V:08X}, {o}, {w})" for o, w in CONST_BFE] + [f"alignbit(0x{CONST_V:08X}, 0x{CONST_LO:08X}, {s})" for s in CONST_ALIGN]
    return {"a": _u32(a), "b": _u32(b), "want": np.stack(rows), "names": names}


def run_lane_const(lib, be):
    ci = const_inputs()
    table = (C.c_uint32 * 64)()
    k = lib.opsprobe_const_table(C.addressof(table))
    mine = [x for p in CONST_BFE for x in p] + list(CONST_ALIGN) + [CONST_V, CONST_LO]
    assert list(table[:k]) == mine, "the probe's compile-time arguments are not the ones this table expects"
    n = ci["a"].size
    a, b = Buf(be, ci["a"]), Buf(be, ci["b"])
    out = _out(be, len(ci["names"]) * n)
    assert lib.opsprobe_lane_const(2, a.addr, b.addr, n, out.addr, be.stream) == 0
    be.sync()
    got = out.read("folded lane arithmetic").reshape(len(ci["names"]), n)
    for k, name in enumerate(ci["names"]):
        if not np.array_equal(got[k], ci["want"][k]):
            i, nbad = _first_bad(got[k], ci["want"][k])
            raise AssertionError(f"{name} with compile-time arguments, v / hi = 0x{ci['a'][i]:08X}, lo = 0x{ci['b'][i]:08X}: "
                                 f"0x{got[k][i]:08X}, want 0x{ci['want'][k][i]:08X} (element {i}; {nbad} of {n} differ)")


# ==== wave operations ================================================================================================================
WAVE_GRID = 64
SHFL_UP_DISTANCES = (0, 1, 15, 16, 17, 32, 63)


@_once
def wave_inputs():
    rng = np.random.default_rng(9503)
    nw = WAVE_GRID * 4
    val = rng.integers(0, 1 << 32, size=(nw, 64), dtype=np.uint64)
    val[0] = 0
    val[1] = M32
    val[2] = np.arange(1, 65)
    for p in range(64):  # waves 4..67: one non-zero lane each
        val[4 + p] = 0
        val[4 + p, p] = int(rng.integers(1, 1 << 32))
    # waves 68..: random, with a few low values mixed in so that ballots and the small scans are not all noise
    val[200:] &= rng.integers(0, 1 << 32, size=(nw - 200, 64), dtype=np.uint64)
    idx = rng.integers(0, 64, size=(nw, 64), dtype=np.int64)
    for w in range(nw):
        kind = (w // 4 + w) % 4  # (every kind meets every wave of a workgroup)
        if kind == 0:
            idx[w] = rng.permutation(64)
        elif kind == 1:
            idx[w] = 0
        elif kind == 2:
            idx[w] = 63
    wdist = np.array([SHFL_UP_DISTANCES[w % 7] for w in range(nw)], dtype=np.int64)
    widx = np.where(np.arange(nw) % 5 < 3, np.array([0, 1, 63, 0, 0])[np.arange(nw) % 5], rng.integers(0, 64, size=nw))
    vsel = np.where(np.arange(nw) % 3 == 0, 63, rng.integers(0, 64, size=nw))  # the lane the vector-register select names
    vsel[7], vsel[8], vsel[9] = 0, 15, 16
    lo = np.minimum(vsel, rng.integers(0, 16, size=nw))
    sel = np.repeat((((vsel - lo) << 4) | lo).reshape(-1, 1), 64, axis=1)
    assert (((sel >> 4) + (sel & 15)) == vsel.reshape(-1, 1)).all()
    wfirst = rng.integers(0, 1 << 32, size=nw, dtype=np.uint64)
    wval = rng.integers(0, 1 << 32, size=nw, dtype=np.uint64)
    wmask = rng.integers(0, 1 << 63, size=nw, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=nw, dtype=np.uint64)
    wmask[0], wmask[1], wmask[2], wmask[3] = 0, (1 << 64) - 1, 1, 1 << 63
    # what the table is there for
    for b in range(WAVE_GRID):
        four = val[4 * b:4 * b + 4]
        assert len({four[i].tobytes() for i in range(4)}) == 4, "the four waves of a workgroup hold different data"
        assert len(set(wfirst[4 * b:4 * b + 4].tolist())) == 4 and len(set(wval[4 * b:4 * b + 4].tolist())) == 4
    sums = val.sum(axis=1, dtype=np.uint64)
    assert (sums[1] >> 32) != 0 and (sums[68:] >> 32 != 0).all(), "scans that wrap mod 2^32"
    assert all((val[4 + p] != 0).sum() == 1 and val[4 + p, p] != 0 for p in range(64))
    for w4 in range(4):  # every distance, and every kind of source, in every wave position of a workgroup, on random values
        ws = np.arange(68, nw)
        ws = ws[ws % 4 == w4]
        assert set(wdist[ws].tolist()) == set(SHFL_UP_DISTANCES)
        assert {0, 1, 63} <= set(widx[ws].tolist()) and 63 in vsel[ws].tolist()
        assert any((idx[w] == 0).all() for w in ws) and any((idx[w] == 63).all() for w in ws)
        assert any(sorted(idx[w].tolist()) == list(range(64)) and (idx[w] != np.arange(64)).any() for w in ws)
    bal = R.wave_ballot(val & 1)
    bal2 = R.wave_ballot((val >> 1) & 1)
    want = {
        "ballot_lo": np.repeat(_u32(bal & np.uint64(M32)).reshape(-1, 1), 64, axis=1),
        "ballot_hi": np.repeat(_u32(bal >> np.uint64(32)).reshape(-1, 1), 64, axis=1),
        "lane_bit_ballot": R.lane_bit(bal2 >> np.uint64(1)),
        "lane_bit_mem": R.lane_bit(wmask),
        "shfl": R.wave_shfl(val, idx),
        "shfl_up": R.wave_shfl_up(val, wdist),
        "shfl_up_1": R.wave_shfl_up(val, np.ones(nw, dtype=np.int64)),
        "read_0": R.wave_read_lane(val, np.full(nw, 0)),
        "read_1": R.wave_read_lane(val, np.full(nw, 1)),
        "read_63": R.wave_read_lane(val, np.full(nw, 63)),
        "read_uniform": R.wave_read_lane(val, widx),
        "read_vgpr": R.wave_read_lane(val, vsel),
        "uniform": np.repeat(R.wave_uniform(wval).reshape(-1, 1), 64, axis=1),
        "scan": R.wave_inclusive_scan(val),
        "xor_last": R.wave_xor_to_last(val),
        "shift_up1": R.wave_shift_up1(val, wfirst),
    }
    return {"val": _u32(val), "idx": _u32(idx), "sel": _u32(sel), "wdist": _u32(wdist), "widx": _u32(widx), "wfirst": _u32(wfirst),
            "wval": _u32(wval), "wmask": np.ascontiguousarray(wmask.astype("<u8")).view(np.uint32), "want": want}


def run_wave(lib, be):
    ci = wave_inputs()
    nw = WAVE_GRID * 4
    names = ("val", "idx", "sel", "wdist", "widx", "wfirst", "wval", "wmask")
    bufs = [Buf(be, ci[k]) for k in names]
    out = _out(be, len(WAVE_OUTS) * nw * 64)
    assert lib.opsprobe_wave(WAVE_GRID, *[b.addr for b in bufs], out.addr, be.stream) == 0
    be.sync()
    got = out.read("wave operations").reshape(len(WAVE_OUTS), nw, 64)
    for k, name in enumerate(WAVE_OUTS):
        want = np.asarray(ci["want"][name])
        if name == "xor_last":  # valid in lane 63 only: the other lanes are taken as they come
            want = np.concatenate([got[k][:, :63], want.reshape(-1, 1)], axis=1)
        if not np.array_equal(got[k], want):
            i, nbad = _first_bad(got[k], want)
            w, lane = divmod(i, 64)
            raise AssertionError(f"wave op {name}: wave {w} (wave {w % 4} of workgroup {w // 4}) lane {lane}: 0x{got[k][w][lane]:08X}, want "
                                 f"0x{want[w][lane]:08X}; {nbad} values differ; the wave's values {[hex(int(x)) for x in ci['val'][w][:4]]}.., "
                                 f"idx[lane] {ci['idx'][w][lane]}, distance {ci['wdist'][w]}, uniform lane {ci['widx'][w]}, select word "
                                 f"0x{ci['sel'][w][0]:X}, first 0x{ci['wfirst'][w]:08X}")


# ==== LDS ============================================================================================================================
LDS_GRID = 2


@_once
def lds_byte_inputs():
    rng = np.random.default_rng(9504)
    n = LDS_GRID * BLOCK
    pat = rng.integers(0, 1 << 32, size=4 * n, dtype=np.uint64)
    phase = np.arange(n) % 9
    v = rng.integers(0, 256, size=(n, 4), dtype=np.uint64)
    for i in range(n):
        while len(set(v[i].tolist())) != 4:
            v[i] = rng.integers(0, 256, size=4)
    v = v[:, 0] | v[:, 1] << 8 | v[:, 2] << 16 | v[:, 3] << 24
    assert (phase % 2 == 1).any() and phase.max() + 7 <= 15, "odd slot addresses; the byte stays inside the lane's slot"
    slots = _u32(pat).view(np.uint8).reshape(n, 16)
    want = [R.ds_store_byte(slots, phase + off, v, hi).reshape(-1).view(np.uint32) for off, hi in LDS_BYTE_FORMS]
    for w in want:
        assert ((w.view(np.uint8).reshape(n, 16) != slots).sum(axis=1) <= 1).all()
    return {"pat": _u32(pat), "phase": _u32(phase), "v": _u32(v), "want": np.stack(want)}


def run_lds_bytes(lib, be):
    ci = lds_byte_inputs()
    n = LDS_GRID * BLOCK
    pat, phase, v = Buf(be, ci["pat"]), Buf(be, ci["phase"]), Buf(be, ci["v"])
    out = _out(be, len(LDS_BYTE_FORMS) * 4 * n)
    assert lib.opsprobe_lds_bytes(LDS_GRID, pat.addr, phase.addr, v.addr, out.addr, be.stream) == 0
    be.sync()
    got = out.read("LDS byte stores").reshape(len(LDS_BYTE_FORMS), 4 * n)
    for k, (off, hi) in enumerate(LDS_BYTE_FORMS):
        if not np.array_equal(got[k], ci["want"][k]):
            i, _ = _first_bad(got[k].view(np.uint8), ci["want"][k].view(np.uint8))
            t, byte = divmod(i, 16)
            raise AssertionError(f"ds_store_byte<{off}, {str(hi).lower()}>: thread {t} (lane {t % 64}), slot byte {byte}: "
                                 f"0x{got[k].view(np.uint8)[i]:02X}, want 0x{ci['want'][k].view(np.uint8)[i]:02X}; address 16 * {t % BLOCK} + "
                                 f"{ci['phase'][t]}, v = 0x{ci['v'][t]:08X}, slot before {ci['pat'][4 * t:4 * t + 4].tolist()}")


@_once
def lds_or_inputs():
    rng = np.random.default_rng(9505)
    n = LDS_GRID * BLOCK
    init = rng.integers(0, 1 << 32, size=n, dtype=np.uint64) & rng.integers(0, 1 << 32, size=n, dtype=np.uint64) & 0x0F0F0F0F
    plain_words = rng.choice(256, size=24, replace=False)
    groups = rng.choice(64, size=6, replace=False)
    at = np.stack([rng.choice(plain_words, size=n), rng.choice(groups, size=n)], axis=1)
    vals = rng.integers(0, 1 << 32, size=(4, n), dtype=np.uint64) & rng.integers(0, 1 << 32, size=(4, n), dtype=np.uint64)
    vals[:, ::7] = 0  # (an OR of nothing)
    want = []
    for b in range(LDS_GRID):
        s = slice(b * BLOCK, (b + 1) * BLOCK)
        targets = np.concatenate([at[s, 0], 4 * at[s, 1], 4 * at[s, 1] + 1, 4 * at[s, 1] + 2])
        want.append(R.ds_or(init[s], targets, np.concatenate([vals[0, s], vals[1, s], vals[2, s], vals[3, s]])))
        # two lanes of one wave, and of two waves, onto one word, with disjoint and with overlapping bits: in both forms
        for tg, vv in ((at[s, 0], vals[0, s]), (at[s, 1], vals[2, s])):
            seen = set()
            for i, j in itertools.combinations(range(BLOCK), 2):
                if tg[i] == tg[j] and vv[i] and vv[j]:
                    seen.add((i // 64 == j // 64, (int(vv[i]) & int(vv[j])) == 0))
                    if len(seen) == 4:
                        break
            assert len(seen) == 4, "ds_or: same / different wave x disjoint / overlapping bits onto one word"
    return {"init": _u32(init), "at": _u32(at.reshape(-1)), "plain": _u32(vals[0]), "off0": _u32(vals[1]), "off4": _u32(vals[2]),
            "off8": _u32(vals[3]), "want": np.concatenate(want)}


def run_lds_or(lib, be):
    ci = lds_or_inputs()
    bufs = [Buf(be, ci[k]) for k in ("init", "at", "plain", "off0", "off4", "off8")]
    out = _out(be, LDS_GRID * BLOCK)
    assert lib.opsprobe_lds_or(LDS_GRID, *[b.addr for b in bufs], out.addr, be.stream) == 0
    be.sync()
    got = out.read("LDS ORs")
    if not np.array_equal(got, ci["want"]):
        i, nbad = _first_bad(got, ci["want"])
        b, word = divmod(i, BLOCK)
        at = ci["at"].reshape(-1, 2)[b * BLOCK:(b + 1) * BLOCK]
        who = [(t, "ds_or_u32") for t in range(BLOCK) if at[t, 0] == word]
        who += [(t, f"ds_or_u32_at<{4 * (word % 4)}>") for t in range(BLOCK) if at[t, 1] == word // 4 and word % 4 < 3]
        raise AssertionError(f"LDS OR: workgroup {b} word {word}: 0x{got[i]:08X}, want 0x{ci['want'][i]:08X}, before 0x{ci['init'][i]:08X}; "
                             f"ORed into by (thread, op) {who}; {nbad} words differ")


# ==== global memory ===================================================================================================================
@_once
def gmem_inputs():
    rng = np.random.default_rng(9506)
    vals = _u32(rng.integers(0, 1 << 32, size=4 * GM_OFFSETS, dtype=np.uint64))
    noise = rng.integers(0, 256, size=256, dtype=np.uint8)
    want = np.full(GM_REGIONS * GM_OFFSETS * GM_SLOT, GUARD, np.uint8)
    for k, (name, nb) in enumerate(GM_STORES):
        for t in range(GM_OFFSETS):
            if name == "store_u4_nt" and t % 16:
                continue
            at = (k * GM_OFFSETS + t) * GM_SLOT + t
            words = vals[4 * t:4 * t + 4]
            want[at:at + nb] = R.le_bytes(words, nb) if nb > 2 else R.le_bytes(words[:1] & 0xFFFF, 2)
    assert GM_OFFSETS + 16 <= GM_SLOT and GM_OFFSETS >= 128 + 16, "every phase of a 128-byte line, and stores across its end"
    loads = _u32([R.load_u32(noise, t) for t in range(GM_OFFSETS)])
    return {"vals": vals, "noise": noise, "want": want, "loads": loads}


def run_gmem(lib, be):
    ci = gmem_inputs()
    vals, noise = Buf(be, ci["vals"]), Buf(be, ci["noise"])
    store = _out(be, GM_REGIONS * GM_OFFSETS * GM_SLOT, np.uint8)
    loads = _out(be, GM_OFFSETS)
    assert store.addr % 128 == 0 and noise.addr % 128 == 0, "the bases must be 128-byte aligned: offsets are phases of a line"
    assert noise.nbytes >= GM_OFFSETS + 3, "the loads stay inside the noise buffer"
    assert lib.opsprobe_gmem(store.addr, vals.addr, noise.addr, loads.addr, be.stream) == 0
    be.sync()
    got = store.read("unaligned stores")
    if not np.array_equal(got, ci["want"]):
        i, nbad = _first_bad(got, ci["want"])
        slot, byte = divmod(i, GM_SLOT)
        k, t = divmod(slot, GM_OFFSETS)
        raise AssertionError(f"{GM_STORES[k][0]} at line offset {t} (thread {t}): byte {byte} of its slot is 0x{got[i]:02X}, want "
                             f"0x{ci['want'][i]:02X} (0x{GUARD:02X} = untouched); operands {[hex(int(x)) for x in ci['vals'][4 * t:4 * t + 4]]}; "
                             f"{nbad} bytes differ")
    gl = loads.read("unaligned loads")
    assert np.array_equal(noise.read("the loads' source"), ci["noise"])
    if not np.array_equal(gl, ci["loads"]):
        i, nbad = _first_bad(gl, ci["loads"])
        raise AssertionError(f"load_u32_unaligned_nt at line offset {i} (thread {i}): 0x{gl[i]:08X}, want 0x{ci['loads'][i]:08X}; {nbad} differ")


# ==== scoped atomics and the hand-off ===================================================================================================
ATOM_GRID = 64
ATOM_INC64 = (1 << 32) + 3
ATOM_START64 = 0xFFFFFF00


@_once
def atomics_inputs():
    rng = np.random.default_rng(9507)
    n = ATOM_GRID * BLOCK
    wg_in = np.zeros((ATOM_GRID, 4), dtype=np.uint64)
    wg_in[:, 0] = rng.integers(0, 1 << 32, size=ATOM_GRID, dtype=np.uint64)
    wg_in[:, 1] = rng.integers(1, 1 << 32, size=ATOM_GRID, dtype=np.uint64) | 1  # odd: 256 different old values
    wg_in[0, :2] = (0xFFFFFF00, 3)  # wraps on the way
    wg_in[1, :2] = (0, 1)
    wg_in[:, 2] = rng.integers(0, 1 << 32, size=ATOM_GRID, dtype=np.uint64)
    xv = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    wg64 = rng.integers(1 << 32, 1 << 63, size=ATOM_GRID, dtype=np.uint64)
    assert R.fetch_add_final(0xFFFFFF00, 3, BLOCK, 64) >> 32, "a workgroup's adds wrap mod 2^32"
    assert ATOM_INC64 >> 32 and (ATOM_START64 + n * ATOM_INC64) < 1 << 64 and ((ATOM_START64 & M32) + n * 3) >> 32, "64-bit adds with a carry"
    return {"wg_in": _u32(wg_in.reshape(-1)), "xv": _u32(xv), "wg64": np.ascontiguousarray(wg64.astype(np.uint64))}


def run_atomics(lib, be):
    ci = atomics_inputs()
    n = ATOM_GRID * BLOCK
    wg_in, xv, wg64 = Buf(be, ci["wg_in"]), Buf(be, ci["xv"]), Buf(be, ci["wg64"])
    old, wg_out = _out(be, n), _out(be, 2 * ATOM_GRID)
    counter = Buf(be, np.array([ATOM_START64], dtype=np.uint64))
    old64, slot64, back64 = _out(be, n, np.uint64), _out(be, ATOM_GRID, np.uint64), _out(be, ATOM_GRID, np.uint64)
    assert lib.opsprobe_atomics(ATOM_GRID, wg_in.addr, xv.addr, old.addr, wg_out.addr, counter.addr, ATOM_INC64, old64.addr, wg64.addr,
                                slot64.addr, back64.addr, be.stream) == 0
    be.sync()
    g_old, g_out = old.read("wg_fetch_add_u32's results").reshape(ATOM_GRID, BLOCK), wg_out.read("the workgroups' words").reshape(ATOM_GRID, 2)
    w = ci["wg_in"].reshape(ATOM_GRID, 4)
    for b in range(ATOM_GRID):
        start, inc = int(w[b, 0]), int(w[b, 1])
        assert sorted(g_old[b].tolist()) == R.fetch_add_progression(start, inc, BLOCK, 32), \
            f"wg_fetch_add_u32: workgroup {b}, start 0x{start:08X}, addend 0x{inc:08X}: the returned values are not start + k * addend, k = 0..255"
        assert int(g_out[b, 0]) == R.fetch_add_final(start, inc, BLOCK, 32), \
            f"wg_fetch_add_u32 / wg_load_u32: workgroup {b}: the word ends as 0x{g_out[b, 0]:08X}, start 0x{start:08X}, 256 x 0x{inc:08X}"
        x = R.xor_all(w[b, 2], ci["xv"][b * BLOCK:(b + 1) * BLOCK])
        assert int(g_out[b, 1]) == x, f"wg_store_u32 / wg_xor_u32: workgroup {b}: the word ends as 0x{g_out[b, 1]:08X}, want 0x{x:08X}"
    g64 = old64.read("agent_fetch_add_u64's results")
    assert sorted(g64.tolist()) == R.fetch_add_progression(ATOM_START64, ATOM_INC64, n, 64), \
        f"agent_fetch_add_u64: the {n} returned values are not 0x{ATOM_START64:X} + k * 0x{ATOM_INC64:X}"
    end = int(counter.read("the launch's counter")[0])
    assert end == R.fetch_add_final(ATOM_START64, ATOM_INC64, n, 64), f"agent_fetch_add_u64: the counter ends as 0x{end:X}"
    assert np.array_equal(slot64.read("agent_store_u64's words"), ci["wg64"]), "agent_store_u64: the stored words"
    assert np.array_equal(back64.read("agent_load_u64's results"), ci["wg64"]), "agent_load_u64: what the storing thread reads back"


@_once
def arrival_inputs():
    rng = np.random.default_rng(9508)
    word = rng.integers(1 << 31, 1 << 32, size=MAX_GRID, dtype=np.uint64)
    assert int(word.sum()) >> 32, "the collector's sum passes 2^32"
    return {"word": _u32(word), "sum": int(word.sum()) & M32}


def run_arrival(lib, be):
    ci = arrival_inputs()
    word = Buf(be, ci["word"])
    data, arrivals, res = Buf(be, np.zeros(MAX_GRID, np.uint32)), Buf(be, np.zeros(1, np.uint32)), Buf(be, np.zeros(3, np.uint32))
    assert lib.opsprobe_arrival(word.addr, data.addr, arrivals.addr, res.addr, be.stream) == 0
    be.sync()
    assert np.array_equal(data.read("the published words"), ci["word"]), "agent_store_u32: the published words"
    assert int(arrivals.read("the arrival counter")[0]) == MAX_GRID, "agent_arrive_u32: 64 arrivals"
    r = res.read("the collector's result").tolist()
    assert r[2] == 1, f"agent_arrive_u32: {r[2]} workgroups were handed {MAX_GRID - 1} (exactly one collects)"
    assert r[1] < MAX_GRID
    assert r[0] == ci["sum"], (f"agent_load_u32 behind agent_arrive_u32: collector {r[1]} read a sum of 0x{r[0]:08X}, the 64 published words add "
                               f"up to 0x{ci['sum']:08X}: a word was not visible to the last arriver")


FAMILIES = {"lane_arith": run_lane_arith, "lane_const": run_lane_const, "wave": run_wave, "lds_bytes": run_lds_bytes, "lds_or": run_lds_or,
            "gmem": run_gmem, "atomics": run_atomics, "arrival": run_arrival}
