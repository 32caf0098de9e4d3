"""Cases of the stand-alone checksum wire pass (crc_kernels.hpp, crc_math.hpp, launch_crc32c in hip_launch.hip) at its group,
round and span boundaries.  Deterministic (seeded numpy generators); the emulated tests (test_crc_boundaries.py) and the GPU
tests (test_gpu_crc.py) import it.  Every family asserts its own premise, so a case cannot silently stop being a boundary
case, and none is skipped or filtered out when the tests run.  TESTS ONLY.

A round is 16384 bytes: the 1024 threads of the one-workgroup kernel take 16 bytes each.  A batch names the path it is meant
for as (parts, rounds): parts == 1 is the one-workgroup kernel, otherwise `parts` spans of rounds * 4 KB each.  The GPU tests
assert the product's achip_crc_parts(max_len, n) against it before they run a batch; the emulated tests force it.  Content is
random bytes unless said otherwise; every slot's slack, from the end of the frame to the stride, is random non-zero bytes
(Batch.slab(slack_seed) regenerates the slack alone).

  (a) frame_tails      every length 0 .. 48 and k * 16384 - 17 .. k * 16384 + 17 for k in 1, 2, 4, 5, 8 (8: up to 131072):
                       every tail count with no group, with one, with a full round (no zero group in front) and with 1023
                       zero groups in front; the four-round prefetch loop at 4 and 5 rounds; the 128 KB ceiling
  (b) frame_content    zeros, FF FF FF FF + zeros (the folded initial value makes the first group zero), FF throughout, single
                       set bits at the group, round and frame edges, and two groups exchanged across lanes, waves and rounds
  (c) error_and_empty  the length codes 0xFFFFFFF0 / F7 / FF and length 0, first, in the middle and last in a batch
  (d) long_frames      the one-workgroup kernel above 128 KB (twelve slots of 196608 bytes)
  (e) span_edges       twelve 16 KB spans: every span edge -17 .. +17 of the first two and the last two spans, in batches of 3
  (f) span_batches     63, 64, 65, 128 and 129 span registers a frame (crc_finish_wave's batches of 64 and their zero
                       registers in front), a short frame next to a full one, lengths with several bits set above 2^16
  (g) wide_spans       eight 64 KB spans of sixteen rounds, 65 frames
  (h) len_bits         one frame of 2^24 + 65536 + 19 bytes: bits 24, 16, 4, 1 and 0 of the length
  (i) packets_only     crc_packets_kernel: arrays only, 1 / 256 / 257 / 600 frames, lengths up to 0xFFFFFFEF
  (j) pack_edges       (a, k <= 2), (c) and (e) through the COPY forms with the capacities of pack_capacities(), and 1100
                       frames of 0 .. 40 bytes (the offset prefix walks a 1024-thread workgroup more than once)

(h): achip_crc_parts(2^24 + 65536 + 19, 1) is 1029 spans of 16 KB (one buffer is far below the 512 spans of 64 KB from which
the launcher cuts wide ones), and 64 KB spans of this length number 258, not 257: the frame ends 19 bytes into span 258.
len_bits() therefore has the lone frame (1029 x 16 KB) and the same frame with a 19-byte one next to it (258 x 64 KB); the
bitwise oracle checksums the long frame once for both.

The bitwise oracle (orc.crc32c), measured on the CPU the suite was written on: family (a), 207 frames of 9.2 MB in all, 0.14 s
for the frame CRCs and 0.67 s for the whole expectation (frame CRC and both header forms' packet CRCs); family (h), 16.8 MB,
0.24 s for the frame CRC and 1.2 s for building the frame and its whole expectation.  (h) alone stays below two seconds, so
its random regions are not halved.

EMU_LEFT_OUT names what the emulated run leaves out; the GPU run leaves out nothing."""
import functools
import zlib

import numpy as np

import crc_ref as R
import orc

ROUND = 16384
ERR = (0xFFFFFFF0, 0xFFFFFFF7, 0xFFFFFFFF)
# (what, reason).  (h) runs under the emulator too: about eight seconds a run.
EMU_LEFT_OUT = (("pack_edges: the 1100 short frames at the capacities total - 1, exact end and 0",
                 "1100 workgroups of 1024 emulated threads take 55 s a call; the emulated run keeps the capacity 'total', and "
                 "the three other capacities run under the emulator over the batches of (a), (c) and (e)"),)


def dims_of(n):
    return [(80 + i % 300, 24 + i % 77) for i in range(n)]


def _rand(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


class Batch:
    """n slots of `stride` bytes; lens[i] the length word of slot i (an error code or len(frames[i])), frames[i] None behind
    an error code"""

    def __init__(self, name, max_len, lens, frames, parts, rounds, tight_stride=False):
        self.name, self.max_len, self.parts, self.rounds = name, max_len, parts, rounds
        self.lens = [int(l) for l in lens]
        self.frames = list(frames)
        self.n = len(self.lens)
        self.stride = (max_len + 15) // 16 * 16 + (0 if tight_stride else 16)
        self.dims = dims_of(self.n)
        assert self.n == len(self.frames) and self.n > 0
        for l, f in zip(self.lens, self.frames):
            assert (f is None and l >= R.ERR_FROM) or (len(f) == l <= max_len), (name, l)
        self._expect = self._packed = None

    def slab(self, slack_seed=0):
        """uint8[n * stride]: the frames in their slots, random non-zero bytes everywhere else"""
        rng = np.random.default_rng([zlib.crc32(self.name.encode()), slack_seed])
        s = rng.integers(1, 256, self.n * self.stride, dtype=np.uint8)
        for i, f in enumerate(self.frames):
            if f:
                s[i * self.stride:i * self.stride + len(f)] = np.frombuffer(f, dtype=np.uint8)
        return s

    def len_words(self):
        return np.array(self.lens, dtype=np.uint32)

    def dim_words(self):
        return np.array(self.dims, dtype=np.uint32).reshape(self.n, 2)

    def expect(self):
        """crc_ref.expect of the batch, computed once"""
        if self._expect is None:
            self._expect = R.expect(self.frames, self.lens, self.dims)
        return self._expect

    def packed(self):
        """crc_ref.packed_reference of the batch: (offsets [n + 1], the packed bytes)"""
        if self._packed is None:
            self._packed = R.packed_reference(self.slab(), self.stride, self.lens)
        return self._packed

    def __repr__(self):
        return f"<{self.name}: {self.n} x {self.max_len}, {self.parts} part(s)>"


def frame_geometry(length):
    """(whole groups, tail bytes, rounds, zero groups in front) of the one-workgroup kernel"""
    full = length >> 4
    rounds = -(-full // 1024)
    return full, length & 15, rounds, rounds * 1024 - full


# ---- (a) --------------------------------------------------------------------------------------------------------------------
TAIL_K = (1, 2, 4, 5, 8)


def _named_tails(kmax):
    """(length, the (groups, tail, rounds, lead) the family names it for), written out case by case"""
    out = [(n, (n // 16, n % 16, 0 if n < 16 else 1, 0 if n < 16 else 1024 - n // 16)) for n in range(49)]
    for k in TAIL_K:
        if k > kmax:
            continue
        for d in range(-17, 18):
            if k == 8 and d > 0:  # the 128 KB ceiling of the path
                continue
            if d == -17:
                t = (k * 1024 - 2, 15, k, 2)
            elif d < 0:
                t = (k * 1024 - 1, d + 16, k, 1)
            elif d < 16:
                t = (k * 1024, d, k, 0)
            else:
                t = (k * 1024 + 1, d - 16, k + 1, 1023)
            out.append((k * ROUND + d, t))
    return out


@functools.lru_cache(maxsize=None)
def frame_tails(kmax=8):
    rng = np.random.default_rng(101)
    named = _named_tails(kmax)
    for n, t in named:
        assert frame_geometry(n) == t, (n, t)
    seen = {t[1:] for _, t in named}
    for tail in range(16):
        assert (tail, 0, 0) in {(t[1], t[2], t[3]) for _, t in named if t[0] == 0}, tail       # no group
        assert any(t[0] == 1 and t[1] == tail for _, t in named), tail                           # one group
        assert (tail, 1, 0) in seen and (tail, 1, 1023) in seen, tail                            # a full round; 1023 in front
    if kmax >= 8:
        assert {t[2] for _, t in named} >= {0, 1, 2, 3, 4, 5, 6, 8}
        assert len(named) == 49 + 4 * 35 + 18 == 207 and max(n for n, _ in named) == 131072
    lens = [n for n, _ in named]
    return Batch(f"frame_tails k<={kmax}", max(lens), lens, [_rand(rng, n) for n in lens], 1, 0)


# ---- (b) --------------------------------------------------------------------------------------------------------------------
CONTENT_LENGTHS = (16, 20, 16384, 16400, 40000)


def _exchange_pairs(length):
    """{kind: (g, g')}: two whole groups of one frame that the one-workgroup kernel gives to two lanes of one wave, to the
    same lane of two waves, to one thread in two rounds"""
    full, _, _, lead = frame_geometry(length)
    where = lambda g: ((g + lead) // 1024, (g + lead) % 1024 // 64, (g + lead) % 64)  # noqa: E731  (round, wave, lane)
    out = {}
    for g in range(full):
        r, w, l = where(g)
        if "lanes" not in out and g + 1 < full and where(g + 1) == (r, w, l + 1):
            out["lanes"] = (g, g + 1)
        if "waves" not in out and g + 64 < full and where(g + 64) == (r, w + 1, l):
            out["waves"] = (g, g + 64)
        if "rounds" not in out and g + 1024 < full and where(g + 1024) == (r + 1, w, l):
            out["rounds"] = (g, g + 1024)
    return out


@functools.lru_cache(maxsize=None)
def frame_content():
    rng = np.random.default_rng(102)
    lens, frames, names = [], [], []

    def add(name, f):
        names.append(name)
        lens.append(len(f))
        frames.append(bytes(f))

    kinds = set()
    for n in CONTENT_LENGTHS:
        add(f"{n} zeros", bytes(n))
        add(f"{n} FF x 4 + zeros", b"\xff" * 4 + bytes(n - 4))
        add(f"{n} FF", b"\xff" * n)
        last_group = ((n >> 4) - 1) * 16
        at = sorted({0, 3, 4, 15, 16, n - 1, last_group} | {p for p in (ROUND - 1, ROUND) if p < n})
        assert all(0 <= p < n for p in at if p != 16) and {0, 3, 4, 15, n - 1, last_group} <= set(at)
        for p in (p for p in at if p < n):  # (byte 16 of a 16-byte frame does not exist)
            f = bytearray(n)
            f[p] = 1 << (p % 8)
            add(f"{n} bit at {p}", f)
        base = _rand(rng, n)
        add(f"{n} random", base)
        pairs = _exchange_pairs(n)
        for kind, (g, g2) in sorted(pairs.items()):
            f = bytearray(base)
            f[16 * g:16 * g + 16], f[16 * g2:16 * g2 + 16] = base[16 * g2:16 * g2 + 16], base[16 * g:16 * g + 16]
            assert bytes(f) != base and orc.crc32c(bytes(f)) != orc.crc32c(base), (n, kind)
            add(f"{n} exchanged across {kind}", f)
            kinds.add((n, kind))
    assert {k for n, k in kinds if n == 40000} == {"lanes", "waves", "rounds"} and (16400, "rounds") in kinds
    assert (16384, "waves") in kinds and not _exchange_pairs(16) and not _exchange_pairs(20)
    assert any(f[:4] == b"\xff" * 4 and not any(f[4:16]) for f in frames)  # the whole first group zero once folded
    b = Batch("frame_content", max(lens), lens, frames, 1, 0)
    b.names = names
    return b


# ---- (c) --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def error_and_empty():
    rng = np.random.default_rng(103)
    special = ERR + (0,)
    batches, placed = [], set()
    for k in range(4):
        first, middle, last = special[k], special[(k + 1) % 4], special[(k + 2) % 4]
        lens = [first, 1, 100, middle, 4097, 20000, last]
        placed |= {(first, "first"), (middle, "middle"), (last, "last")}
        frames = [None if l >= R.ERR_FROM else _rand(rng, l) for l in lens]
        batches.append(Batch(f"error_and_empty {k}", 20000, lens, frames, 1, 0))
    assert placed == {(s, p) for s in special for p in ("first", "middle", "last")}
    return tuple(batches)


# ---- (d) --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_frames():
    rng = np.random.default_rng(104)
    lens = [131073, 131088, 163840, 196607, 196608, 0xFFFFFFF7, 0, 5, 16, 4097, 65536, 131072]
    assert len(lens) == 12 and sum(1 for l in lens if 131072 < l < R.ERR_FROM) == 5
    assert {frame_geometry(l)[2] for l in lens if l < R.ERR_FROM} >= {0, 1, 4, 8, 9, 10, 12}
    return Batch("long_frames", 196608, lens, [None if l >= R.ERR_FROM else _rand(rng, l) for l in lens], 1, 0, tight_stride=True)


# ---- (e) --------------------------------------------------------------------------------------------------------------------
SPAN16 = 16384


@functools.lru_cache(maxsize=None)
def span_edges():
    rng = np.random.default_rng(105)
    max_len = 12 * SPAN16
    lens = [s * SPAN16 + d for s in (1, 2, 11, 12) for d in (-17, -16, -1, 0, 1, 15, 16, 17) if s * SPAN16 + d <= max_len]
    assert len(lens) == 28 and max_len in lens
    lens += [0, 1, 15, 0xFFFFFFF0, 100000]  # (100000: the filler that makes whole batches of three)
    assert len(lens) % 3 == 0
    for l in lens:  # a short frame leaves every later span empty
        if l < R.ERR_FROM:
            live = -(-l // SPAN16)
            assert 0 <= live <= 12
    assert {-(-l // SPAN16) for l in lens if l < R.ERR_FROM} >= {0, 1, 2, 3, 11, 12}
    frames = [None if l >= R.ERR_FROM else _rand(rng, l) for l in lens]
    out = tuple(Batch(f"span_edges {i // 3}", max_len, lens[i:i + 3], frames[i:i + 3], 12, 4, tight_stride=True)
                for i in range(0, len(lens), 3))
    assert all(any(l < R.ERR_FROM and l % 16 for l in b.lens) for b in out)  # a partial last group in every batch: (j)
    return out


# ---- (f) --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def span_batches():
    rng = np.random.default_rng(106)
    out = []
    for max_len, parts in ((1032192, 63), (1048576, 64), (1048577, 65)):
        assert -(-max_len // SPAN16) == parts
        lens = [max_len, 16385]  # the short frame: two live spans, every other one empty
        assert -(-16385 // SPAN16) == 2
        out.append(Batch(f"span_batches {parts}", max_len, lens, [_rand(rng, l) for l in lens], parts, 4, tight_stride=True))
    for max_len, parts, lens in ((2097152, 128, (0x155555, 0x1FFFFF, 2097152)), (2097168, 129, (2097168, 0x155555))):
        assert -(-max_len // SPAN16) == parts
        for l in lens:
            assert l == max_len or bin(l >> 16).count("1") >= 3  # several bits above 2^16
            out.append(Batch(f"span_batches {parts} len {l:#x}", max_len, [l], [_rand(rng, l)], parts, 4, tight_stride=True))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def span_batches_swapped():
    """the 63- and 64-register batches of (f) with other bytes and the short frame first: the second launch on a set of
    arrival counters"""
    rng = np.random.default_rng(116)
    out = []
    for b in span_batches()[:2]:
        lens = b.lens[::-1]
        out.append(Batch(b.name + " swapped", b.max_len, lens, [_rand(rng, l) for l in lens], b.parts, 4, tight_stride=True))
    return tuple(out)


# ---- (g) --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_spans():
    rng = np.random.default_rng(107)
    long_ones = [65535, 65536, 65537, 131072, 524287, 524288]
    lens = [int(v) for v in rng.integers(0, 65, 65)]
    lens[1], lens[63] = 64, 0
    for k, l in enumerate(long_ones):  # spread over the batch, the first and the last slot among them
        lens[k * 64 // 5] = l
    assert len(lens) == 65 and sorted(l for l in lens if l > 64) == long_ones and lens[0] == 65535 and lens[64] == 524288
    return Batch("wide_spans", 524288, lens, [_rand(rng, l) for l in lens], 8, 16, tight_stride=True)


# ---- (h) --------------------------------------------------------------------------------------------------------------------
LEN_BITS = (1 << 24) + 65536 + 19


@functools.lru_cache(maxsize=None)
def len_bits():
    rng = np.random.default_rng(108)
    assert [k for k in range(32) if LEN_BITS >> k & 1] == [0, 1, 4, 16, 24]
    f = bytearray(LEN_BITS)
    f[:4096] = _rand(rng, 4096)
    f[-4096:] = _rand(rng, 4096)
    f = bytes(f)
    assert -(-LEN_BITS // SPAN16) == 1029 and -(-LEN_BITS // 65536) == 258
    lone = Batch("len_bits lone", LEN_BITS, [LEN_BITS], [f], 1029, 4, tight_stride=True)
    pair = Batch("len_bits pair", LEN_BITS, [LEN_BITS, 19], [f, _rand(rng, 19)], 258, 16, tight_stride=True)
    lone.expect()
    e = lone._expect
    small = R.expect(pair.frames[1:], pair.lens[1:], pair.dims[1:])
    assert pair.dims[0] == lone.dims[0]  # the long frame's expectation serves both batches
    pair._expect = {k: np.concatenate([e[k], small[k]]) for k in e}
    return lone, pair


# ---- (i) --------------------------------------------------------------------------------------------------------------------
PACKET_LENGTHS = (0, 1, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, 0x80000000, 0xFFFFFFEF)
PACKET_DIMS = (0, 1, 65535, 0xFFFFFFFF, 80, 24)


@functools.lru_cache(maxsize=None)
def packets_only():
    """-> ((n, lens uint32[n], crcs uint32[n], dims uint32[n, 2]), ...)"""
    rng = np.random.default_rng(109)
    pool = PACKET_LENGTHS + ERR
    out = []
    for n in (1, 256, 257, 600):
        lens = np.array([pool[(i * 5 + n) % len(pool)] for i in range(n)], dtype=np.uint32)
        if n == 1:
            lens[0] = (1 << 24) + 1
        else:
            lens[n - 1] = 0xFFFFFFEF  # the last thread of the last block: the longest length there is
            assert set(int(v) for v in lens) == set(pool)
        if n > 256:
            assert any(int(v) >= 1 << 24 and int(v) < R.ERR_FROM for v in lens[256:])  # beyond one block, above 2^24
        crcs = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        dims = np.array([PACKET_DIMS[int(v)] for v in rng.integers(0, len(PACKET_DIMS), 2 * n)], dtype=np.uint32).reshape(n, 2)
        dims[0] = (0xFFFFFFFF, 65535)
        out.append((n, lens, crcs, dims))
    return tuple(out)


def packets_expect(case):
    n, lens, crcs, dims = case
    hdr, pkt = bytearray(), np.zeros(n, dtype=np.uint32)
    for i in range(n):
        h, p = R.packet_crc_from_frame_crc(int(dims[i][0]), int(dims[i][1]), int(lens[i]), int(crcs[i]))
        hdr += h
        pkt[i] = p
    return np.frombuffer(bytes(hdr), dtype=np.uint8), pkt


# ---- (j) --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def short_pack_batch():
    rng = np.random.default_rng(110)
    lens = [int(v) for v in rng.integers(0, 41, 1100)]
    lens[0], lens[1023], lens[1024], lens[1099] = 40, 17, 0, 33
    assert len(lens) > 1024 and max(lens) == 40 and min(lens) == 0
    return Batch("pack 1100 short", 40, lens, [_rand(rng, l) for l in lens], 1, 0)


def pack_batches():
    """the batches of (j), the 1100 short frames last"""
    return (frame_tails(2),) + error_and_empty() + span_edges() + (short_pack_batch(),)


def pack_capacities(batch):
    """[(what, capacity)]: exactly the total, one byte less, the exact end (not rounded to 16) of a frame with a partial
    last group -- the one nearest the middle of the packed bytes -- and 0"""
    off, _ = batch.packed()
    total = off[batch.n]
    ends = [off[i] + l for i, l in enumerate(batch.lens) if l < R.ERR_FROM and l % 16]
    assert ends and total > 16, batch
    exact = min(ends, key=lambda e: abs(e - total // 2))
    assert exact % 16 and 0 < exact < total
    return [("total", total), ("total - 1", total - 1), ("exact end", exact), ("zero", 0)]
