"""Cases of the zhuf wire pass at its block, stream and batch boundaries.  Deterministic; the emulated tests
(test_zpack_boundaries.py) and the GPU tests (test_gpu_zpack.py) import it.  Every family asserts its own premise with the
restatement (tests/zhuf_ref.py): block type, Size_Format, equality, phase -- a case cannot silently stop being a boundary
case, and none is skipped or filtered out when the tests run.  TESTS ONLY.

What a piece does at a boundary shows only inside a frame that is sent compressed, and a Huffman block below 1024 bytes
exists only behind another piece.  So the per-piece families (a) to (d) are carrier + tail: a full first piece that
compresses to an eighth, then the piece under test.  They take the piece size as a parameter: the emulated tests run them at
2048 bytes a piece (a second emulator library), the GPU tests at the product's 131072.

  (a) tail_lengths       tails of 1 .. 65 bytes round the 16-byte groups and MIN_HUF, and of 1023 / 1024 / 16383 / 16384
                         bytes, where Size_Format goes 1 / 2 / 2 / 3
  (b) tail_gain          tails whose compressed block is exactly as long as the piece (sent raw) and one byte shorter (sent
                         compressed), and the smallest block there is: 17 bytes of 00 / 01 -> 16
  (c) tail_symbols       the largest symbol 1, 2, 3, 127, 128; two, three and 129 distinct symbols; symbol 0
  (d) tail_phases        the tail block starts at every phase of a 16-byte group (Huffman), at 0 / 1 / 8 / 15 (raw, RLE);
                         three pieces Huffman / raw / Huffman
  (e) ratio_frames       5 * zlen == 4 * len exactly and a byte either side; 1024 / 1025 bytes
  (f) stream_cut_frames  every length 1280 .. 1343: the three stream cuts at every position within a 16-byte group
  (g) chunk_step_frames  streams of 1009 .. 1040 and 2041 .. 2056 symbols: a lane's share steps from 16 to 32 (32 to 48)
                         symbols where the stream, counted from the start of its first 16-byte group, passes 1024 (2048)
  (h) histograms         254 histograms for the length algorithm, each a frame of at most 8 KB
  (i) short_batch, piece_batch   more than 256 frames; empty frames, error codes and frames of whole pieces among
                         multi-piece frames

Not here: offsets above 4 GB (ZF_OFF_HI) -- a test would have to move more than 4 GB; lengths above max_len (the caller's
contract).

(b) above 1024 bytes: there is no such tail.  An optimal code of at most 129 symbols costs at most (127 * 7 + 2 * 8) / 129
< 7.02 bits a symbol (the fixed 7 / 8-bit code, its two long codes on the two rarest symbols, costs no more than that and no
Huffman code costs more than it), and where the limiter runs the tree was deeper than 11, which takes counts as steep as
Fibonacci's, far below that.  With at most 80 bytes of headers, tree and stream ends, 7.02 / 8 * n + 80 >= n - 1 ends near
n = 650.  The search that found the cases below found none above 414 bytes.
"""
import numpy as np

import zhuf_ref as Z
from zpack_support import ERR, ansi_truecolor, skewed, uniform7

SMALL_PIECE = 2048  # the second emulator library's ACHIP_ZPACK_PIECE
A, B, C_ = 0x41, 0x42, 0x43


# ---- carrier + tail ----------------------------------------------------------------------------------------------------
def carrier(piece, k=0):
    """a full piece of three symbols (code lengths 1 / 2 / 2 whatever the counts): `A` everywhere but for 2 + 8 k of the
    rarer two at its start, all in stream 0 -- whose bytes, and the block's, grow by one per k"""
    assert 0 <= k < 16 and 2 + 8 * 15 < piece // 4
    a = np.full(piece, A, dtype=np.uint8)
    a[0:2 + 8 * k:2] = B
    a[1:2 + 8 * k:2] = C_
    return a.tobytes()


def tail_block(frame, piece):
    """-> (type, size, offset in the zhuf frame, Size_Format or 0) of the frame's last block, the frame being one that is
    sent compressed"""
    assert Z.wire(frame, piece)[2] == Z.FLAG_COMPRESSED
    z = Z.encode(frame, piece=piece)
    kind, size, at = Z.blocks(z)[-1]
    return kind, size, at, ((z[at + 3] >> 2) & 3) if kind == 2 else 0


def _on(piece, tail, k=0):
    assert 0 < len(tail) <= piece
    return carrier(piece, k) + tail


HUF_FROM = 17  # the tails are coded from MIN_HUF up: two small symbols, a tree of two bytes (asserted below)
TAIL_LENGTHS = (1, 2, 15, 16, 17, 18, 31, 32, 33, 63, 64, 65, 1023, 1024)
TAIL_LENGTHS_LONG = ((16383, 2), (16384, 3))


def _length_tail(n):
    return skewed(n, 200 + n, spread=0.6, base=0, top=1) if n < 1023 else skewed(n, 200 + n)


def tail_lengths(piece):
    """(a), the lengths that fit a piece of SMALL_PIECE"""
    out = []
    for n in TAIL_LENGTHS:
        f = _on(piece, _length_tail(n))
        kind, _, _, fmt = tail_block(f, piece)
        body = Z.huf_block_body(_length_tail(n))
        assert (kind == 2) == (body is not None) == (n >= HUF_FROM), (n, kind)
        if n >= 1023:
            assert fmt == {1023: 1, 1024: 2}[n]
        out.append((f"tail of {n}", f))
    return out


def tail_lengths_long(piece=Z.PIECE):
    """(a), 16383 and 16384: the product's piece size only"""
    out = []
    for n, want in TAIL_LENGTHS_LONG:
        f = _on(piece, _length_tail(n))
        assert tail_block(f, piece)[3] == want
        out.append((f"tail of {n}", f))
    return out


# found by search with the restatement: (n, seed, spread, top) of skewed(n, seed, spread, 0, top)
GAIN_EQUAL = ((21, 1, 0.35, 6), (23, 4, 0.35, 6), (395, 1, 0.02, 128), (404, 5, 0.02, 128))
GAIN_ONE = ((22, 1, 0.35, 6), (24, 3, 0.35, 6), (400, 1, 0.02, 128), (414, 5, 0.02, 128))
SMALLEST = b"\x00" * 9 + b"\x01" + b"\x00" * 7  # 17 bytes -> a block of 16: 3 + (1 + 1) + 6 + 4 streams of 1 + 1


def tail_gain(piece):
    """(b)"""
    out = []
    for n, seed, spread, top in GAIN_EQUAL:
        t = skewed(n, seed, spread=spread, base=0, top=top)
        f = _on(piece, t)
        assert len(Z.huf_block_candidate(t)) == n and tail_block(f, piece)[:2] == (0, n)  # blk == n: raw
        out.append((f"block as long as its piece of {n}", f))
    for n, seed, spread, top in GAIN_ONE:
        f = _on(piece, skewed(n, seed, spread=spread, base=0, top=top))
        assert tail_block(f, piece)[:2] == (2, n - 1)  # blk == n - 1: compressed
        out.append((f"block one byte below its piece of {n}", f))
    f = _on(piece, SMALLEST)
    assert tail_block(f, piece)[:2] == (2, 16) and max(SMALLEST) == 1 and min(SMALLEST) == 0
    out.append(("the smallest block: 17 bytes of 00 / 01", f))
    return out


def _symbols_tail(values, n, seed):
    """n bytes over `values`, geometric counts in that order"""
    r = np.random.default_rng(seed)
    v = np.array(values, dtype=np.uint8)
    return v[np.minimum(r.geometric(0.4 if len(values) < 20 else 0.06, n) - 1, len(values) - 1)].tobytes()


def tail_symbols(piece):
    """(c): name -> (values, length)"""
    kinds = [("top 1: 00 01", [0, 1], 300), ("top 2, three symbols with 0", [1, 0, 2], 300), ("top 2, two symbols", [2, 1], 301),
             ("top 3", [0, 3, 1, 2], 302), ("top 3, two symbols with 0", [3, 0], 303), ("top 127", [127, 5, 126, 0], 304),
             ("top 127, two symbols", [64, 127], 299), ("top 128", [128, 7, 127], 298), ("top 128, two symbols with 0", [0, 128], 297),
             ("129 symbols", list(range(128, -1, -1)), 1500)]
    out = []
    for name, values, n in kinds:
        t = _symbols_tail(values, n, 300 + n)
        if len(values) == 129:
            t = bytes(range(129)) + t[129:]
        assert len(set(t)) == len(values) and max(t) == max(values) and (0 in t) == (0 in values)
        f = _on(piece, t)
        assert tail_block(f, piece)[0] == 2, name
        out.append((name, f))
    tops = {max(v) for _, v, _ in kinds}
    assert {1, 2, 3, 127, 128} <= tops and {2, 3, 129} <= {len(v) for _, v, _ in kinds}
    return out


RAW_TAIL = uniform7(99, 41) + b"\x90"  # a byte above 0x80: never coded
RLE_TAIL = b"z" * 37


def tail_phases(piece):
    """(d): the tail block's header at phase (offset in the zhuf frame) & 15"""
    out, seen = [], {0: set(), 1: set(), 2: set()}
    by_phase = {}
    for k in range(16):
        f = _on(piece, skewed(200 + k, 400 + k), k)
        kind, _, at, _ = tail_block(f, piece)
        assert kind == 2
        seen[2].add(at & 15)
        by_phase[at & 15] = k
        out.append((f"Huffman tail at phase {at & 15}", f))
    assert seen[2] == set(range(16))
    for name, t, want in (("raw", RAW_TAIL, 0), ("RLE", RLE_TAIL, 1)):
        for phase in (0, 1, 8, 15):
            f = _on(piece, t, by_phase[phase])
            kind, _, at, _ = tail_block(f, piece)
            assert kind == want and at & 15 == phase
            seen[want].add(phase)
            out.append((f"{name} tail at phase {phase}", f))
    f = carrier(piece, 3) + bytes(np.random.default_rng(42).integers(0, 256, piece, dtype=np.uint8)) + skewed(777, 43)
    assert Z.wire(f, piece)[2] == Z.FLAG_COMPRESSED
    assert [b[0] for b in Z.blocks(Z.encode(f, piece=piece))] == [2, 0, 2]
    out.append(("three pieces: Huffman, raw, Huffman", f))
    return out


def one_per_tail_kind(piece=Z.PIECE):
    """one carrier + tail per tail kind (Huffman, raw, RLE), each at a phase that is not 0"""
    out = []
    for name, t, want in (("Huffman", skewed(205, 405), 2), ("raw", RAW_TAIL, 0), ("RLE", RLE_TAIL, 1)):
        f = _on(piece, t, 5)
        kind, _, at, _ = tail_block(f, piece)
        assert kind == want and at & 15
        out.append((f"{name} tail", f))
    return out


# ---- whole frames ------------------------------------------------------------------------------------------------------
RATIO_EQUAL = ((0, 3340), (1, 3320), (2, 3340))  # found by search: skewed(1200, s, 0.7) + uniform7(4000, 100 + s)[:k]


def ratio_frames():
    """(e)"""
    out = []
    for s, k in RATIO_EQUAL:
        base, pad = skewed(1200, s, spread=0.7), uniform7(4000, 100 + s)
        flags = []
        for d in (-1, 0, 1):
            f = base + pad[:k + d]
            z = Z.encode(f)
            flags.append(Z.wire(f)[2])
            if d == 0:
                assert 5 * len(z) == 4 * len(f) and Z.wire(f) == (f, 0, 0)  # equality: as it is
            out.append((f"ratio {s}: {len(f)} bytes, zhuf {len(z)}", f))
        assert Z.FLAG_COMPRESSED in flags and 0 in flags
    for n in (1024, 1025):
        f = skewed(n, 500 + n)
        assert (Z.wire(f)[2] == Z.FLAG_COMPRESSED) == (n == 1025)
        out.append((f"{n} skewed", f))
    return out


def _spans(n):
    """s1 - b0 of the four streams of a piece of n bytes: what encode_stream shares out over the lanes"""
    seg = (n + 3) // 4
    return [min(n, (w + 1) * seg) - (w * seg & ~15) for w in range(4)]


def stream_cut_frames():
    """(f)"""
    out = []
    for n in range(1280, 1344):
        f = skewed(n, 600 + n)
        assert Z.wire(f)[2] == Z.FLAG_COMPRESSED
        out.append((f"{n} bytes", f))
    segs = {(n + 3) // 4 % 16 for n in range(1280, 1344)}
    assert segs == set(range(16)) and {n % 4 for n in range(1280, 1344)} == {0, 1, 2, 3}
    return out


def chunk_step_frames():
    """(g)"""
    out, spans = [], set()
    for segs, rs in ((range(1009, 1041), (0, 1, 2, 3)), (range(2041, 2057), (0, 3))):
        for seg in segs:
            for r in rs:
                n = 4 * seg - r
                assert (n + 3) // 4 == seg
                f = skewed(n, 700 + n, spread=0.3)
                assert Z.wire(f)[2] == Z.FLAG_COMPRESSED
                spans.update(_spans(n))
                out.append((f"{n} bytes: streams of {seg}", f))
    assert {1023, 1024, 1025, 2047, 2048, 2049} <= spans
    return out


# ---- histograms --------------------------------------------------------------------------------------------------------
HIST_LIMIT = 8192


def _scaled(counts):
    """the counts brought down to HIST_LIMIT in all, none below 1"""
    total = sum(counts)
    if total <= HIST_LIMIT:
        return list(counts)
    out = [max(1, c * (HIST_LIMIT - len(counts)) // total) for c in counts]
    assert sum(out) <= HIST_LIMIT
    return out


def _fib(m):
    f = [1, 1]
    while len(f) < m:
        f.append(f[-1] + f[-2])
    return f[:m]


def histogram_counts():
    """(h): [(name, counts)], counts of m symbols before they are given values"""
    out = []
    for m in range(12, 41):
        out.append((f"powers of two, {m}", _scaled([1 << k for k in range(m)])))
        out.append((f"powers of two x 3, {m}", _scaled([3 << k for k in range(m)])))
        out.append((f"Fibonacci, {m}", _scaled(_fib(m))))
    for m in (2, 3, 64, 127, 128, 129):
        out.append((f"equal counts, {m}", [HIST_LIMIT // m] * m))
    for m in (2, 3, 4, 5, 9, 17, 33, 64, 65, 100, 128, 129):
        out.append((f"one dominant symbol and {m - 1} singletons", [1] * (m - 1) + [3000]))
    out.append(("129 symbols, geometric", _scaled([max(1, int(4000 * 0.9 ** k)) for k in range(129)])))
    r = np.random.default_rng(77)
    for k in range(150):
        m = int(r.integers(2, 130))
        style = k % 3
        if style == 0:  # few distinct values: ties everywhere
            c = r.choice([1, 1, 2, 3, 5, 8, 40], m)
        elif style == 1:  # steep, with ties: the limiter
            c = 1 << r.integers(0, 13, m)
        else:
            c = np.minimum(r.geometric(0.02, m), 300)
        out.append((f"random {k}: {m} symbols", _scaled([int(x) for x in c])))
    return out


def histograms():
    """(h): [(name, hist[129], frame)]: symbol values drawn from 0 .. 128, the bytes shuffled"""
    out, steps, demoted, promoted = [], {}, [], []
    for k, (name, counts) in enumerate(histogram_counts()):
        r = np.random.default_rng(1000 + k)
        values = r.permutation(129)[:len(counts)] if len(counts) < 129 else r.permutation(129)
        hist = [0] * 129
        for v, c in zip(values, counts):
            hist[int(v)] = int(c)
        a = np.repeat(np.arange(129, dtype=np.uint8), hist)
        r.shuffle(a)
        assert 17 <= len(a) <= HIST_LIMIT
        Z.code_lengths(hist, steps)
        demoted.append(steps["demoted"])
        promoted.append(steps["promoted"])
        out.append((name, hist, a.tobytes()))
    assert len(out) >= 200 and max(demoted) > 1 and max(promoted) > 0
    return out


# ---- batches -----------------------------------------------------------------------------------------------------------
def short_batch(n):
    """(i): n short frames -- as they are, zhuf, empty, error codes with the threshold 0xFFFFFFF0 itself and 0xFFFFFFFF"""
    pool = [skewed(1025, 3), b"", 0xFFFFFFF0, skewed(700, 4), ansi_truecolor(20, 6, 13), 0xFFFFFFFF, uniform7(2000, 12), b"a" * 2000,
            skewed(5, 1), ERR, skewed(1300, 5), b"x"]
    frames = [pool[(i * 7 + i // len(pool)) % len(pool)] for i in range(n - 1)] + [pool[10]]  # (the last one is sent compressed)
    assert {0xFFFFFFF0, 0xFFFFFFFF, b""} <= set(frames) and len(set(frames)) == len(pool)
    return frames


def capacity_inside(frames, dims, first, expect, piece=Z.PIECE, plus=5):
    """-> (i, capacity): the capacity ends `plus` bytes into the first frame at or behind index `first` that is sent with
    more than a group behind that"""
    exp, _ = expect(frames, dims, piece)
    i = next(i for i in range(first, len(frames)) if exp[i]["sent"] > plus + 16)
    return i, exp[i]["off"] + plus


def piece_batch(piece):
    """(i): short frames, an empty one and an error code among frames of whole pieces; frame 4 is the first of more than one
    piece"""
    frames = [b"", ERR, skewed(5, 1), skewed(piece, 50), skewed(2 * piece + 17, 51, spread=0.3), skewed(piece + 1, 52), skewed(2 * piece, 53)]
    assert [len(f) for f in frames[3:]] == [piece, 2 * piece + 17, piece + 1, 2 * piece]
    for f in frames[3:]:
        assert Z.wire(f, piece)[2] == Z.FLAG_COMPRESSED
    assert [b[0] for b in Z.blocks(Z.encode(frames[4], piece=piece))][:2] == [2, 2]
    return frames


def piece_batch_capacities(frames, dims, expect, piece):
    """capacities that end inside frame 4's first block and inside its second"""
    exp, total = expect(frames, dims, piece)
    b = Z.blocks(exp[4]["payload"])
    caps = [exp[4]["off"] + b[0][2] + 3 + b[0][1] // 2, exp[4]["off"] + b[1][2] + 3 + b[1][1] // 2]
    assert exp[4]["off"] < caps[0] < exp[4]["off"] + b[1][2] < caps[1] < exp[4]["off"] + b[2][2] < total
    return caps
