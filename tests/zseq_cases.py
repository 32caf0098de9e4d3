"""zseq wire form test support: the boundary families the restatement, the emulated and the GPU tests share -- every case asserts
its premise with the restatement (tests/zseq_ref.py) -- and tests/zwire.py's expectation, check and emulator run bound to the
sequence form.  TESTS ONLY."""
import functools

import numpy as np

import zhuf_ref as Z
import zpack_support as ZS
import zseq_ref as S
import zwide_support as WS
import zwire as ZW

FILL, ERR = ZS.FILL, ZS.ERR
SMALL = 512  # the second emulator library's ACHIP_ZSEQ_PIECE


# ---- inputs ------------------------------------------------------------------------------------------------------------
def rnd(n, seed):
    """n uniform bytes: no 4-byte match within 64 bytes but by a 2^-26 accident (the premises would catch it)"""
    return bytes(np.random.default_rng(1000 + seed).integers(0, 256, n, dtype=np.uint8))


def text(n, seed):
    """n bytes of a synthetic truecolor frame: compresses to about 0.45 in this form"""
    return (ZS.ansi_truecolor(40, 2 + n // 700, seed) * 2)[:n]


def run(unit, n):
    """n bytes that continue `unit` periodically BEHIND it: a match of distance len(unit)"""
    return (unit * (n // len(unit) + 2))[:n]


def units(spec, seed):
    """[(LL, ML, d)] -> bytes that parse into exactly these sequences: LL random bytes, then ML bytes that repeat the last d"""
    out = b""
    for k, (ll, ml, d) in enumerate(spec):
        assert d <= ll
        lit = rnd(ll, 50 * seed + k)
        out += lit + run(lit[-d:], ml)
    return out


def infos_of(frame, piece=S.PIECE):
    infos = []
    S.encode(frame, piece, infos)
    return infos


def _seqs(frame, piece=S.PIECE, block=0):
    return infos_of(frame, piece)[block]["seqs"]


def _sent_compressed(frame, piece):
    assert S.wire(frame, piece)[2] == Z.FLAG_COMPRESSED, "the case must travel compressed to be seen"
    return frame


def _exact_body(piece, delta):
    """a second block of n bytes with one sequence whose body is n - delta bytes: raw for 0, compressed for 1"""
    for ml in range(4, 40):
        lead = piece * max(1, -(-1100 // piece))
        f = text(lead, 31) + rnd(98, 32) + b"xy" + run(b"xy", ml)
        info = infos_of(f, piece)[lead // piece]
        n = len(f) - lead
        if len(info["seqs"]) == 1 and info["body"] == n - delta:
            assert info["kind"] == (2 if delta else 0)
            return f
    raise AssertionError("no block with that body")


def _exact_ratio(piece, short):
    """a frame whose zseq form is exactly 4/5 of it (sent as it is), or one byte of literals less (sent compressed)"""
    for a in range(1100, 2200):
        lit = rnd(a, 33)
        f = lit + run(lit[-8:], 400)
        z = S.encode(f, piece)
        if 5 * len(z) == 4 * len(f):
            g = f[1:] if short else f
            zg = S.encode(g, piece)
            assert (5 * len(zg) < 4 * len(g)) == bool(short) and len(g) > 1024 and len(g) <= piece
            return g
    raise AssertionError("no frame at the ratio")


_cases = {}


def cases(piece=S.PIECE):
    """name -> frame bytes (or an error code).  piece: the piece size the frames are built around; a piece below the product's
    gives the families of the block cuts only."""
    if piece in _cases:
        return _cases[piece]
    P = piece
    out = {"error code": ERR, "empty": b"", "another error code": 0xFFFFFFFF}

    def add(name, frame, premise, compressed=True):
        assert premise(infos_of(frame, P)), name
        out[name] = _sent_compressed(frame, P) if compressed else frame

    # block cuts (behind B whole blocks of text, so that the frame is above the size floor whatever the piece)
    B = max(1, -(-1100 // P))
    u = rnd(40, 400)
    f = text(B * P - 40, 401) + u + u + text(700, 402)
    add("a match back over the block cut", f, lambda i: len(i) >= 2 and i[B]["seqs"][0][0] == 0 and i[B]["seqs"][0][2] == 40 and i[B]["seqs"][0][1] >= 40)
    u = rnd(30, 410)
    f = text(B * P - 34, 411) + u + u[:4] + u[4:] + text(700, 412)
    add("a match cut to 4 by the block's end, no tail literals", f,
        lambda i: i[B - 1]["seqs"][-1][1:] == (4, 30) and i[B - 1]["tail"] == 0 and i[B]["seqs"][0] == (0, 26, 30))
    f = text(B * P - 33, 413) + u + u[:3] + u[3:] + text(700, 414)
    add("a match cut to 3 by the block's end: literals", f, lambda i: i[B - 1]["tail"] >= 3 and i[B]["seqs"][0] == (0, 27, 30))
    f = text(B * P, 420) + rnd(10, 421) + run(b"ab", 120)
    add("a block with one sequence", f, lambda i: i[B]["seqs"] == [(12, 118, 2)] and i[B]["kind"] == 2)
    f = text(B * P, 422) + rnd(300, 423)
    add("a block with no sequence (raw)", f, lambda i: i[B]["seqs"] == [] and i[B]["kind"] == 0)
    out["a body of n bytes (raw)"] = _sent_compressed(_exact_body(P, 0), P)
    out["a body of n - 1 bytes (compressed)"] = _sent_compressed(_exact_body(P, 1), P)
    u = rnd(8, 430)
    f = text(B * P - 8, 431) + u + run(u, 260)
    add("a block without literals", f, lambda i: i[B]["lits"] == b"" and i[B]["seqs"] == [(0, 130, 8), (0, 130, 8)])
    w = bytes(x if x != 0x61 else 0x62 for x in rnd(64, 440))
    f = text(B * P - 64, 441) + w + b"".join(b"aa" + w[6 * k + 2:6 * k + 6] for k in range(10))
    add("20 equal literals (raw literals)", f, lambda i: i[B]["lits"] == b"a" * 20 and len(i[B]["seqs"]) == 10 and i[B]["kind"] == 2 and not i[B]["huf"])
    for blocks in (B, B + 1, B + 2):
        f = text(blocks * P, 450 + blocks)
        add("exactly %d blocks" % blocks, f, lambda i, blocks=blocks: len(i) == blocks and all(x["kind"] == 2 for x in i))
    if P >= 8192:  # the families of one block: built for the product's piece size
        # match lengths at the minimum and at the cap; a run longer than the cap
        for k in (3, 4, 5, 129, 130, 131, 300):
            head = rnd(50, k)
            f = rnd(20, 100 + k) + head + run(head, k) + bytes([head[k % 50] ^ 0xFF]) + text(1200, k)
            want = {3: None, 4: (70, 4, 50), 5: (70, 5, 50), 129: (70, 129, 50), 130: (70, 130, 50), 131: (70, 130, 50), 300: (70, 130, 50)}[k]
            add("match of %d" % k, f, lambda i, want=want, k=k: (i[0]["seqs"][0] == want if want else i[0]["seqs"][0][0] > 73) and
                (k != 300 or i[0]["seqs"][1:3] == [(0, 130, 50), (0, 40, 50)]))
        # distances: 64 is coded, 65 is not
        for d in (1, 63, 64):
            f = rnd(70, 200 + d) + run(rnd(70, 200 + d)[-d:], 1000)
            add("period %d" % d, f, lambda i, d=d: i[0]["seqs"][0] == (70, 130, d) and all(s[2] == d for s in i[0]["seqs"]))
        f = run(rnd(65, 265), 1500)
        add("period 65 (no sequence)", f, lambda i: i[0]["seqs"] == [], compressed=False)
        # the window is cut by the frame's start; bytes as the emulator's LDS poison in front would match where the cut is ignored
        f = run(rnd(10, 300), 200) + text(1000, 301)
        add("a match at position 10 of the frame", f, lambda i: i[0]["seqs"][0] == (10, 130, 10))
        f = b"\xcd" * 5 + b"x" + b"\xcd" * 3 + rnd(7, 302) + text(1100, 303)
        add("0xCD at the frame's start", f, lambda i: i[0]["seqs"][0][0] >= 1 and i[0]["lits"][:1] == b"\xcd")
        f = b"ab" + b"cdefcdef" + text(1100, 304)
        add("a match at position 6 of the frame", f, lambda i: i[0]["seqs"][0] == (6, 4, 4))
        # every position 1 .. 63 of the frame as the first match, at the largest distance the cut allows there (d = i); the frame
        # starts with the emulator's LDS poison byte, so position 0 would match in front of the frame where the cut is ignored
        for i in range(1, 64):
            unit = (b"\xcd" + rnd(63, 310 + i))[:i]
            f = unit + run(unit, 150) + bytes([unit[150 % i] ^ 0xFF]) + text(1000, 305)
            add("the window cut at position %d" % i, f, lambda x, i=i: x[0]["seqs"][0] == (i, 130, i) and x[0]["seqs"][1][:2] == (0, 20))
        # the code tables' steps
        spec = [(ll, ml, 5) for ll in (15, 16, 17, 63, 64) for ml in (34, 35, 36)] + [(24, 130, 7), (32, 99, 9), (48, 98, 11), (64, 67, 64)]
        f = units(spec, 5)
        add("LL and ML at the code tables' steps", f, lambda i: i[0]["seqs"] == spec)
        for count in (127, 128):
            f = units([(4, 8, 4)] * count, 6 + count)
            add("%d sequences" % count, f, lambda i, count=count: len(i[0]["seqs"]) == count)
        # literal counts at the raw header's steps and at MIN_HUF
        for nlit in (16, 17):
            f = units([(8, 520, 8), (8, 520, 8)], 20 + nlit) + rnd(nlit - 16, 21)
            add("%d literals" % nlit, f, lambda i, nlit=nlit: len(i[0]["lits"]) == nlit and not i[0]["huf"])
        for nlit in (31, 32):
            f = units([(nlit, 1040, 8)], 30 + nlit)
            add("%d literals" % nlit, f, lambda i, nlit=nlit: len(i[0]["lits"]) == nlit and len(i[0]["lit_section"]) == nlit + (1 if nlit < 32 else 2))
        for nlit in (4095, 4096):
            f = units([(nlit, 3900, 8)], 40 + nlit % 10)
            add("%d literals" % nlit, f, lambda i, nlit=nlit: len(i[0]["lits"]) == nlit and len(i[0]["lit_section"]) == nlit + (2 if nlit < 4096 else 3))
        # the literals' trees
        f = ZS.ansi_truecolor(20, 6, 13)
        add("truecolor 20x6 (direct tree)", f, lambda i: i[0]["huf"] and max(i[0]["lits"]) <= 0x80 and i[0]["lit_section"][2 + ((i[0]["lit_section"][0] >> 2) & 3)] >= 128)
        f = WS.utf8_truecolor(20, 6, 17)
        add("utf-8 palette truecolor 20x6 (FSE tree)", f, lambda i: i[0]["huf"] and max(i[0]["lits"]) > 0x80 and i[0]["lit_section"][2 + ((i[0]["lit_section"][0] >> 2) & 3)] < 128)
        f = WS.halfblock_truecolor(20, 6, 16)
        add("half-block truecolor 20x6", f, lambda i: i[0]["huf"] and len(i[0]["seqs"]) > 200)
        # the frame rule
        out["5 zlen = 4 len (as it is)"] = _exact_ratio(P, 0)
        out["5 zlen = 4 len - 1 (compressed)"] = _exact_ratio(P, 1)
        lit = rnd(20, 460)
        f = lit + run(lit[-8:], 1004)
        add("1024 bytes (as it is: the size floor)", f, lambda i: i[0]["kind"] == 2 and len(f) == 1024, compressed=False)
        assert S.wire(f, P)[2] == 0
        add("1025 bytes", f + f[-8:-7], lambda i: i[0]["kind"] == 2)
        out["one byte value (RLE)"] = b"\xe2" * 2000
        out["uniform bytes (as it is)"] = rnd(3000, 461)
        out["1 byte"] = b"x"
        out["5 bytes"] = b"ababa"
    _cases[piece] = out
    return out


# ---- the shared expectation, check and emulator run (tests/zwire.py), bound to the sequence form ----------------------------
FORM = ZW.SEQ
expect, check, emulator, emu_run = (functools.partial(f, FORM) for f in (ZW.expect, ZW.check, ZW.emulator, ZW.emu_run))
