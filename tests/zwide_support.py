"""Wide zhuf form test support: the cases the restatement, the emulated and the GPU tests share, tests/zwire.py's expectation,
check and emulator run bound to the wide form, and the check of the scratch records against the restatement
(tests/zwide_ref.py).  TESTS ONLY."""
import functools

import numpy as np

import zhuf_ref as Z
import zpack_support as ZS
import zwide_ref as W
import zwire as ZW

FILL, ERR = ZS.FILL, ZS.ERR
HALF = "▀".encode()  # E2 96 80


# ---- inputs ------------------------------------------------------------------------------------------------------------
def from_lengths(lens, seed, least=2048):
    """a piece whose symbols get exactly these code lengths: dyadic counts 2^(K - length), shuffled; at least `least` bytes"""
    assert sum(2.0 ** -d for d in lens.values()) == 1.0
    k = max(lens.values())
    while sum(1 << (k - d) for d in lens.values()) < least:
        k += 1
    a = np.concatenate([np.full(1 << (k - d), s, dtype=np.uint8) for s, d in sorted(lens.items())])
    np.random.default_rng(seed).shuffle(a)
    return bytes(a)


def zero_run(z, top=0xE2, max_bits=11):
    """a piece whose table description skips z absent weight values in one run (z = 0: none at all): weights 1 and
    z + 2 .. max_bits present, weight 0 too (symbols below `top` are absent)"""
    a = z + 2
    syms = list(range(0x20, 0x20 + (1 << (a - 1)))) + [top - k for k in range(max_bits - a + 1)]
    assert len(set(syms)) == len(syms)
    lens = {s: max_bits for s in syms[:1 << (a - 1)]}
    for k, w in enumerate(range(max_bits, a - 1, -1)):  # (the weight of `top` is not listed: it takes the last value)
        lens[top - k] = max_bits + 1 - w
    return from_lengths(lens, 40 + z)


def skewed_high(n, seed, top=0xFF, spread=0.3, symbols=None):
    """n bytes with a geometric histogram over `symbols` distinct values ending at `top`"""
    r = np.random.default_rng(seed)
    m = top + 1 if symbols is None else symbols
    order = r.permutation(top)[:m - 1]
    pal = np.concatenate([[top], order]).astype(np.uint8)
    idx = np.minimum(r.geometric(spread, n) - 1, m - 1)
    idx[:m] = np.arange(m)  # every symbol is there
    r.shuffle(idx)
    return bytes(pal[idx])


def halfblock_truecolor(w, h, seed):
    """a synthetic truecolor half-block frame: ESC[38;2;..m ESC[48;2;..m + E2 96 80 per cell"""
    r = np.random.default_rng(seed)
    rows = []
    for _ in range(h):
        rows.append("".join("\x1b[38;2;%d;%d;%dm\x1b[48;2;%d;%d;%dm▀" % tuple(r.integers(0, 256, 6)) for _ in range(w)))
    return ("\x1b[0m\n".join(rows) + "\x1b[0m").encode()


def utf8_truecolor(w, h, seed, palette=" ░▒▓█"):
    """a synthetic truecolor-foreground frame over a palette of multi-byte glyphs"""
    r = np.random.default_rng(seed)
    rows = []
    for _ in range(h):
        rows.append("".join("\x1b[38;2;%d;%d;%dm%s" % (*r.integers(0, 256, 3), palette[int(r.integers(0, len(palette)))]) for _ in range(w)))
    return ("\x1b[0m\n".join(rows) + "\x1b[0m").encode()


def info_of(piece):
    """what the restatement's encoder met in one piece: form, dec, add, runs, bits, tree; "coded": the block gains"""
    info = {}
    body = W.huf_block_body(piece, None, info)
    info["coded"] = body is not None
    return info


def _search(make, want, what, tries=400):
    for seed in range(tries):
        f = make(seed)
        if want(info_of(f)):
            return f
    raise AssertionError("no piece with " + what)


def stream_bits(residue):
    """a piece whose weights' FSE bitstream holds residue (mod 8) bits before its end mark"""
    return _search(lambda s: skewed_high(1500 + 7 * s, 300 + s, top=0x90 + s % 100, symbols=20 + s % 90),
                   lambda i: i["coded"] and i["form"] == "fse" and i["bits"] % 8 == residue, "%d bits mod 8" % residue)


def csize_of(body):
    fmt = (body[0] >> 2) & 3
    return (int.from_bytes(body[:2 + fmt], "little") >> 4) >> {1: 10, 2: 14, 3: 18}[fmt]


def with_csize(target):
    """a piece with a byte above 0x80 whose literals section is exactly `target` bytes: a prefix of one skewed stream"""
    for seed in range(80, 90):
        stream = skewed_high(4 * target, seed, top=0xE2, symbols=40, spread=0.35)
        n = 2 * target
        for _ in range(8):
            n = max(64, min(len(stream), n * target // csize_of(W.huf_block_candidate(stream[:n]))))
        for k in range(max(64, n - 40), min(len(stream), n + 40)):
            if csize_of(W.huf_block_candidate(stream[:k])) == target:
                return stream[:k]
    raise AssertionError("no piece of that compressed size")


_cases = None


def wide_cases():
    """name -> frame bytes (or an error code): the families of the wide form; every one of them is a single piece"""
    global _cases
    if _cases is not None:
        return _cases
    r = np.random.default_rng(77)
    out = {
        "error code": ERR,
        "empty": b"",
        "top 128 (direct form)": ZS.skewed(2500, 10) + b"\x80" * 3,
        "top 129 (odd count of weights)": ZS.skewed(2500, 11) + b"\x81" * 3,
        "top 130 (even count)": ZS.skewed(2500, 12) + b"\x82" * 5,
        "top 254": skewed_high(3000, 13, top=254, symbols=60),
        "top 255": skewed_high(3000, 14, top=255, symbols=61),
        "two symbols, one above 0x80": bytes(r.integers(0, 2, 3000, dtype=np.uint8) * 0xA1 + 0x41),
        "all 256 symbols skewed": skewed_high(6000, 15, spread=0.08),
        "256 equal counts (raw)": bytes(r.permutation(np.repeat(np.arange(256, dtype=np.uint8), 8))),
        "uniform bytes (raw by size)": bytes(r.integers(0, 256, 3000, dtype=np.uint8)),
        "one byte value above 0x80 (RLE)": b"\xe2" * 2000,
        "half blocks below the size floor (as it is)": (HALF * 340)[:1020],
        "half-block truecolor 20x6": halfblock_truecolor(20, 6, 16),
        "utf-8 palette truecolor 20x6": utf8_truecolor(20, 6, 17),
        "another error code": 0xFFFFFFFF,
        "bitstream of 0 bits mod 8": stream_bits(0),
        "bitstream of 7 bits mod 8": stream_bits(7),
        "csize 1023": with_csize(1023),
        "csize 1024": with_csize(1024),
    }
    for z in (0, 1, 2, 3, 4, 6):
        out["zero run of %d weight values" % z] = zero_run(z)
    out["normalisation decrements"] = zero_run(5, top=0xF0)  # three lone weight values rounded up to 1: 66 cells asked for
    # all 256 symbols: one at length 1, 50 / 107 / 98 at lengths 8 / 9 / 10 -- the floors of 64 c / 255 come to 63
    lens = {0x20: 1}
    rest = [x for x in range(256) if x != 0x20]
    lens.update({x: 8 for x in rest[:50]})
    lens.update({x: 9 for x in rest[50:157]})
    lens.update({x: 10 for x in rest[157:]})
    out["normalisation adds"] = from_lengths(lens, 61)
    _cases = out
    return out


# ---- the shared expectation, check and emulator run (tests/zwire.py), bound to the wide form --------------------------------
FORM = ZW.WIDE
wire_of, expect, check, emu_run = (functools.partial(f, FORM) for f in (ZW.wire_of, ZW.expect, ZW.check, ZW.emu_run))


# ---- the wide scratch records (csrc/zpack.h) -----------------------------------------------------------------------------
REC_WORDS, ZR_KIND, ZR_MAXBITS, ZR_TABLE, ZWR_TREELEN, ZWR_TREE = ZW.WIDE_REC_WORDS, 0, 8, 16, 272, 276


def device_record(out, i, p=0):
    """-> (block type, 256 words code | length << 16, maxBits, tree bytes of the FSE form) measure left for piece p of frame i"""
    rec = out["scratch"][(i * out["pieces"] + p) * REC_WORDS:][:REC_WORDS]
    tree = rec[ZWR_TREE:ZWR_TREE + 32].tobytes()[:int(rec[ZWR_TREELEN])] if int(rec[ZR_KIND]) == 2 else b""
    return int(rec[ZR_KIND]), [int(x) for x in rec[ZR_TABLE:ZR_TABLE + 256]], int(rec[ZR_MAXBITS]), tree


def check_records(frames, out, piece=W.PIECE):
    """every coded piece's table and tree in the scratch records against the restatement's"""
    coded = 0
    for i, f in enumerate(frames):
        if isinstance(f, int):
            continue
        for p in range(max(1, -(-len(f) // piece))):
            part = f[p * piece:(p + 1) * piece]
            kind, table, dev_bits, tree = device_record(out, i, p)
            t, info = [], {}
            body = W.huf_block_body(part, t, info)
            assert (kind == 2) == (body is not None), (i, p, kind)
            if body is None:
                continue
            coded += 1
            codes, max_bits = Z.canonical_codes(t[0])
            assert dev_bits == max_bits and table == [c | (d << 16) if d else 0 for c, d in zip(codes, t[0])], (i, p)
            if info["form"] == "fse":
                hl = 2 + ((body[0] >> 2) & 3)
                assert tree == body[hl:hl + 1 + body[hl]], (i, p, tree.hex())
    return coded
