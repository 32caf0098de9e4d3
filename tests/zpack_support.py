"""zhuf wire pass test support: the cases the restatement, the emulated and the GPU tests share, and tests/zwire.py's
expectation, check and emulator run bound to the narrow form.  TESTS ONLY."""
import functools

import numpy as np

import orc
import zwire as ZW

FILL, ERR = ZW.FILL, ZW.ERR


# ---- inputs ------------------------------------------------------------------------------------------------------------
def skewed(n, seed, spread=0.5, base=0x30, top=0x50):
    """n bytes below 0x80 with a geometric histogram"""
    r = np.random.default_rng(seed)
    return bytes(np.minimum(r.geometric(spread, n) - 1 + base, top).astype(np.uint8))


def uniform7(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 128, n, dtype=np.uint8))


def fibonacci():
    """20 symbols with Fibonacci counts, shuffled: unlimited Huffman depth 19"""
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    a = np.concatenate([np.full(c, s + 1, dtype=np.uint8) for s, c in enumerate(fib)])
    np.random.default_rng(5).shuffle(a)
    return bytes(a)


def ansi_truecolor(w, h, seed):
    """a synthetic truecolor-foreground frame: ESC[38;2;R;G;Bm + glyph per cell"""
    r = np.random.default_rng(seed)
    pal = orc.PALETTE_STANDARD
    rows = []
    for _ in range(h):
        rows.append("".join("\x1b[38;2;%d;%d;%dm%s" % (*r.integers(0, 256, 3), pal[int(r.integers(0, len(pal)))]) for _ in range(w)))
    return ("\x1b[0m\n".join(rows) + "\x1b[0m").encode()


def small_cases():
    """name -> frame bytes (or an error code): what the emulated and the GPU batch run"""
    every = bytes(range(129)) * 6 + skewed(3000, 11)
    out = {
        "error code": ERR,
        "empty": b"",
        "1 byte": b"x",
        "5 bytes": skewed(5, 1),
        "1024 skewed (as it is: the size floor)": skewed(1024, 2),
        "1025 skewed": skewed(1025, 3),
        "1026 skewed": skewed(1026, 4),
        "1027 skewed": skewed(1027, 5),
        "1028 skewed": skewed(1028, 6),
        "one byte value (RLE)": b"a" * 2000,
        "two byte values": bytes(np.random.default_rng(7).integers(0, 2, 3000, dtype=np.uint8) * 5 + 0x41),
        "fibonacci counts (limiter and repair)": fibonacci(),
        "all 129 symbols": every,
        "0x81 present (raw)": skewed(2000, 8) + b"\x81" + skewed(100, 9),
        "S = 128": skewed(2500, 10) + b"\x80" * 3,
        "uniform below 0x80 (as it is: the ratio)": uniform7(2000, 12),
        "another error code": 0xFFFFFFFF,
        "truecolor 20x6": ansi_truecolor(20, 6, 13),
        "17 bytes": skewed(17, 14),
    }
    return out


# ---- the shared expectation, check and emulator run (tests/zwire.py), bound to the narrow form ------------------------------
FORM = ZW.NARROW
slab_of, dims_of = ZW.slab_of, ZW.dims_of
wire_of, expect, check, emu_run = (functools.partial(f, FORM) for f in (ZW.wire_of, ZW.expect, ZW.check, ZW.emu_run))


# ---- the scratch records (csrc/zpack.h) --------------------------------------------------------------------------------
REC_WORDS, ZR_KIND, ZR_N, ZR_MAXBITS, ZR_TABLE = 160, 0, 1, 8, 16


def device_table(out, i, p=0):
    """-> (129 words code | length << 16, maxBits) that measure left for piece p of frame i"""
    rec = out["scratch"][(i * out["pieces"] + p) * REC_WORDS:][:REC_WORDS]
    return [int(x) for x in rec[ZR_TABLE:ZR_TABLE + 129]], int(rec[ZR_MAXBITS])
