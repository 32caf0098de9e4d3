"""Cases of the digital rain pass at its boundaries and parameter extremes, and the rule they are compared under.  Pure
Python and deterministic: the CPU tests (test_rain_boundaries.py), the GPU tests (test_gpu_rain.py) and the fixture script
(golden/make_rain_golden.py) import it; nothing here touches a GPU, the emulator or the restatement.  TESTS ONLY.

boundary_cases(): every token kind with its first byte at every position from B - len(token) - 1 to B + 1 round each
boundary B the kernel has -- the 16-byte thread segment, the 4096-byte chunk, the end of the staged look-ahead (chunk + 64,
behind which the kernel reads global memory), the second chunk boundary -- and round the frame's last byte, where the
frame end cuts the token at every length.  The bytes in front are grid-shaped lines in two variants: "mid" puts the
token mid-row behind a colour event that is pending in its cell (k > 0), "nl" directly behind a newline.  Behind the
token come a colour SGR, a character, a newline and more characters, so that a wrong carry of tokenizer state, cell
position or output offset shows as wrong bytes.  Two steps per case: the second blends with what the first stored.

parameter_cases(): one short multi-event frame, three steps (the last with dt = 0), one field at one extreme per case,
and a few pairs.
"""
import collections
import struct

E = b"\x1b"
SEG, CHUNK, LOOKAHEAD = 16, 4096, 64
BOUNDARIES = (SEG, CHUNK, CHUNK + LOOKAHEAD, 2 * CHUNK, "end")
END_LEN = 230  # length of the frames of the "end" boundary: inside one chunk, at no other boundary
LINE = b"abcdefghijklmnopqrs\n"  # 19 characters and the newline
PENDING = b"ab" + E + b"[48;2;9;80;7m"  # two cells, then a colour event that waits for its character
TAIL = E + b"[38;2;5;6;7mQ\nrest" + E + b"[48;2;30;20;10m+" + LINE[:12]
SMALL_GRID = (11, 7)  # narrower and shorter than the text

Case = collections.namedtuple("Case", "name cols rows frames dts ops")

# name -> (bytes, long).  The offsets of the long kinds (beyond the 64-byte look-ahead) are never thinned.
TOKENS = collections.OrderedDict([
    ("ascii", (b"Z", False)),
    ("utf8_2", ("é".encode(), False)),
    ("utf8_3", ("█".encode(), False)),
    ("utf8_4", ("\U0001F600".encode(), False)),
    ("lead3_cut", (b"\xe2\x96", False)),       # a 3-byte lead with one continuation byte: the tail or the end cuts it
    ("lead4_cut", (b"\xf0\x9f\x98", False)),   # a 4-byte lead with two
    ("stray_continuation", (b"\x80", False)),
    ("newline", (b"\n", False)),
    ("esc_bare", (E, False)),                  # followed by the tail's ESC: two lone ESCs
    ("esc_other", (E + b"x", False)),
    ("esc_bracket", (E + b"[m", False)),       # at one offset its '[' is the first byte behind the boundary
    ("colour_min", (E + b"[48;2;;;m", False)),
    ("colour_fg", (E + b"[38;2;200;100;50m", False)),
    ("colour_bg", (E + b"[48;2;10;220;30m", False)),
    ("colour_long", (E + b"[38;2;" + b"0" * 70 + b"12;" + b"0" * 3 + b"7;9m", True)),  # every run's value < 2^31
    ("colour_broken_long", (E + b"[38;2;1;2;" + b"0" * 60 + b"3;4m", True)),  # a fourth run: the generic CSI takes it
    ("csi_100", (E + b"[" + b"1;" * 49 + b"H", True)),
    ("csi_unterminated", (E + b"[" + b"12;" * 26, True)),  # no tail behind it: it runs to the frame end
    ("rep", (E + b"[5b", False)),
    ("nul", (b"\0zz", False)),                 # the frame ends here; the tail is never read
])


def _lines(n):
    """n bytes of whole lines, the first one shortened: ends in a newline (n > 0)"""
    r = n % len(LINE)
    return (LINE[len(LINE) - r:] if r else b"") + LINE * (n // len(LINE))


def filler(variant, n):
    """n bytes in front of the token"""
    if variant == "nl" or n < len(PENDING) + 1:
        return _lines(n)
    return _lines(n - len(PENDING)) + PENDING


def _offsets(length, long, thin):
    offs = list(range(-length - 1, 2))
    if long or not thin:
        return offs
    return [o for o in offs if o >= -3 or abs(o + length - 1) <= 3 or o % 4 == 0]


def boundary_cases(thin=False, boundaries=BOUNDARIES, kinds=None):
    """[Case].  thin: the short kinds at every offset within 3 of the boundary (their first or their last byte) and every
    fourth beyond; the long kinds always at every offset."""
    out = []
    for kind, (tok, long) in TOKENS.items():
        if kinds is not None and kind not in kinds:
            continue
        tail = b"" if kind == "csi_unterminated" else TAIL
        for B in boundaries:
            for variant in ("mid", "nl"):
                for off in _offsets(len(tok), long, thin):
                    if B == "end":
                        start = END_LEN + off  # off = -1: the token's first byte is the frame's last
                        if off > -1:
                            continue
                        frame = (filler(variant, start) + tok + tail)[:END_LEN]
                        if kind == "nul":
                            frame = filler(variant, start) + tok  # (what lies behind a NUL never counts)
                    else:
                        start = B + off
                        if start < 0:
                            continue
                        frame = filler(variant, start) + tok + tail
                    n = len(out)
                    rows_of_text = frame.count(b"\n") + 1
                    cols, rows = SMALL_GRID if n % 4 == 3 else (20, rows_of_text + 1)
                    out.append(Case(f"{kind}@{B}{off:+d}/{variant}/{cols}x{rows}", cols, rows, [frame, frame], [0.05, 0.07], []))
    return out


def end_cases(cases):
    """the cases at the frame end (their output is what the slot tests size the slot by)"""
    return [c for c in cases if "@end" in c.name]


# The reference takes its sines with sinf, the contract with (float)sin((double)x), and glibc's sinf is one ulp off the
# correctly rounded sine for about one argument in 7 000.  With the sweep's first dt of 0.05 the 20-column
# grids of 200 rows meet two such arguments (cells (78, 13) and (81, 13): sinf(6.5955906f) = 0.3073484 against 0.30734837,
# sinf(6.0365734f) = -0.24411978 against -0.24411976), so the cases recorded from the reference step by 0.04 instead,
# where the two sines agree on every cell of every chosen case.
FIXTURE_DTS = [0.04, 0.07]


def chosen_boundary_cases():
    """about two dozen for the reference fixture: every kind at the chunk boundary, the long ones at chunk + 64 too"""
    pick = []
    for kind, (tok, long) in TOKENS.items():
        # first byte three in front of the boundary, or (long ones) far enough in front to end two bytes behind it
        want = [(CHUNK, -(len(tok) - 2) if long else max(-3, -len(tok)))]
        if long:
            want.append((CHUNK + LOOKAHEAD, -(len(tok) - 2)))
            want.append((CHUNK, -5))  # starts in the chunk, runs on behind the look-ahead
        for B, off in want:
            variant = "mid" if (len(pick) % 2 == 0) else "nl"
            tail = b"" if kind == "csi_unterminated" else TAIL
            frame = filler(variant, B + off) + tok + tail
            cols, rows = (20, frame.count(b"\n") + 2) if len(pick) % 3 else SMALL_GRID
            pick.append(Case(f"{kind}@{B}{off:+d}/{variant}/{cols}x{rows}", cols, rows, [frame, frame], FIXTURE_DTS, []))
    return pick


# ---- parameters ----
NAN, INF = float("nan"), float("inf")
PARAM_ROW = (E + b"[38;2;200;100;50ma" + b"b" + E + b"[48;2;1;2;3m" + E + b"[38;2;9;9;9mc" + b"d" + E + b"[38;2;70;7;7m\n")
PARAM_FRAME = PARAM_ROW * 5 + E + b"[38;2;100;100;100m"  # colour events at each row's end and at the frame's end
PARAM_GRID = (6, 5)
PARAM_DTS = [0.05, 0.07, 0.0]
EXTREMES = [
    ("raindrop_length", [0.0, -0.0, 1e-30, 1e-45, -2.0, 1e30, INF, NAN]),
    ("brightness_decay", [0.0, 1.0, 1.5, -0.5, 1e-45, INF, NAN]),
    ("fall_speed", [0.0, -3.0, 1e20, INF, NAN]),
    ("animation_speed", [0.0, -1.0, 1e9]),
    ("time", [1e7, -5.0, 3e38]),
]
PAIRS = [
    [("raindrop_length", 1e-30), ("time", 1e7)],      # a tiny length with a large time
    [("raindrop_length", 1e30), ("brightness_decay", 1.5)],
    [("fall_speed", 1e20), ("animation_speed", 1e9)],
    [("brightness_decay", 1e-45), ("time", -5.0)],
    [("raindrop_length", -2.0), ("fall_speed", -3.0)],
]


def pack_frame(frame):
    """a frame as [[hex, times], ...] for the fixture: the run of whole filler lines is stored once"""
    i = frame.find(LINE)
    n = 0
    while i >= 0 and frame[i + n * len(LINE):i + (n + 1) * len(LINE)] == LINE:
        n += 1
    if n < 2:
        return [[frame.hex(), 1]]
    return [[frame[:i].hex(), 1], [LINE.hex(), n], [frame[i + n * len(LINE):].hex(), 1]]


def unpack_frame(parts):
    return b"".join(bytes.fromhex(h) * t for h, t in parts)


def fnum(v):
    """a parameter value as the fixture stores it (JSON has no NaN or infinity): repr, read back with float()"""
    return repr(float(v))


def parameter_cases():
    """[Case]; ops are applied before the first step: [field, value as fnum() text] or ["color", r, g, b]"""
    out = []
    for field, values in EXTREMES:
        for v in values:
            out.append(Case(f"{field}={fnum(v)}", *PARAM_GRID, [PARAM_FRAME] * 3, PARAM_DTS, [[field, fnum(v)]]))
    for rgb in ((0, 0, 0), (255, 255, 255)):
        out.append(Case("color=%d,%d,%d" % rgb, *PARAM_GRID, [PARAM_FRAME] * 3, PARAM_DTS, [["color", *rgb]]))
    for pair in PAIRS:
        out.append(Case(",".join(f"{f}={fnum(v)}" for f, v in pair), *PARAM_GRID, [PARAM_FRAME] * 3, PARAM_DTS,
                        [[f, fnum(v)] for f, v in pair]))
    return out


# parameter cases left out of the reference fixture (at most a tenth), each with its reason; they stay in the
# emulator-against-restatement and device-against-restatement tests
NOT_IN_FIXTURE = {}


def apply_case_ops(ctx, ops):
    """a case's ops on a Restated / Emulated / product Rain context (set_field and set_color)"""
    for op in ops:
        if op[0] == "color":
            ctx.set_color(*op[1:])
        else:
            ctx.set_field(op[0], float(op[1]))


# ---- a grid written smaller than allocated ----
SHRUNK_FRAME = (E + b"[38;2;200;100;50mabcdefghijkl" + E + b"[48;2;3;2;1m\n") * 6 + E + b"[38;2;1;1;1m"
# (cols, rows or None for unchanged, dt, overflow): a 12x6 context written down to 7x4 and back
SHRUNK_STEPS = [(None, None, 0.05, False), (None, None, 0.04, False), (7, 4, 0.03, False), (7, 4, 0.06, False),
                (7, 4, 0.02, True), (7, 4, 0.05, False), (12, 6, 0.03, False), (12, 6, 0.04, False)]


# ---- the comparison rule ----
def float_bits(values):
    """binary32 bit patterns of a sequence of floats (a list, a numpy array, a ctypes array)"""
    vals = [float(v) for v in values]
    return list(struct.unpack("<%dI" % len(vals), struct.pack("<%df" % len(vals), *vals)))


def _is_nan_bits(u):
    return (u & 0x7F800000) == 0x7F800000 and (u & 0x007FFFFF) != 0


def canonical_grid_bytes(values):
    """the grid as bytes for hashing, every NaN replaced by the one quiet NaN 0x7FC00000 (sign and payload of an invalid
    operation's NaN differ between x86 and gfx950)"""
    bits = [0x7FC00000 if _is_nan_bits(u) else u for u in float_bits(values)]
    return struct.pack("<%dI" % len(bits), *bits)


def first_difference(got, want):
    n = min(len(got), len(want))
    i = next((k for k in range(n) if got[k] != want[k]), n)
    return f"{len(got)} vs {len(want)} bytes, first difference at byte {i}: {got[max(0, i - 24):i + 24]!r} vs {want[max(0, i - 24):i + 24]!r}"


def check_output(got, want, what):
    """output bytes are equal"""
    assert got == want, f"{what}: {first_difference(got, want)}"


def check_grid(got, want, what, cols=None):
    """stored brightness is equal bit for bit, except where both sides hold a NaN"""
    a, b = float_bits(got), float_bits(want)
    assert len(a) == len(b), f"{what}: grids of {len(a)} and {len(b)} cells"
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y and not (_is_nan_bits(x) and _is_nan_bits(y)):
            where = f"cell {i}" if not cols else f"cell {i} (row {i // cols}, column {i % cols})"
            fx, fy = struct.unpack("<2f", struct.pack("<2I", x, y))
            raise AssertionError(f"{what}: {where} holds {fx!r} (0x{x:08x}), expected {fy!r} (0x{y:08x})")


def check(got_out, want_out, got_grid, want_grid, what, cols=None):
    check_output(got_out, want_out, what)
    check_grid(got_grid, want_grid, what + ": grid", cols)

