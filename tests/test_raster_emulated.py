"""The rasteriser without a GPU: the Python restatement checked by hand, the kernels under the CPU emulator against the
restatement (bytes equal, nothing stored outside an image), what libasciichat_raster.so decides before it needs a device,
and what the two libraries export."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import raster_ref as RR
import raster_support as RS

CASES = RS.cases()
INVALID, NO_DEVICE = 86, 200


# ---- the restatement by hand ------------------------------------------------------------------------------------------------
def _tiny_font():
    # cell 2x2, baseline 2: 'a' fills its cell with alphas 0, 255 / 128, 64; 'w' is 6 wide from x0 = -2, full coverage
    cov = np.array([0, 255, 128, 64] + [255] * 12, dtype=np.uint8)
    return RR.Font(2, 2, 2, [RR.Glyph(ord("a"), 0, 2, 2, 2, 2, 0), RR.Glyph(ord("w"), -2, 2, 6, 2, 6, 4)], cov, default_fg=0xCCCCCC,
                   default_bg=0x102030)


def test_restatement_two_cells_by_hand():
    img, st = RR.render(RS.fgc(255, 0, 0) + RS.bgc(0, 0, 255) + b"a" + RS.sgr(0) + b" ", 2, 1, _tiny_font())
    assert st == 0
    # (255 * 128) / 255 = 128, (255 * 127) / 255 = 127; (255 * 64) / 255 = 64, (255 * 191) / 255 = 191
    assert img.tolist() == [[[0, 0, 255, 255], [255, 0, 0, 255], [16, 32, 48, 255], [16, 32, 48, 255]],
                            [[128, 0, 127, 255], [64, 0, 191, 255], [16, 32, 48, 255], [16, 32, 48, 255]]]
    # truncating division: (1 * 128 + 0 * 127) / 255 = 0, (2 * 128 + 255 * 127) / 255 = 32641 / 255 = 128
    img, _ = RR.render(RS.fgc(1, 2, 0) + RS.bgc(0, 255, 0) + b"a", 1, 1, _tiny_font())
    assert img[1, 0].tolist() == [0, 128, 0, 255]


def test_restatement_overhang_order_by_hand():
    red, dflt = [255, 0, 0, 255], [16, 32, 48, 255]
    # 'w' in the middle of three cells covers all six pixels: it overwrites the EARLIER cell on its left, the LATER cell on its
    # right erases the overhang with its own fill
    img, st = RR.render(b" " + RS.fgc(255, 0, 0) + b"w" + RS.sgr(0) + b" ", 3, 1, _tiny_font())
    assert st == 0 and img[0].tolist() == [red] * 4 + [dflt] * 2 and img[1].tolist() == img[0].tolist()
    # clipped to the image on the left; the later cell's own glyph wins over the overhang
    img, _ = RR.render(RS.fgc(255, 0, 0) + b"w" + RS.fgc(0, 255, 0) + RS.bgc(0, 0, 9) + b"a", 2, 1, _tiny_font())
    assert img[0].tolist() == [red, red, [0, 0, 9, 255], [0, 255, 0, 255]]


def test_restatement_grammar_by_hand():
    f = RS.ATLASES["synth"]
    cells, st = RR.parse(b"X\x1b[5b", 8, 1, f)
    assert st == 0 and [c[0] for c in cells[0]] == [88] * 6 + [0, 0]
    cells, st = RR.parse(RS.fgc(1, 2, 3) + b"a\n\nb" + RS.sgr() + b"c", 2, 3, f)
    assert st == 0 and cells[2] == [(98, 0x010203, f.default_bg), (99, f.default_fg, f.default_bg)] and cells[1][0][0] == 0
    assert RR.parse(b"\x1b[3bA", 4, 1, f)[1] == RR.UNKNOWN and RR.parse(b"abc", 2, 1, f)[1] == RR.OVERFLOW_COLS
    assert RR.xterm_rgb(1) == 0x800000 and RR.xterm_rgb(16) == 0 and RR.xterm_rgb(231) == 0xFFFFFF and RR.xterm_rgb(67) == 0x5F87AF
    assert RR.xterm_rgb(232) == 0x080808 and RR.xterm_rgb(255) == 0xEEEEEE
    assert [RR.matrix_char_map(c) for c in (32, 58, 59, 126, 0xE91A, 31, 127)] == [0xE900, 0xE91A, 0xE900, 0xE90D, 0xE91A, 31, 127]


# ---- the kernels under the emulator -----------------------------------------------------------------------------------------
def test_case_table_places_its_tokens_at_the_builders_chunk():
    assert RS.emulator().emu_raster_chunk() == RS.CHUNK


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_match_restatement(name):
    case = CASES[name]
    pixels, start, pitch, status = RS.emu_run(case)
    RS.check(name, case, pixels, start, pitch, status)


def test_division_by_multiplication_is_exact_for_every_numerator():
    v = np.arange(65536, dtype=np.uint64)
    assert np.array_equal((v * 0x8081) >> 23, v // 255)


def test_cases_cover_what_they_claim():
    # every alpha and both extremes of every channel are in the division pin; the flags frames set one flag each
    assert set(RS.ATLASES["ramp"].coverage[3:].tolist()) == set(range(256))
    one = [s for s in CASES["flags"].status if s]
    assert set(one) == {RR.UNKNOWN, RR.BAD_UTF8, RR.OVERFLOW_COLS, RR.OVERFLOW_ROWS, RR.NO_FRAME}
    # the staged atlas and the atlas read through memory both occur
    assert RS.ATLASES["big"].coverage.size > 32768 >= RS.ATLASES["synth"].coverage.size


# ---- the host, before it needs a device -------------------------------------------------------------------------------------
def _lib():
    L = C.CDLL(RS.LIB)
    L.asciichat_raster_create.restype = C.c_int
    L.asciichat_raster_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(RS.CFont), C.c_int, C.c_int, C.c_int]
    L.asciichat_raster_destroy.argtypes = [C.c_void_p]
    L.asciichat_raster_destroy.restype = None
    L.asciichat_raster_device_count.restype = C.c_int
    L.asciichat_raster_image_pitch.restype = C.c_size_t
    L.asciichat_raster_image_pitch.argtypes = [C.c_void_p]
    return L


def _one_glyph_font(left=0, top=5, width=5, rows=7, pitch=5, offset=0, cov=35, **kw):
    """cell 5x7, baseline 5, one glyph: y0 = 5 - top"""
    return RR.Font(5, 7, 5, [RR.Glyph(65, left, top, width, rows, pitch, offset)], np.zeros(cov, dtype=np.uint8), **kw)


def test_create_refuses_before_it_needs_a_device_and_needs_one_after():
    L = _lib()
    have = L.asciichat_raster_device_count() > 0
    h = C.c_void_p()

    def create(font, cols=3, rows=2, max_frames=1):
        cf = font if isinstance(font, RS.CFont) else RS.c_font(font)
        rc = L.asciichat_raster_create(C.byref(h), C.byref(cf), cols, rows, max_frames)
        if rc == 0:
            assert h.value
            L.asciichat_raster_destroy(h)
        else:
            assert not h.value
        return rc

    accepted = 0 if have else NO_DEVICE
    # the atlas rule (x0 = left, x1 = left + width, y0 = 5 - top, y1 = y0 + rows within [-5, 10] x [-7, 14]), the pitch and the
    # coverage bound: each at its limit is taken, one beyond is refused
    def glyph(left=0, top=5, width=5, rows=7, pitch=None, cov=None):
        pitch = width if pitch is None else pitch
        return _one_glyph_font(left, top, width, rows, pitch, 0, max(pitch, width) * rows if cov is None else cov)

    for ok, bad in ((dict(left=-5, width=1), dict(left=-6, width=1)), (dict(width=10), dict(width=11)),
                    (dict(top=12, rows=1), dict(top=13, rows=1)), (dict(rows=14), dict(rows=15)),
                    (dict(pitch=5), dict(pitch=4, cov=35)), (dict(cov=35), dict(cov=34))):
        assert create(glyph(**ok)) == accepted, ok
        assert create(glyph(**bad)) == INVALID, bad
    two = _one_glyph_font()
    two.glyphs = [RR.Glyph(66, 0, 5, 5, 7, 5, 0), RR.Glyph(65, 0, 5, 5, 7, 5, 0)]
    assert create(two) == INVALID  # unsorted
    two.glyphs = [RR.Glyph(65, 0, 5, 5, 7, 5, 0), RR.Glyph(65, 0, 5, 5, 7, 5, 0)]
    assert create(two) == INVALID  # duplicate
    two.glyphs = [RR.Glyph(65, 0, 5, 5, 7, 5, 0), RR.Glyph(66, 0, 5, 5, 7, 5, 0)]
    assert create(two) == accepted
    # every limit: at it, and one beyond
    good = _one_glyph_font()
    for kw_ok, kw_bad in ((dict(cols=1), dict(cols=0)), (dict(cols=1024, rows=1), dict(cols=1025, rows=1)), (dict(rows=1), dict(rows=0)),
                          (dict(rows=512, cols=1), dict(rows=513, cols=1)), (dict(max_frames=1), dict(max_frames=0)),
                          (dict(max_frames=4096, cols=1, rows=1), dict(max_frames=4097, cols=1, rows=1))):
        assert create(good, **kw_ok) == accepted, kw_ok
        assert create(good, **kw_bad) == INVALID, kw_bad
    empty = np.zeros(0, dtype=np.uint8)
    for (cw, ch, bl), rc in (((1, 1, 0), accepted), ((0, 1, 0), INVALID), ((32, 64, 64), accepted), ((33, 64, 0), INVALID),
                             ((32, 65, 0), INVALID), ((1, 0, 0), INVALID), ((5, 7, -1), INVALID), ((5, 7, 8), INVALID),
                             ((5, 7, 7), accepted)):
        assert create(RR.Font(cw, ch, bl, [], empty)) == rc, (cw, ch, bl)
    many = [RR.Glyph(100 + k, 0, 5, 1, 1, 1, 0) for k in range(1025)]
    assert create(RR.Font(5, 7, 5, many[:1024], np.zeros(1, dtype=np.uint8))) == accepted
    assert create(RR.Font(5, 7, 5, many, np.zeros(1, dtype=np.uint8))) == INVALID
    assert create(RR.Font(5, 7, 5, [], np.zeros(1 << 20, dtype=np.uint8))) == accepted
    assert create(RR.Font(5, 7, 5, [], np.zeros((1 << 20) + 1, dtype=np.uint8))) == INVALID
    for indexed in (0, 3, -1):
        assert create(good.replace(indexed=indexed)) == INVALID
    assert create(good.replace(indexed=RR.INDEXED_XTERM)) == accepted
    # NULL arguments
    cf = RS.c_font(good)
    assert L.asciichat_raster_create(None, C.byref(cf), 3, 2, 1) == INVALID
    assert L.asciichat_raster_create(C.byref(h), None, 3, 2, 1) == INVALID and not h.value
    cf.glyphs = C.POINTER(RS.CGlyph)()
    assert create(cf) == INVALID
    cf = RS.c_font(good)
    cf.coverage = None
    assert create(cf) == INVALID
    cf.n_glyphs = -1
    assert create(cf) == INVALID
    assert L.asciichat_raster_image_pitch(None) == 0
    L.asciichat_raster_destroy(None)  # nothing happens


# ---- what the libraries export ----------------------------------------------------------------------------------------------
def _exports(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in nm.splitlines() if l.strip())


def test_raster_library_exports_only_its_interface():
    syms = _exports(RS.LIB)
    assert syms and all(s.startswith("asciichat_raster_") for s in syms), syms
    for name in ("create", "run", "destroy", "device_count", "width_px", "height_px", "image_pitch"):
        assert "asciichat_raster_" + name in syms
    needed = subprocess.run(["readelf", "-d", RS.LIB], capture_output=True, text=True, check=True).stdout
    assert "libasciichat_hip" not in needed  # it needs nothing of the other library


def test_hip_library_exports_what_it_exported_before():
    with open(os.path.join(RS.ROOT, "tests", "golden", "hip_exports.txt")) as f:
        before = f.read().split()
    assert _exports(RS.HIP_LIB) == before
