"""Cells straight from frame descriptors, without a GPU: the new kernel and the unchanged draw kernel under the CPU emulator
against the existing chain on the CPU -- the oracle's text for what a descriptor samples, parsed and painted by the
restatement (cells, pixels and status equal, nothing stored outside an image) --, what images_set decides on the host, the
overflow rule, and the host code under the sanitizers as a program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu
import orc
import raster_images_support as RI
import raster_ref as RR
from achip_ctypes import Frame

CASES = RI.cases()
ROOT = RI.emubuild.ROOT


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_the_text_path(name):
    case = CASES[name]
    pixels, start, pitch, status, cells = RI.emu_run(case)
    RI.check(name, case, RI.expected(name, case), pixels, start, pitch, status, cells)


def test_cases_cover_what_they_claim():
    L = emu.lib()
    face = RI.ATLASES["face"]
    assert all(face.coverage[g.offset + r * g.pitch + c] for g in face.glyphs for r in range(g.rows) for c in range(g.width))
    assert {g.codepoint for g in face.glyphs} == set(range(32, 127)) | {0x2580, 0x2591, 0x2592, 0x2593, 0x2588}
    assert any(g.left < 0 or g.left + g.width > face.cell_w for g in face.glyphs)

    def desc(name, i=0):
        case = CASES[name]
        return RI.descriptor(L, Frame, case.mode, case.frames[i], case.frames[i].buf.ctypes.data)

    d = desc("true_fg pad_left 8")
    assert (d.pad_left, d.pad_top, d.out_w, d.out_h) == (8, 0, 4, 6)
    assert desc("true_fg pad_top").pad_top > 0 and desc("hb_256 pad_top").pad_top > 0
    assert desc("hb_true odd height").out_h == 5 and desc("true_fg row stride 160").src_stride == 160
    assert desc("true_fg both flips").ops & 3 == 3 and desc("hb_true tint").ops & 12 == 4 and desc("256_fg tint on white").ops & 12 == 12
    assert CASES["true_fg 300x2: two workgroups, two tiles"].cols > RI.emulator().emu_raster_images_cells_per_group()
    # the pad pen: row 1's pad cells carry the colour of row 0's last cell, not the default
    name = "true_fg pad_left 8"
    flat = RI.expected(name, CASES[name])[0][2].reshape(6, 20, 3)
    assert (flat[1:, :8, 1] == flat[:-1, 11:12, 1]).all() and (flat[0, :8, 1] == face.default_fg).all()
    assert (flat[1:, :8, 1] != face.default_fg).all() and (flat[:, :8, 0] == RI.NO_GLYPH).all()
    # the mixed palette: a one-byte cell shows the colour of the multi-byte cell in front of it
    name = "true_fg mixed palette: a pen outlives its cell"
    flat = RI.expected(name, CASES[name])[0][2].reshape(2, 6, 3)
    assert flat[0, 2, 1] == flat[0, 3, 1] == flat[0, 1, 1] == 0xC8D2DC and flat[0, 4, 1] == 0x1E140A and flat[1, 0, 1] == 0xC8D2DC
    # the run's first cell decides: three spaces, a coloured cell, four drawn cells of which two are black
    name = "hb_256 the run's first cell decides"
    flat = RI.expected(name, CASES[name])[0][2]
    assert (flat[:3, 0] == RI.NO_GLYPH).all() and (flat[3:, 0] != RI.NO_GLYPH).all()
    # both sides of l = 16 and of every shade step; a cell dark above and bright below draws
    flat = RI.expected("hb_mono shade steps", CASES["hb_mono shade steps"])[0][2]
    shades = [RI.slot_of(face, cp) for cp in (0x2591, 0x2592, 0x2593, 0x2588)]
    assert flat[:, 0].tolist() == [RI.NO_GLYPH, shades[0], shades[0], shades[1], shades[1], shades[2], shades[2], shades[3], shades[0]]
    # a missing glyph occurs, and flat and xterm colours differ
    flat = RI.expected("true_fg a glyph the face lacks", CASES["true_fg a glyph the face lacks"])[0][2]
    full = RI.expected("true_fg 48x16 -> 16x4", CASES["true_fg 48x16 -> 16x4"])[0][2]
    assert ((flat[:, 0] == RI.NO_GLYPH) & (full[:, 0] == RI.slot_of(face, ord("o")))).any()
    a, b = (RI.expected(n, CASES[n])[0][0] for n in ("256_fg 48x16 -> 16x4", "256_fg flat indexed colours"))
    assert not np.array_equal(a, b)


def test_overflow_rule_is_the_parsers():
    """OVERFLOW_COLS iff pad_left + out_w > cols in a text row of the grid, OVERFLOW_ROWS iff pad_top + text rows > rows"""
    L = emu.lib()
    seen = set()
    for name, case in CASES.items():
        descs = RI.descriptors(L, Frame, case, [s.buf.ctypes.data for s in case.frames])
        for d, (_, st, _) in zip(descs, RI.expected(name, case)):
            t = (d.out_h + 1) // 2 if case.mode in RI.HALF_BLOCK else d.out_h
            rule = (RR.OVERFLOW_COLS if d.pad_left + d.out_w > case.cols and d.pad_top < case.rows else 0) | \
                   (RR.OVERFLOW_ROWS if d.pad_top + t > case.rows else 0)
            assert st == rule, (name, st, rule)
            seen.add(st)
    assert seen == {0, 8, 16, 24}


# ---- what images_set decides on the host ------------------------------------------------------------------------------------
def _check(mode, palette, frames, n=None, max_frames=4):
    arr = (Frame * max(1, len(frames)))(*frames)
    why = C.c_char_p()
    pal = palette.encode("utf-8") if isinstance(palette, str) else palette
    rc = RI.emulator().emu_raster_images_check(mode, pal, arr if frames else None, len(frames) if n is None else n, max_frames,
                                               C.byref(why))
    assert (rc == 0) == (why.value is None)
    return rc == 0


def _good():
    img = np.zeros((4, 4, 3), dtype=np.uint8)
    f = emu.frame_for_convert(img, 4, 2, 0)
    f._img = img
    return f


def _with(**kw):
    f = _good()
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def test_set_refusals_at_their_limits():
    std = orc.PALETTE_STANDARD
    assert _check(0, std, [_good()])
    # the mode: 0 and 8 are taken, -1 and 9 (the dithered mode) and 10 are not
    assert [_check(m, std, [_good()]) for m in (-1, 0, 8, 9, 10)] == [False, True, True, False, False]
    # the palette
    assert not _check(1, None, [_good()]) and not _check(1, "", [_good()])
    for ok in ("#", "é", "ࠀ", "￿", "\U00010000", "\U0010ffff", "~ ", orc.PALETTE_BLOCKS):
        assert _check(1, ok, [_good()]), ok
    for bad in (b"a\x80", b"\xc3", b"a\xe2\x96", b"\xc0\x80", b"\xc1\xbf", b"\xe0\x9f\xbf", b"\xed\xa0\x80", b"\xf0\x8f\xbf\xbf",
                b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xff", b"a\x1b[0m", b"a\nb", b"a\x1fb", b"a\x7fb", b"\xe2\x96a"):
        assert not _check(1, bad, [_good()]), bad
    assert _check(1, b"\xed\x9f\xbf\xee\x80\x80", [_good()])  # the code points on either side of the surrogates
    # the number of frames
    four = [_good() for _ in range(4)]
    assert _check(1, std, four, max_frames=4) and not _check(1, std, four + [_good()], max_frames=4)
    assert not _check(1, std, four, n=0) and not _check(1, std, [], n=1) and _check(1, std, four, n=1, max_frames=1)
    # a composite, no source
    assert not _check(1, std, [_with(comp=1)]) and not _check(1, std, [_with(src=None)])
    assert not _check(1, std, [_good(), _with(src=None)]) and _check(1, std, [_good(), _with(src=None)], n=1)
    # sizes
    for field in ("src_w", "src_h", "out_w", "out_h"):
        assert _check(1, std, [_with(**{field: 1})]) and not _check(1, std, [_with(**{field: 0})]), field
    for field in ("pad_left", "pad_top"):
        assert _check(1, std, [_with(**{field: 0})]) and not _check(1, std, [_with(**{field: -1})]), field
    # (out - 1) * ratio below 2^32
    top = (1 << 32) - 1
    assert _check(1, std, [_with(out_w=16, x_ratio=top // 15)]) and not _check(1, std, [_with(out_w=16, x_ratio=top // 15 + 1)])
    assert _check(1, std, [_with(out_h=4, y_ratio=top // 3)]) and not _check(1, std, [_with(out_h=4, y_ratio=top // 3 + 1)])
    # the extent: a stride below 2^24, not negative
    assert _check(1, std, [_with(src_stride=(1 << 24) - 1)]) and not _check(1, std, [_with(src_stride=1 << 24)])
    assert not _check(1, std, [_with(src_stride=-1)])
    # ops: flips, a tint or an override are taken; a dither bit, or a tint with an override, is not
    for ops, ok in ((3, True), (4 | 0x112233 << 8, True), (12, True), (64 | 0x112233 << 8, True), (16, False), (32, False), (48, False),
                    (4 | 64, False), (12 | 64, False)):
        assert _check(1, std, [_with(ops=ops)]) == ok, ops


# ---- the host code under the sanitizers, as a program of its own ----------------------------------------------------------------
def test_host_code_is_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "raster_images_fuzz")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ascii-chat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fuzz", "raster_images_fuzz.c"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([exe, "20000"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "raster images fuzz ok" in out.stdout, out.stderr[-3000:]
