"""Cells straight from grid composites, without a GPU: both forms of the cells kernel and the unchanged draw kernel under the CPU
emulator against the oracle's text for the case's canvas, parsed and painted by the restatement (cells, pixels and status
equal, nothing stored outside an image) -- every boundary family of composite_cases.py, several workgroups per descriptor and
idle lanes behind the staging barrier, plain and composite frames in one set, the three walks across tile edges, the flags, the
overflow rule, a plain set after a composite one through either entry --, what images_set_composites decides on the host, and
that host code under the sanitizers as a program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import composite_cases as CC
import emu
import orc
import raster_composites_support as RC
import raster_images_support as RI
import raster_ref as RR
from achip_ctypes import MODE_NAMES, Frame

CASES = RC.cases()
ROOT = RI.emubuild.ROOT
UPPER_HALF = 0x2580


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_the_text_path(name):
    case = CASES[name]
    pixels, start, pitch, status, cells, form = RC.emu_run(case)
    assert form == 1, "a set with a composite frame takes the form with the staged sampler"
    RC.check(name, case, RC.expected(name, case), pixels, start, pitch, status, cells)


def _cells(name):
    case = CASES[name]
    flat = RC.expected(name, case)[0][2]
    return flat.reshape(case.rows, case.cols, 3)


def test_cases_cover_what_they_claim():
    L = emu.lib()
    group = RC.emulator().emu_raster_composites_cells_per_group()
    assert RC.emulator().emu_raster_composites_lds_bytes() == 480 == C.sizeof(RC.Composite) + 16
    # every family, and the cases the families are there for
    singles = [case.frames[0].case for case in CASES.values() if len(case.frames) == 1]
    assert {k.family for k in singles} >= set(CC.FAMILIES)
    assert {k.name for k in singles} >= {CC.ALL_NONE, CC.ZERO_CELL, CC.ONE_PIXEL_CELLS, "a 1x1 source", "a client without video in the middle",
                                         "a small tile in a row of 130 cells"}
    for name in (RC.NINE, RC.HOLE):
        assert {case.mode for case in CASES.values() if len(case.frames) == 1 and case.frames[0].case.name == name
                and case.status is None and case.frames[0].ops is None and case.palette == RC.STD} == set(range(9)), name
    # several workgroups stage one descriptor; the last one has idle lanes behind the barrier, in grids of 1800 and of 620 cells
    for name in (f"true_fg {RC.NINE}", "true_bg three columns at width 62"):
        case = CASES[name].size(L)
        assert case.cols * case.rows > 2 * group and (case.cols * case.rows) % group, name
    assert (CASES[f"true_fg {RC.NINE}"].cols, CASES[f"true_fg {RC.NINE}"].rows) == (60, 30)
    # a grid made from the descriptor, not the terminal's rows: the half-block frames are taller
    case = CASES[f"hb_true {RC.NINE}"].size(L)
    assert case.rows > RC.BY_NAME[RC.NINE].term[1]
    # the mixed batch: plain, A, B, A among the frames run, more set than run, more room than set
    for m in ("true_fg", "hb_256"):
        case = CASES[f"{m} mixed batch: 4 of 6 set, handle of 8"]
        kinds = [it.case.name if isinstance(it, RC.Comp) else None for it in case.frames]
        assert kinds[:4] == [None, RC.NINE, "sources of different sizes", RC.NINE] and case.n == 4 < len(case.frames) < case.max_frames
        d = RC.emu_descriptors(case)
        assert d[0].src and not d[0].comp and d[0].ops & (RI.FLIP_X | RI.TINT) and d[1].comp and not d[1].src and d[1].comp == d[3].comp != d[2].comp
    # HB_256 / HB_16 next to a black margin: the near-black cells at the tile's edge continue the margin's run and are spaces
    slot = RI.slot_of(RI.ATLASES["face"], UPPER_HALF)
    cv = RC.MARGIN_TILE.canvas()
    assert not cv[:, :8].any() and (cv[:, 8:10] == RC.NEAR_BLACK).all() and cv[:, 10].all() and not cv[:, 11:].any()
    cv = RC.EDGE_TILE.canvas()
    assert (cv[:, :4] == RC.NEAR_BLACK).all() and not cv[:, 4:8].any() and cv[:, 8:].all()
    for m in ("hb_256", "hb_16"):
        flat = _cells(f"{m} {RC.MARGIN_TILE.name}")
        top = CASES[f"{m} {RC.MARGIN_TILE.name}"].rows - 10  # (10 text rows under the padding)
        assert (flat[top:, :10, 0] == RI.NO_GLYPH).all() and (flat[top:, 10, 0] == slot).all() and (flat[top:, 11:, 0] == RI.NO_GLYPH).all()
        assert (flat[:top, :, 0] == RI.NO_GLYPH).all()
        # ... and in a tile that fills its cell from column 0 the run begins with the near-black cell: it draws, and so do the
        # black cells behind it
        flat = _cells(f"{m} {RC.EDGE_TILE.name}")
        assert (flat[top:, :, 0] == slot).all()
        assert (flat[top:, :8, 1] == flat[top:, 0:1, 1]).all() and (flat[top:, :8, 2] == flat[top:, 0:1, 2]).all()
    # TRUE_FG with one-byte and multi-byte glyphs over a composite: the black cells behind a bright tile show the tile's colour
    # (their walk back crosses the tile and reaches the black margin in front of it); those in front show their own
    name = f"true_fg mixed palette, {RC.BRIGHT_TILE.name}"
    flat, face = _cells(name), RI.ATLASES["face"]
    dot, full = RI.slot_of(face, ord(".")), RI.slot_of(face, 0x2588)
    assert flat.shape[:2] == (10, 20) and (flat[:, :8, 0] == dot).all() and (flat[:, 8:11, 0] == full).all() and (flat[:, 11:, 0] == dot).all()
    assert (flat[0, :8, 1] == 0).all() and (flat[:, 10, 1] != 0).all() and (flat[:, 11:, 1] == flat[:, 10:11, 1]).all()
    assert (flat[1:, :8, 1] == flat[:-1, 10:11, 1]).all()  # (... and so do those in front of it in the rows below: the row before's)
    # the flags: the descriptor carries them, and the expectation is the frame without them / with the override
    for m in ("true_fg", "hb_true", "256_fg"):
        name = f"{m} flips and a tint on a composite"
        d = RC.emu_descriptors(CASES[name])[0]
        assert d.ops & RI.FLIP_X and d.ops & RI.FLIP_Y and d.ops & RI.TINT and d.comp
        item = CASES[name].frames[0]
        assert item.text(CASES[name].mode, RC.STD) == RC.Comp(RC.FLAGGED).text(CASES[name].mode, RC.STD)
    for m in ("true_fg", "true_bg", "hb_true"):
        name = f"{m} override on a composite"
        item = CASES[name].frames[0]
        assert RC.emu_descriptors(CASES[name])[0].ops & RI.FG_OVERRIDE
        assert item.text(CASES[name].mode, RC.STD) != RC.Comp(RC.FLAGGED).text(CASES[name].mode, RC.STD)


def test_overflow_rule_is_the_parsers():
    seen = set()
    for name, case in CASES.items():
        descs = RC.emu_descriptors(case)
        for d, (_, st, _) in zip(descs, RC.expected(name, case)):
            t = (d.out_h + 1) // 2 if case.mode in RI.HALF_BLOCK else d.out_h
            rule = (RR.OVERFLOW_COLS if d.pad_left + d.out_w > case.cols and d.pad_top < case.rows else 0) | \
                   (RR.OVERFLOW_ROWS if d.pad_top + t > case.rows else 0)
            assert st == rule, (name, st, rule)
            if any(isinstance(it, RC.Comp) for it in case.frames):
                seen.add(st)
    assert seen == {0, 8, 16, 24}


def test_a_plain_set_after_a_composite_one_through_either_entry():
    """nothing of a composite set survives a set without composites: such a set takes the form without the staged sampler through
    either entry and gives images_set's cells, pixels and status; forced into the other form it still does (a plain frame of a
    composite launch takes the plain sampler)"""
    name = f"true_fg {RC.NINE}"
    first = RC.emu_run(CASES[name])
    RC.check(name, CASES[name], RC.expected(name, CASES[name]), *first[:5])
    for mode in (RC.TRUE_FG, RC.HB_256):
        plain = RC.plain_only_case(mode)
        ri = RI.Case(mode, plain.frames, plain.cols, plain.rows)
        want = RI.emu_run(ri)
        RI.check(RC.PLAIN_ONLY, ri, RI.expected(f"{RC.PLAIN_ONLY} {mode}", ri), *want)
        for entry, force, form in ((0, False, 0), (1, False, 0), (0, True, 1)):
            got = RC.emu_run(plain, entry=entry, force_comp=force)
            assert got[5] == form
            assert np.array_equal(got[4], want[4]) and np.array_equal(got[3], want[3])
            span = plain.n * want[2]
            assert got[2] == want[2] and np.array_equal(got[0][got[1]:got[1] + span], want[0][want[1]:want[1] + span])
            RC.check(RC.PLAIN_ONLY, plain, RI.expected(f"{RC.PLAIN_ONLY} {mode}", ri), *got[:5])
    # images_set's own check still refuses the composite frame
    arr = (Frame * 1)(*RC.emu_descriptors(CASES[name]))
    assert RI.emulator().emu_raster_images_check(RC.TRUE_FG, RC.STD.encode(), arr, 1, 1, None) == 1


# ---- what images_set_composites decides on the host ---------------------------------------------------------------------------
def _check(mode, palette, frames, n=None, max_frames=4):
    arr = (Frame * max(1, len(frames)))(*frames)
    why, bad, comps = C.c_char_p(), C.c_int(77), C.c_int(77)
    pal = palette.encode("utf-8") if isinstance(palette, str) else palette
    rc = RC.emulator().emu_raster_composites_check(mode, pal, arr if frames else None, len(frames) if n is None else n, max_frames,
                                                   C.byref(why), C.byref(bad), C.byref(comps))
    assert (rc == 0) == (why.value is None)
    assert (bad.value == -1 and comps.value == sum(1 for f in frames[:len(frames) if n is None else n] if f.comp)) if rc == 0 \
        else (comps.value == 0 and -1 <= bad.value < max(1, len(frames)))
    return rc == 0


def _plain(**kw):
    img = np.zeros((4, 4, 3), dtype=np.uint8)
    f = emu.frame_for_convert(img, 4, 2, 0)
    f._img = img
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def _comp(**kw):
    """a composite frame as a caller makes it; the descriptor is never read on the host: its address here is not one"""
    f = Frame()
    assert emu.lib().achip_frame_setup(C.byref(f), None, 60, 60, 60, 30, 0, True, True, False) == 0
    f.comp = 0x10
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def test_set_refusals_at_their_limits():
    std = orc.PALETTE_STANDARD
    assert _check(1, std, [_comp()]) and _check(1, std, [_plain()]) and _check(1, std, [_plain(), _comp(), _plain(), _comp()])
    # the mode: 0 and 8 are taken, -1 and 9 (the dithered mode) and 10 are not
    assert [_check(m, std, [_comp()]) for m in (-1, 0, 8, 9, 10)] == [False, True, True, False, False]
    # the palette
    assert not _check(1, None, [_comp()]) and not _check(1, "", [_comp()]) and not _check(1, b"a\x1b[0m", [_comp()])
    assert not _check(1, b"a\xe2\x96", [_comp()]) and _check(1, RI.PALETTE_MIXED, [_comp()])
    # the number of frames: 1..max_frames
    four = [_comp() for _ in range(4)]
    assert _check(1, std, four, max_frames=4) and not _check(1, std, four + [_comp()], max_frames=4)
    assert not _check(1, std, four, n=0) and not _check(1, std, [], n=1) and _check(1, std, four, n=1, max_frames=1)
    assert not _check(1, std, four, n=2, max_frames=1)
    # a source, a composite, or both; never neither
    assert _check(1, std, [_comp(src=0x20)]) and not _check(1, std, [_comp(comp=None)]) and not _check(1, std, [_plain(src=None)])
    assert not _check(1, std, [_comp(), _comp(comp=None)]) and _check(1, std, [_comp(), _comp(comp=None)], n=1)
    # sizes and paddings: a plain frame's rules
    for field in ("src_w", "src_h", "out_w", "out_h"):
        assert _check(1, std, [_comp(**{field: 1})]) and not _check(1, std, [_comp(**{field: 0})]), field
    for field in ("pad_left", "pad_top"):
        assert _check(1, std, [_comp(**{field: 0})]) and not _check(1, std, [_comp(**{field: -1})]), field
    top = (1 << 32) - 1
    assert _check(1, std, [_comp(out_w=16, x_ratio=top // 15)]) and not _check(1, std, [_comp(out_w=16, x_ratio=top // 15 + 1)])
    assert _check(1, std, [_comp(out_h=4, y_ratio=top // 3)]) and not _check(1, std, [_comp(out_h=4, y_ratio=top // 3 + 1)])
    # the source extent is a plain frame's matter: a composite frame has no source to measure
    assert not _check(1, std, [_plain(src_stride=1 << 24)]) and _check(1, std, [_plain(src_stride=(1 << 24) - 1)])
    assert _check(1, std, [_comp(src_stride=1 << 24)]) and _check(1, std, [_comp(src_stride=-1)]) and not _check(1, std, [_plain(src_stride=-1)])
    # ops: flips, a tint or an override are taken (the first two do nothing); a dither bit, or a tint with an override, is not
    for ops, ok in ((3, True), (4 | 0x112233 << 8, True), (12, True), (64 | 0x112233 << 8, True), (16, False), (32, False), (48, False),
                    (4 | 64, False), (12 | 64, False)):
        assert _check(1, std, [_comp(ops=ops)]) == ok, ops
        assert _check(1, std, [_plain(), _comp(ops=ops)]) == ok, ops


# ---- the host code under the sanitizers, as a program of its own ----------------------------------------------------------------
def test_host_code_is_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "raster_composites_fuzz")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "ascii-chat_amd", "csrc"), os.path.join(ROOT, "tests", "fuzz", "raster_composites_fuzz.c"),
                           "-o", exe])
    out = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "raster composites fuzz ok" in out.stdout, out.stderr[-3000:]
