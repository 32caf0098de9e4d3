"""Packed RGB sources as the tiles of grid composites, without a GPU: the two kernels of libasciichat_pixgrid.so under the CPU
emulator against tests/pixgrid_ref.py (pix_ref's whole conversion indexed by the samplers' rule, and box_ref over it) over the
shared case table -- the averaged kernel also at every other segment width and under DESC, LATE and RANDOM wave schedules with
shuffled workgroup order --, hand-derived tiles, the cut shapes the case table claims from the library's own cut, the host walks
of the rule, the handle's ticks and every refusal at its limit through pixgrid.c itself (over the mock HIP runtime), what the
library and the package export, and the host code under the sanitizers as a program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pix_support as PS
import pixgrid_ref as GR
import pixgrid_support as XS
from emu_schedule import DEFAULT, Schedule, scheduled

ROOT = XS.emubuild.ROOT
PKG = os.path.join(ROOT, "ascii-chat_amd")
LIB = os.path.join(PKG, "libasciichat_pixgrid.so")
CASES = XS.cases()


# ---- the rule by hand ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", XS.FORMATS, ids=[XS.NAMES[f] for f in XS.FORMATS])
def test_hand_derived_tiles(fmt):
    """a 2x2 source written out byte by byte: pixels (R, G, B) = (10, 20, 30) (50, 60, 70) / (90, 100, 110) (130, 140, 151), alpha
    0xEE; the 1x1 sampled tile is pixel (0, 0), the 1x1 averaged tile (280 + 2) / 4, (320 + 2) / 4, (361 + 2) / 4"""
    rgb = [(10, 20, 30), (50, 60, 70), (90, 100, 110), (130, 140, 151)]
    data = []
    for r, g, b in rgb:
        data += {XS.RGB: [r, g, b], XS.RGBA: [r, g, b, 0xEE], XS.BGR: [b, g, r], XS.BGRA: [b, g, r, 0xEE]}[fmt]
    pixels = np.array(data, dtype=np.uint8)
    s = PS.CSource()
    s.format, s.width, s.height, s.pixels, s.stride = fmt, 2, 2, pixels.ctypes.data, 0
    nine = (PS.CSource * 9)()
    nine[0] = s
    comp = XS.Composite()
    comp.canvas_w = comp.canvas_h = comp.cols = comp.rows = comp.cell_w = comp.cell_h = comp.n_src = 1
    d = comp.s[0]
    d.src, d.src_w, d.src_h, d.src_stride, d.tile_w, d.tile_h, d.x_ratio, d.y_ratio = XS.PLACED, 2, 2, 6, 1, 1, GR.ratio(2, 1), GR.ratio(2, 1)
    comps, nines = (C.c_void_p * 1)(C.addressof(comp)), (C.c_void_p * 1)(C.addressof(nine))
    for box, want in ((0, (10, 20, 30)), (1, (70, 80, 90))):
        for host in (0, 1):
            buf = np.full(48, XS.FILL, np.uint8)
            at = (-buf.ctypes.data) % 16
            assert XS.emulator().emu_pixgrid_run(C.cast(comps, C.c_void_p), C.cast(nines, C.c_void_p), 1, 1, buf.ctypes.data + at, box, host) == 0
            assert tuple(buf[at:at + 3].tolist()) == want and (buf[:at] == XS.FILL).all() and (buf[at + 3:] == XS.FILL).all(), (box, host)


# ---- the kernels under the emulator -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", XS.KINDS)
@pytest.mark.parametrize("name", list(CASES))
def test_tiles_match_the_restatement(name, kind):
    case = CASES[name]
    buf, start, p = XS.emu_run(case, kind)
    XS.check_slab(name, case, kind, buf, start)
    # the offsets and the slab's size
    lay = XS.emu_layout(case, p)
    assert (lay["at"], lay["bytes"]) == case.layout(), name
    # composites(): the named fields of the packed slots and nothing else -- the RGB24 and the empty slots byte for byte
    tiles = buf.ctypes.data + start
    out = XS.emu_composites(case, p, tiles)
    XS.check_rewrite(name, case, p.comps, out, tiles)
    for comp, given, got in zip(case.comps, p.comps, out):
        for k in range(9):
            if not comp.is_yuv(k):
                assert bytes(got.s[k]) == bytes(given.s[k]), (name, k)


@pytest.mark.parametrize("seg", XS.OTHER_WIDTHS, ids=["no split" if s == XS.NO_SPLIT else str(s) for s in XS.OTHER_WIDTHS])
def test_averaged_tiles_at_the_other_segment_widths(seg):
    """the averaged kernel over every case with the host's cut at another width (the driver built with -DPIXGRID_SEG_COLS)"""
    assert XS.emulator(seg).emu_pixgrid_seg_cols() == seg and set(XS.CANDIDATES) - {XS.SHIPPED} <= set(XS.OTHER_WIDTHS)
    for name, case in CASES.items():
        buf, start, p = XS.emu_run(case, "box", seg)
        XS.check_slab(f"{name} at width {seg}", case, "box", buf, start)
        if case.tiles:
            _check_table(name, case, seg)


# the averaged kernel has one barrier between the column sums and the box sums: four waves a workgroup; segments of a row and
# rows of a tile are workgroups of their own, so their order must not matter either
SCHEDULES = [Schedule.desc().workgroups("shuffle", 2), Schedule.late(3, 30, 0).workgroups("desc"), Schedule.late(0, 300, 1).workgroups("shuffle", 5),
             Schedule.random(1).workgroups("shuffle", 1), Schedule.random(3).workgroups("shuffle", 7)]


@pytest.mark.parametrize("seg", (None, 16), ids=("shipped", "16"))
def test_averaged_tiles_under_other_schedules(seg):
    for name, case in CASES.items():
        for s in SCHEDULES:
            try:
                with scheduled(XS.emulator(seg), s) as r:
                    buf, start, _ = XS.emu_run(case, "box", seg)
                    XS.check_slab(name, case, "box", buf, start)
            except AssertionError as e:
                raise AssertionError(f"case [{name}] at segment width [{seg or XS.SHIPPED}] under [{s}]: {e}") from None
            assert r.naps == 0, "the kernel has no polling loop"
    assert DEFAULT not in SCHEDULES and {s.waves for s in SCHEDULES} == {"desc", "late", "random"} and all(s.wg != "asc" for s in SCHEDULES)


@pytest.mark.parametrize("kind", XS.KINDS)
def test_host_walks_equal_the_restatement(kind):
    """pixgrid.h's pixgrid_host_tile and pixgrid_host_box_tile (what the fuzz program walks): the same bytes, the same guard"""
    for name in [n for n in CASES if "20x6" in n or "x1 ->" in n or "larger" in n] + [XS.MIXED, "BGRA " + XS.CLAMPED]:
        buf, start, _ = XS.emu_run(CASES[name], kind, host=True)
        XS.check_slab(name, CASES[name], kind, buf, start)


def test_alpha_plays_no_part():
    """the same pixels under two alphas: equal tiles in both forms"""
    for name, clear, opaque in XS.alpha_pairs():
        for kind in XS.KINDS:
            got = []
            for case in (clear, opaque):
                buf, start, _ = XS.emu_run(case, kind)
                XS.check_slab(f"{name} alpha", case, kind, buf, start)
                got.append(buf[start:start + 45].copy())
            assert np.array_equal(got[0], got[1]), (name, kind)


# ---- the workgroup table and the cut of a row ----------------------------------------------------------------------------------------
def _check_table(name, case, seg):
    p = XS.place_on_host(case)
    lay = XS.emu_layout(case, p, seg)
    width = XS.SHIPPED if seg is None else seg
    first = 0
    for t, tile in enumerate(case.tiles):
        segs, k = lay["segs"][t], lay["seg_out"][t]
        assert lay["first_wg"][t] == first, (name, seg, t)
        first += segs * tile.tile_h
        cut = XS.segments(tile.src_w, tile.tile_w, k)
        assert len(cut) == segs and cut[0][0] == 0 and cut[-1][1] == tile.tile_w and all(a[1] == b[0] for a, b in zip(cut, cut[1:])), (name, seg, t)
        assert all(xb - xa == k for xa, xb, _, _ in cut[:-1]) and 1 <= cut[-1][1] - cut[-1][0] <= k, (name, seg, t)
        for xa, xb, c0, c1 in cut:
            assert c0 % 4 == 0 and c0 < c1 <= tile.src_w
            assert (c1 + 3) // 4 * 4 - c0 <= lay["cols"][t], (name, seg, t, xa)  # the groups that touch [c0, c1) end at most three columns behind it
            # the bound: a segment's source columns stay within the width, unless it is one box that no width can cut
            assert width == XS.NO_SPLIT or c1 - c0 <= width or xb - xa == 1, (name, seg, t, xa, c1 - c0)
        if width == XS.NO_SPLIT:
            assert (segs, k) == (1, tile.tile_w)
        cols, slices = lay["cols"][t], lay["slices"][t]
        assert cols % 4 == 0 and cols <= (tile.src_w + 3) // 4 * 4 and slices == (4 if cols <= 256 else 2 if cols <= 512 else 1), (name, seg, t)
    assert lay["workgroups"] == first and 0 < lay["stage_cols"] <= XS.MAX_W and lay["boxable"]
    assert lay["stage_cols"] == max(c * s for c, s in zip(lay["cols"], lay["slices"]))
    assert lay["max_pixels"] == max(t.tile_w * t.tile_h for t in case.tiles)
    return lay


def test_the_cases_have_the_cut_shapes_they_claim():
    """from the library's own host cut, at the width it ships with"""
    assert XS.emulator().emu_pixgrid_seg_cols() == XS.SHIPPED == 512 and XS.SHIPPED in XS.CANDIDATES
    for n in ("BGRA", "BGR"):
        lay = _check_table("three segments", CASES[f"{n} {XS.THREE_SEGMENTS}"], None)
        assert (lay["segs"], lay["seg_out"], lay["slices"], lay["workgroups"]) == ([3], [5], [2], 6) and 13 % 5 == 3
        lay = _check_table("wide box", CASES[f"{n} {XS.WIDE_BOX}"], None)
        assert (lay["segs"], lay["seg_out"], lay["slices"]) == ([2], [1], [1]) and lay["cols"][0] > 512
        for name, rows in ((XS.MANY_ROWS, 37), (XS.FEW_ROWS, 3)):
            lay = _check_table(name, CASES[f"{n} {name}"], None)
            assert (lay["segs"], lay["slices"], lay["cols"]) == ([1], [4], [40])
            box_rows = [hi - lo for lo, hi in (XS.bounds(rows, 3, y) for y in range(3))]
            assert all(r > 4 for r in box_rows) if rows == 37 else all(r < 4 for r in box_rows)
        t = CASES[f"{n} 1031x3 -> tile 7x2 a second group per lane, segments start off a multiple of four"].tiles[0]
        assert t.src_w // 4 > 256 and any(XS.bounds(1031, 7, x)[0] % 4 for x in range(7))
    white = CASES[XS.WHITE]
    lay = _check_table("white", white, None)
    assert (lay["segs"], lay["slices"], lay["cols"], lay["stage_cols"]) == ([1], [1], [XS.MAX_W], XS.MAX_W)
    assert XS.MAX_W * 9 * 255 > 1 << 23 and (white.tiles[0].source.whole() == 255).all() and all((e == 255).all() for e in white.expected("box"))


def test_cases_cover_what_they_claim():
    for fmt in XS.FORMATS:
        n = XS.NAMES[fmt]
        offs = set()
        for off in (0, 1 + fmt % 3):
            for kind in XS.STRIDES:
                s = CASES[f"{n} 20x6 -> tile 5x3 base +{off} stride {kind}"].tiles[0].source
                offs.add((s.at - 64) % 16)
                assert {"tight": s.given == 0, "16": s.stride % 16 == 0 and s.stride > XS.BPP[fmt] * 20, "1": s.stride % 2 == 1}[kind]
        assert offs == {0, 1 + fmt % 3}
        assert all(f"{n} {w}x1 -> tile 2x1" in CASES for w in (1, 2, 3, 5, 6, 7))
    assert {1 + f % 3 for f in XS.FORMATS} == {1, 2, 3} and {w % 4 for w in (1, 2, 3, 5, 6, 7)} == {1, 2, 3}
    assert {(t.tile_w * t.tile_h) % 4 for c in CASES.values() for t in c.tiles if t.tile_w * t.tile_h < 16} == {0, 1, 2, 3}
    assert any(t.tile_w == 3 and t.tile_h > 1 for c in CASES.values() for t in c.tiles)
    up = CASES["BGRA 4x2 -> tile 9x5 larger than its source"].tiles[0]
    assert up.x_ratio < 65536 and up.y_ratio < 65536
    cl = CASES["BGRA " + XS.CLAMPED].tiles[0]
    assert (8 * cl.x_ratio) >> 16 > 3 and (4 * cl.y_ratio) >> 16 > 1
    assert 37 * 29 > 1024
    one_axis = [t for c in CASES.values() for t in c.tiles if "one axis" in [n for n, v in CASES.items() if v is c][0]]
    assert one_axis and all(t.tile_w > t.src_w and t.tile_h < t.src_h for t in one_axis)
    mixed = CASES[XS.MIXED]
    assert [len([s for s in c.slots if s is not None]) for c in mixed.comps] == [7, 4, 1] and mixed.comps[0].n_src == 8 < 9
    nine = mixed.comps[0]
    assert nine.slots[6] is None and not nine.slots[4].yuv and len(mixed.tiles) == 11 < mixed.max_tiles == 20
    assert {t.source.format for t in mixed.tiles} == set(XS.FORMATS) and len({(t.tile_w, t.tile_h) for t in mixed.tiles}) >= 10
    assert any(3 * t.tile_w * t.tile_h % 16 for t in mixed.tiles)
    assert not CASES[XS.NO_PACKED].tiles and CASES[XS.NO_PACKED].layout() == ([], 0)


def test_mixed_set_pins_the_table_and_the_offsets():
    case = CASES[XS.MIXED]
    sizes = [(t.tile_w, t.tile_h) for t in case.tiles]
    assert sizes == [(20, 15), (7, 4), (5, 3), (19, 2), (1, 1), (9, 11), (20, 12), (17, 5), (8, 8), (20, 3), (24, 10)]
    lay = _check_table(XS.MIXED, case, None)
    heights = [h for _, h in sizes]
    assert lay["segs"] == [1] * 11 and lay["first_wg"] == [sum(heights[:t]) for t in range(11)] and lay["workgroups"] == sum(heights) == 74
    assert lay["at"][:6] == [0, 912, 1008, 1056, 1184, 1200] and lay["max_pixels"] == 300
    lay = _check_table(XS.MIXED, case, 16)  # segments of a few boxes: many workgroups a row
    assert max(lay["segs"]) > 4 and lay["workgroups"] == sum(s * h for s, h in zip(lay["segs"], heights))


# ---- the host side, through pixgrid.c over the mock runtime --------------------------------------------------------------------------
def _host_slab(case):
    buf, start = XS.slab(case)
    return buf.ctypes.data + start, lambda: (buf, start)


def test_refusals_at_their_limits_and_a_refused_set_changes_nothing():
    XS.check_refusals(XS.mock_library(), XS.place_on_host, _host_slab)


def test_a_source_beyond_the_box_pass_is_served_by_run_and_refused_by_run_box():
    L = XS.mock_library()
    before = L.emu_pixgrid_launches()
    XS.check_too_large_for_the_box(L, XS.place_on_host, _host_slab)
    assert L.emu_pixgrid_launches() == before + 1  # (run's; run_box launched nothing)
    case = XS.too_large_case()
    assert not XS.emu_layout(case, XS.place_on_host(case))["boxable"]


def test_set_check_names_composite_and_slot():
    case = XS.refusal_case()
    p = XS.place_on_host(case)

    def check(t, n=2, max_tiles=3):
        bad_c, bad_s, tiles, why = C.c_int(-5), C.c_int(-5), C.c_int(-5), C.c_char_p()
        rc = XS.emulator().emu_pixgrid_set_check(C.cast(t.comp_ptrs, C.c_void_p), C.cast(t.nine_ptrs, C.c_void_p), n, max_tiles, C.byref(bad_c),
                                                 C.byref(bad_s), C.byref(tiles), C.byref(why))
        assert (rc == 0) == (why.value is None)
        return rc, bad_c.value, bad_s.value, tiles.value

    assert check(p) == (0, -1, -1, 3) and check(p, n=1) == (0, -1, -1, 1)
    t = XS.Trial(p)
    t.comps[1].s[2].tile_h = XS.MAX_TILE + 1
    assert check(t) == (1, 1, 2, 0)
    t = XS.Trial(p)
    t.nines[0][0].stride = -1
    assert check(t) == (1, 0, 0, 0)
    assert check(p, max_tiles=2) == (1, 1, 2, 0) and check(p, n=0) == (1, -1, -1, 0)


def test_the_handle_through_the_mock_runtime():
    """set, tiles_bytes, run, run_box, composites of pixgrid.c itself: two ticks on one stream -- other pixels, other formats, the
    same geometry: every tile stays where it was --, a refused set in between, then a set without packed slots, which launches
    nothing"""
    L = XS.mock_library()
    ticks = [XS.mixed_set(700), XS.mixed_set(1700, shift=1)]
    assert ticks[0].layout() == ticks[1].layout() and all(a.source.format != b.source.format for a, b in zip(ticks[0].tiles, ticks[1].tiles))
    g = XS.Handle(L, 20)
    try:
        for k, case in enumerate(ticks):
            p = XS.place_on_host(case)  # (fresh copies: other pixel pointers)
            assert g.set(p) == 0 and g.tiles_bytes() == case.layout()[1]
            for kind in XS.KINDS:
                buf, start = XS.slab(case)
                tiles = buf.ctypes.data + start
                launches = L.emu_pixgrid_launches()
                assert g.run(tiles, kind) == 0 and L.emu_pixgrid_launches() == launches + 1  # one launch per form
                XS.check_slab(f"tick {k}", case, kind, buf, start)
                rc, out = g.composites(tiles, 3)
                assert rc == 0
                XS.check_rewrite(f"tick {k}", case, p.comps, out, tiles)
        # a refused set leaves the previous set's run intact
        bad = XS.Trial(p)
        bad.comps[0].s[0].tile_w = 0
        for kind in XS.KINDS:
            buf, start = XS.slab(case)
            assert g.set(bad) == XS.INVALID and "composite 0 slot 0" in g.error() and g.run(buf.ctypes.data + start, kind) == 0
            XS.check_slab("after a refused set", case, kind, buf, start)
        none = CASES[XS.NO_PACKED]
        p = XS.place_on_host(none)
        guard, start = XS.slab(ticks[0])
        launches = L.emu_pixgrid_launches()
        assert g.set(p) == 0 and g.tiles_bytes() == 0
        for kind in XS.KINDS:  # nothing to launch, with or without a slab
            assert g.run(None, kind) == 0 and g.run(guard.ctypes.data + start, kind) == 0
        assert L.emu_pixgrid_launches() == launches and (guard == XS.FILL).all()
        rc, out = g.composites(None, 1)
        assert rc == 0 and bytes(out[0]) == bytes(p.comps[0])
    finally:
        g.close()


# ---- what the library and the package export -----------------------------------------------------------------------------------------
def test_pixgrid_library_exports_only_its_interface():
    assert os.path.exists(LIB), "libasciichat_pixgrid.so has not been built (make -C ascii-chat_amd)"
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[-1] for l in nm.splitlines() if l.strip())
    assert len(XS.EXPORTS) == 9 and syms == sorted("asciichat_pixgrid_" + n for n in XS.EXPORTS), syms
    needed = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libasciichat" not in needed  # it needs none of the other seven libraries
    assert "libasciichat_pixgrid.so" in open(os.path.join(PKG, "Makefile")).read()


def test_the_package_exports_the_binding():
    """PixGrid and pixgrid_lib leave the package where pix.py's names do"""
    assert '__all__ = ["PixGrid", "pixgrid_lib"' in open(os.path.join(PKG, "pixgrid.py")).read()
    assert "from .pixgrid import *" in open(os.path.join(PKG, "__init__.py")).read()


def test_pix_set_points_a_composite_descriptor_to_this_library():
    """asciichat_pix_set keeps refusing comp; its message names where the packed tiles of a composite go"""
    case = PS.refusal_case()
    keep, sources = PS.place_on_host(case.sources())
    frames = case.frames()
    frames[1] = PS.changed(frames[1], comp=1)
    g = PS.Handle(PS.mock_library(), 2)
    try:
        assert g.set(sources, frames) == PS.NOT_SUPPORTED and "asciichat_pixgrid" in g.error()
    finally:
        g.close()


# ---- the host code under the sanitizers, as a program of its own ------------------------------------------------------------------
def test_host_code_is_clean_under_sanitizers(tmp_path):
    """(the child inherits LD_PRELOAD as it is, neither set nor unset; should something be preloaded, the link-order check of the
    sanitizer's runtime must not end the program before it starts: its own code is instrumented all the same)"""
    exe = str(tmp_path / "pixgrid_fuzz")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ascii-chat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fuzz", "pixgrid_fuzz.c"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0")
    out = subprocess.run([exe, "4000"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "pixgrid fuzz ok" in out.stdout, out.stderr[-3000:]
