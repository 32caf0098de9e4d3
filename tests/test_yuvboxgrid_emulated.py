"""The YUV tiles of grid composites box-averaged straight from their planes, without a GPU: the kernel of
libasciichat_yuvboxgrid.so under the CPU emulator against the composition of the restatements already in the tree
(tests/yuvbox_ref.py = box_ref over yuv_ref for the tiles, tests/yuvgrid_ref.py for the slab and the rewritten descriptors) over
the shared case table -- at every segment width of SEG_WIDTHS, under the default and under DESC, LATE and RANDOM wave schedules
with shuffled workgroup order --, hand-derived tiles, the workgroup table and the cut of a row, the host walk of the rule, the
handle's ticks and every refusal at its limit through yuvboxgrid.c itself (over the mock HIP runtime), the emulated
box_composites over the rewritten descriptors against the same over whole converted frames, what the library and the package
export, and the host code under the sanitizers as a program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import box_comp_support as CS
import yuv_ref as YR
import yuv_support as YS
import yuvgrid_ref as GR
import yuvgrid_support as GS
import yuvboxgrid_support as XS
from achip_ctypes import Composite
from emu_schedule import DEFAULT, Schedule, scheduled
from test_yuvbox_emulated import _by_hand

ROOT = XS.emubuild.ROOT
PKG = os.path.join(ROOT, "ascii-chat_amd")
LIB = os.path.join(PKG, "libasciichat_yuvboxgrid.so")
CASES = XS.cases()
NAMES = {XS.NO_SPLIT: "no split", 256: "256", 4: "4"}


# ---- the rule by hand ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", YS.FORMATS, ids=[YR.NAMES[f] for f in YS.FORMATS])
def test_hand_derived_tile(fmt):
    """test_yuvbox_emulated's 2x2 image written out byte by byte, as slot 0 of a one-slot composite with a 1x1 tile"""
    src, _, mean = _by_hand(fmt)
    assert mean == ((217, 90, 89) if fmt in YS.PLANAR else (172, 109, 108))
    s = YS.CSource()
    s.format, s.width, s.height = src.format, 2, 2
    keep = [np.ascontiguousarray(p) for p in src.planes]
    for k, p in enumerate(keep):
        s.plane[k], s.stride[k] = p.ctypes.data, src.strides[k]
    nine = (YS.CSource * 9)()
    nine[0] = s
    comp = Composite()
    comp.canvas_w = comp.canvas_h = comp.cols = comp.rows = comp.cell_w = comp.cell_h = comp.n_src = 1
    d = comp.s[0]
    d.src, d.src_w, d.src_h, d.src_stride, d.tile_w, d.tile_h = GS.PLACED, 2, 2, 6, 1, 1
    comps, nines = (C.c_void_p * 1)(C.addressof(comp)), (C.c_void_p * 1)(C.addressof(nine))
    for seg in XS.SEG_WIDTHS:
        for host in (0, 1):
            buf = np.full(48, XS.FILL, np.uint8)
            at = (-buf.ctypes.data) % 16
            assert XS.emulator().emu_yuvboxgrid_run(C.cast(comps, C.c_void_p), C.cast(nines, C.c_void_p), 1, 1, seg, buf.ctypes.data + at, host) == 0
            assert tuple(buf[at:at + 3].tolist()) == mean and (buf[:at] == XS.FILL).all() and (buf[at + 3:] == XS.FILL).all(), (seg, host)


# ---- the kernel under the emulator -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg", XS.SEG_WIDTHS, ids=[NAMES[s] for s in XS.SEG_WIDTHS])
@pytest.mark.parametrize("name", list(CASES))
def test_tiles_match_the_restatement(name, seg):
    case = CASES[name]
    buf, start, p = XS.emu_run(case, seg)
    XS.check_slab(name, case, buf, start)
    # the offsets and the slab's size: yuvgrid's layout
    lay = XS.emu_layout(case, p, seg)
    assert (lay["at"], lay["bytes"]) == case.layout(), name
    # composites(): the named fields of the YUV slots and nothing else
    tiles = buf.ctypes.data + start
    XS.check_rewrite(name, case, p.comps, XS.emu_composites(case, p, tiles), tiles)


# every case has the kernel's one barrier between the column sums and the box sums: four waves a workgroup; segments of a row
# and rows of a tile are workgroups of their own, so their order must not matter either
SCHEDULES = [Schedule.desc().workgroups("shuffle", 2), Schedule.late(3, 30, 0).workgroups("desc"), Schedule.late(0, 300, 1).workgroups("shuffle", 5),
             Schedule.random(1).workgroups("shuffle", 1), Schedule.random(3).workgroups("shuffle", 7)]


@pytest.mark.parametrize("name", list(CASES))
def test_tiles_under_other_schedules(name):
    case = CASES[name]
    for seg in XS.SEG_WIDTHS:
        for s in SCHEDULES:
            try:
                with scheduled(XS.emulator(), s) as r:
                    buf, start, _ = XS.emu_run(case, seg)
                    XS.check_slab(name, case, buf, start)
            except AssertionError as e:
                raise AssertionError(f"case [{name}] at segment width [{NAMES[seg]}] under [{s}]: {e}") from None
            assert r.naps == 0, "the kernel has no polling loop"
    assert DEFAULT not in SCHEDULES and {s.waves for s in SCHEDULES} == {"desc", "late", "random"} and all(s.wg != "asc" for s in SCHEDULES)


@pytest.mark.parametrize("name", [n for n in CASES if "box edges" in n or "upscale" in n or "strides +1" in n] + [XS.MIXED, XS.RATIOS_NOT_READ])
def test_host_walk_equals_the_restatement(name):
    """yuvboxgrid.h's yuvboxgrid_host_tile (what the fuzz program walks): the same bytes, the same guard"""
    buf, start, _ = XS.emu_run(CASES[name], host=True)
    XS.check_slab(name, CASES[name], buf, start)


# ---- the workgroup table and the cut of a row ----------------------------------------------------------------------------------------
def _check_table(name, case, seg):
    p = XS.place_on_host(case)
    lay = XS.emu_layout(case, p, seg)
    first, widest = 0, 0
    for t, tile in enumerate(case.tiles):
        segs, k = lay["segs"][t], lay["seg_out"][t]
        assert lay["first_wg"][t] == first, (name, seg, t)
        first += segs * tile.tile_h
        cut = XS.segments(tile.src_w, tile.tile_w, k)
        assert len(cut) == segs and cut[0][0] == 0 and cut[-1][1] == tile.tile_w and all(a[1] == b[0] for a, b in zip(cut, cut[1:])), (name, seg, t)
        assert all(xb - xa == k for xa, xb, _, _ in cut[:-1]) and 1 <= cut[-1][1] - cut[-1][0] <= k, (name, seg, t)
        for xa, xb, c0, c1 in cut:
            assert c0 % 4 == 0 and c0 < c1 <= tile.src_w
            staged = (c1 + 3) // 4 * 4 - c0  # the groups that touch [c0, c1) end at most three columns behind it
            assert staged <= lay["cols"][t], (name, seg, t, xa)
            widest = max(widest, staged)
            # the bound: a segment's source columns stay within the width, unless it is one box that no width can cut
            assert seg == XS.NO_SPLIT or c1 - c0 <= seg or xb - xa == 1, (name, seg, t, xa, c1 - c0)
        if seg == XS.NO_SPLIT:
            assert (segs, k) == (1, tile.tile_w)
        # the row slices: as many as keep every lane of a slice (256 / slices lanes) a group of four columns of its own
        cols, slices = lay["cols"][t], lay["slices"][t]
        assert cols % 4 == 0 and cols <= (tile.src_w + 3) // 4 * 4 and slices == (4 if cols <= 256 else 2 if cols <= 512 else 1), (name, seg, t)
    assert lay["workgroups"] == first and 0 < lay["stage_cols"] <= XS.MAX_W
    assert lay["stage_cols"] == max(c * s for c, s in zip(lay["cols"], lay["slices"]))
    return lay, widest


@pytest.mark.parametrize("seg", XS.SEG_WIDTHS + (512, 1024), ids=str)
def test_workgroup_table_and_segments(seg):
    for name, case in CASES.items():
        if case.tiles:
            _check_table(name, case, seg)


def test_mixed_set_pins_the_table_and_the_offsets():
    case = CASES[XS.MIXED]
    sizes = [(t.tile_w, t.tile_h) for t in case.tiles]
    assert sizes == [(20, 15), (7, 4), (5, 3), (19, 2), (1, 1), (9, 11), (13, 6), (20, 12), (17, 5), (8, 8), (20, 3), (24, 10)]
    lay, _ = _check_table(XS.MIXED, case, XS.NO_SPLIT)
    heights = [h for _, h in sizes]
    assert lay["first_wg"] == [sum(heights[:t]) for t in range(12)] == [0, 15, 19, 22, 24, 25, 36, 42, 54, 59, 67, 70] and lay["workgroups"] == 80
    lay, _ = _check_table(XS.MIXED, case, 4)  # a box a segment: a workgroup per tile pixel
    assert lay["segs"] == [w for w, _ in sizes] and lay["workgroups"] == sum(w * h for w, h in sizes)
    # the 16-rounded offsets: yuvgrid_ref's, and yuvgrid_fill's own for the same set (through yuvgrid's emulator driver)
    assert lay["at"] == GR.layout(sizes)[0] and any(3 * w * h % 16 for w, h in sizes)
    assert lay["at"][:6] == [0, 912, 1008, 1056, 1184, 1200]
    p = XS.place_on_host(case)
    at = (C.c_uint64 * case.max_tiles)()
    total = GS.emulator().emu_yuvgrid_layout(C.cast(p.comp_ptrs, C.c_void_p), C.cast(p.nine_ptrs, C.c_void_p), 3, case.max_tiles, C.cast(at, C.c_void_p))
    assert (list(at)[:12], total) == (lay["at"], lay["bytes"])


def test_cases_cover_what_they_claim():
    for fmt in YS.FORMATS:
        n = YR.NAMES[fmt]
        planar = fmt in YS.PLANAR
        assert [XS.bounds(10, 4, x) for x in range(4)] == [(0, 2), (2, 5), (5, 7), (7, 10)]  # 5 and 7 split a pair
        assert [XS.bounds(6, 4, y) for y in range(4)] == [(0, 1), (1, 3), (3, 4), (4, 6)]  # rows 0|1 and 3|4 share chroma rows
        wide = 1031 if planar else 1030
        t = CASES[f"{n} {wide}x3 -> tile 7x2 a second group per lane, segments start off a multiple of four"].tiles[0]
        assert t.src_w // 4 > 256 and any(XS.bounds(wide, 7, x)[0] % 4 for x in range(7))
        assert CASES[f"{n} 3840x2 -> tile 80x1 the widest source"].tiles[0].src_w == XS.MAX_W
        assert CASES[f"{n} 4x2160 -> tile 1x1 the tallest source"].tiles[0].src_h == XS.MAX_H
        up = CASES[f"{n} {'3x2' if planar else '4x2'} -> tile 7x5 upscale: every box one pixel"].tiles[0]
        assert all(hi - lo == 1 for lo, hi in [XS.bounds(up.src_w, 7, x) for x in range(7)] + [XS.bounds(2, 5, y) for y in range(5)])
        white = CASES[f"{n} 600x4 -> tile 2x2 saturating white: sums pass 16 bits"]
        assert 300 * 2 * 255 > 65535 and (white.tiles[0].source.whole() == 255).all() and (white.expected()[0] == 255).all()
        for off in range(4):
            s = CASES[f"{n} 20x6 -> tile 5x3 planes +{off} strides +4"].tiles[0].source
            assert all(a % 16 == off for a in s.at) and all(st > YR.row_bytes(fmt, k, 20) for k, st in enumerate(s.ref.strides))
        s = CASES[f"{n} 20x6 -> tile 5x3 planes +0 strides +1"].tiles[0].source
        assert all(a % 16 == 0 for a in s.at) and all(st % 2 == 1 for st in s.ref.strides)
    for fmt in YS.PLANAR:
        assert {w % 4 for w in (9, 10, 11)} == {1, 2, 3} and all(f"{YR.NAMES[fmt]} {w}x4 -> tile 3x2 width 4k+{w % 4}" in CASES for w in (9, 10, 11))
    d = CASES[XS.RATIOS_NOT_READ].tiles[0]
    assert (d.x_ratio, d.y_ratio) == (0xFFFFFFFF, 0)
    mixed = CASES[XS.MIXED]
    assert [len([s for s in c.slots if s is not None]) for c in mixed.comps] == [8, 4, 1] and [len(c.slots) for c in mixed.comps] == [9, 4, 1]
    nine = mixed.comps[0]
    assert nine.slots[6] is None and not nine.slots[4].yuv and len(mixed.tiles) == 12 < mixed.max_tiles == 20
    assert {t.source.format for t in mixed.tiles} == set(YS.FORMATS) and len({(t.src_w, t.src_h) for t in mixed.tiles}) == 4
    assert (1, 1) in {(t.tile_w, t.tile_h) for t in mixed.tiles} and len({t.tile_h for t in mixed.tiles}) > 6
    assert any(a % 4 for t in mixed.tiles for a in t.source.at)
    assert XS.emulator().emu_yuvboxgrid_seg_cols() in XS.CANDIDATES  # whichever ships, the widths above cover its code paths


# ---- the host side, through yuvboxgrid.c over the mock runtime ----------------------------------------------------------------------
def _host_slab(case):
    buf, start = XS.slab(case)
    return buf.ctypes.data + start, lambda: (buf, start)


def test_refusals_at_their_limits_and_a_refused_set_changes_nothing():
    XS.check_refusals(XS.mock_library(), XS.place_on_host, _host_slab)


def test_set_check_names_composite_and_slot():
    case = XS.refusal_case()
    p = XS.place_on_host(case)

    def check(t, n=2, max_tiles=3, seg=0):
        bad_c, bad_s, tiles, why = C.c_int(-5), C.c_int(-5), C.c_int(-5), C.c_char_p()
        rc = XS.emulator().emu_yuvboxgrid_set_check(C.cast(t.comp_ptrs, C.c_void_p), C.cast(t.nine_ptrs, C.c_void_p), n, max_tiles, seg, C.byref(bad_c),
                                                    C.byref(bad_s), C.byref(tiles), C.byref(why))
        assert (rc == 0) == (why.value is None)
        return rc, bad_c.value, bad_s.value, tiles.value

    assert check(p) == (0, -1, -1, 3) and check(p, n=1) == (0, -1, -1, 1)
    t = XS.Trial(p)
    t.comps[1].s[2].tile_h = XS.MAX_TILE + 1
    assert check(t) == (1, 1, 2, 0)
    t = XS.Trial(p)
    t.nines[0][0].width = t.comps[0].s[0].src_w = XS.MAX_W + 1
    assert check(t) == (1, 0, 0, 0)
    assert check(p, max_tiles=2) == (1, 1, 2, 0) and check(p, n=0) == (1, -1, -1, 0)


def test_the_handle_through_the_mock_runtime():
    """set, tiles_bytes, run, composites of yuvboxgrid.c itself: two ticks queued on one stream -- other planes, other formats,
    the same geometry: every tile stays where it was --, then a set without YUV slots, which launches nothing"""
    L = XS.mock_library()
    ticks = [XS.mixed_set(700), XS.mixed_set(1700, shift=1)]
    assert ticks[0].layout() == ticks[1].layout() and all(a.source.format != b.source.format for a, b in zip(ticks[0].tiles, ticks[1].tiles))
    g = XS.Handle(L, 20)
    try:
        for k, case in enumerate(ticks):
            p = XS.place_on_host(case)  # (fresh copies: other plane pointers)
            buf, start = XS.slab(case)
            tiles = buf.ctypes.data + start
            assert g.set(p) == 0 and g.tiles_bytes() == case.layout()[1]
            assert g.run(tiles) == 0
            XS.check_slab(f"tick {k}", case, buf, start)
            rc, out = g.composites(tiles, 3)
            assert rc == 0
            XS.check_rewrite(f"tick {k}", case, p.comps, out, tiles)
        # a refused set leaves the previous set's run intact
        bad = XS.Trial(p)
        bad.comps[0].s[0].tile_w = 0
        buf, start = XS.slab(case)
        assert g.set(bad) == XS.INVALID and "composite 0 slot 0" in g.error() and g.run(buf.ctypes.data + start) == 0
        XS.check_slab("after a refused set", case, buf, start)
        none = XS.BoxGridCase([XS.Comp((20, 16), (1, 1), (20, 16), [XS.Slot(XS.orc.frame_hash_noise(8, 6, 880), 20, 15, 0, 0)])])
        p = XS.place_on_host(none)
        guard, start = XS.slab(ticks[0])
        assert g.set(p) == 0 and g.tiles_bytes() == 0 and g.run(None) == 0 and g.run(guard.ctypes.data + start) == 0  # nothing to launch
        assert (guard == XS.FILL).all()
        rc, out = g.composites(None, 1)
        assert rc == 0 and bytes(out[0]) == bytes(p.comps[0])
    finally:
        g.close()


# ---- end to end: box_composites over the rewritten descriptors ----------------------------------------------------------------------
def test_box_composites_over_the_tiles_equals_box_composites_over_whole_frames():
    """use (b) of the header: one composite of four mixed-format 64x36 sources, canvas 40x24, averaged to 20x12 -- the emulated
    asciichat_hip_box_composites over the rewritten descriptors against the same over the descriptors whose sources are
    yuv_ref.convert_whole's frames"""
    srcs = [YS.Src(fmt, 64, 36, 600 + fmt, offs=(fmt, 0, (fmt + 1) % 4)) for fmt in YS.FORMATS]
    comp = GS.from_setup(srcs, (40, 12))
    assert comp.canvas == (40, 24) and len(comp.slots) == 4
    case = XS.BoxGridCase([comp])
    L = XS.mock_library()
    g = XS.Handle(L, 4)
    try:
        p = XS.place_on_host(case, whole=True)
        buf, start = XS.slab(case)
        tiles = buf.ctypes.data + start
        assert g.set(p) == 0 and g.run(tiles) == 0
        rc, rewritten = g.composites(tiles, 1)
        assert rc == 0
    finally:
        g.close()
    XS.check_slab("four sources", case, buf, start)
    for s in srcs:
        assert np.array_equal(s.whole(), YR.convert_whole(s.ref))
    images = []
    for desc in (rewritten[0], p.whole[0]):
        got, pitch, counts = CS.emu_run([CS.frame_for(desc, 20, 12)], [desc])
        assert (got[3 * 20 * 12:] == CS.BS.FILL).all() and counts["tiles"] == 4
        images.append(got[:3 * 20 * 12].copy())
    assert np.array_equal(images[0], images[1]) and len(set(images[0].tolist())) > 50


# ---- what the library and the package export -----------------------------------------------------------------------------------------
def test_yuvboxgrid_library_exports_only_its_interface():
    assert os.path.exists(LIB), "libasciichat_yuvboxgrid.so has not been built (make -C ascii-chat_amd)"
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[-1] for l in nm.splitlines() if l.strip())
    assert len(XS.NAMES) == 8 and syms == sorted("asciichat_yuvboxgrid_" + n for n in XS.NAMES), syms
    needed = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libasciichat" not in needed  # it needs none of the other five libraries
    assert "libasciichat_yuvboxgrid.so" in open(os.path.join(PKG, "Makefile")).read()


def test_the_package_exports_the_binding():
    """YuvBoxGrid and yuvboxgrid_lib leave the package where yuvgrid.py's names do"""
    assert '__all__ = ["YuvBoxGrid", "yuvboxgrid_lib"' in open(os.path.join(PKG, "yuvboxgrid.py")).read()
    assert "from .yuvboxgrid import *" in open(os.path.join(PKG, "__init__.py")).read()


# ---- the host code under the sanitizers, as a program of its own ------------------------------------------------------------------
def test_host_code_is_clean_under_sanitizers(tmp_path):
    """(the child inherits LD_PRELOAD as it is, neither set nor unset; should something be preloaded, the link-order check of the
    sanitizer's runtime must not end the program before it starts: its own code is instrumented all the same)"""
    exe = str(tmp_path / "yuvboxgrid_fuzz")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ascii-chat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fuzz", "yuvboxgrid_fuzz.c"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0")
    out = subprocess.run([exe, "6000"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "yuvboxgrid fuzz ok" in out.stdout, out.stderr[-3000:]
