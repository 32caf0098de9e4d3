"""YUV sources as the tiles of grid composites without a GPU: the kernel of libasciichat_yuvgrid.so under the CPU emulator against
the NumPy restatement (tests/yuvgrid_ref.py) over the shared case table -- tiles equal byte for byte, nothing stored outside them,
the descriptors rewritten in the named fields only --, the canvas and the rendered text over the rewritten descriptors against
those over the whole conversions and against the oracle, the host fill of yuvgrid_math.h, every refusal at its limit through
yuvgrid.c itself (over the mock HIP runtime), what the library exports, and the host code under the sanitizers as a program of
its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu
import orc
import yuv_ref as YR
import yuv_support as YS
import yuvgrid_ref as GR
import yuvgrid_support as GS
from achip_ctypes import MODE_HB_TRUE, MODE_MONO, MODE_NAMES, MODE_TRUE_FG

CASES = GS.cases()
ROOT = GS.emubuild.ROOT
PKG = os.path.join(ROOT, "ascii-chat_amd")
LIB = os.path.join(PKG, "libasciichat_yuvgrid.so")
PAL = orc.PALETTE_STANDARD


# ---- the restatement itself, by hand --------------------------------------------------------------------------------------------
def test_restatement_by_hand():
    """a 4x2 I420 source into a 3x2 tile: ratios 87382 and 65537 pick columns 0, 1, 2 and rows 0, 1; doubled, columns 0, 2, 3
    (the last one clamped) and rows 0, 1 (clamped)"""
    Y = np.array([[16, 81, 145, 235], [41, 106, 170, 210]], dtype=np.uint8)
    src = YR.Source(YR.I420, 4, 2, [Y.reshape(-1), np.array([128, 128], np.uint8), np.array([128, 128], np.uint8)], [4, 2, 2])
    assert (GR.ratio(4, 3), GR.ratio(2, 2)) == (87382, 65537)
    grey = lambda y: int(YR.rule(y, 128, 128)[0])  # noqa: E731
    t = GR.tile(src, 3, 2, 87382, 65537)
    assert t[:, :, 0].tolist() == [[grey(16), grey(81), grey(145)], [grey(41), grey(106), grey(170)]]
    t = GR.tile(src, 3, 2, 2 * 87382, 2 * 65537)
    assert t[:, :, 0].tolist() == [[grey(16), grey(145), grey(235)], [grey(41), grey(170), grey(210)]]
    assert GR.layout([(5, 3), (1, 1), (20, 15)]) == ([0, 48, 64], 1024) and GR.layout([]) == ([], 0) and GR.layout([(1, 1)]) == ([0], 128)


# ---- the kernel under the emulator -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_tiles_match_the_restatement(name):
    case = CASES[name]
    buf, start, p = GS.emu_run(case)
    GS.check_slab(name, case, buf, start)
    # the offsets and the slab's size, as the host lays them out
    n = len(case.comps)
    at = (C.c_uint64 * max(1, case.max_tiles))()
    total = GS.emulator().emu_yuvgrid_layout(C.cast(p.comp_ptrs, C.c_void_p), C.cast(p.nine_ptrs, C.c_void_p), n, case.max_tiles, C.cast(at, C.c_void_p))
    assert (list(at)[:len(case.tiles)], total) == case.layout(), name
    # composites(): the named fields of the YUV slots and nothing else
    tiles = buf.ctypes.data + start
    GS.check_rewrite(name, case, p.comps, GS.emu_composites(case, p, tiles), tiles)


@pytest.mark.parametrize("name", [n for n in CASES if "stride" in n or "clamp" in n] + [GS.GRID_3X3])
def test_host_fill_equals_the_restatement(name):
    """yuvgrid_math.h's host fill (what the fuzz program walks): the same bytes, the same guard"""
    buf, start, _ = GS.emu_run(CASES[name], host=True)
    GS.check_slab(name, CASES[name], buf, start)


def _canvas(comp_desc, dims):
    W, H = dims
    out = np.full(H * W * 3 + 64, 0xEE, np.uint8)
    emu.lib().emu_composite(C.byref(comp_desc), out.ctypes.data)
    assert (out[H * W * 3:] == 0xEE).all()
    return out[:H * W * 3].reshape(H, W, 3)


@pytest.mark.parametrize("name", GS.RENDERED)
def test_canvas_and_text_over_the_tiles_equal_those_over_whole_frames(name):
    """the rewritten descriptors over the tiles against the original descriptors whose sources are the whole conversions: the
    same canvas (emu_composite), the same text in TRUE_FG, HB_TRUE and MONO -- and both the oracle's"""
    case = CASES[name]
    buf, start, p = GS.emu_run(case, whole=True)
    rewritten = GS.emu_composites(case, p, buf.ctypes.data + start)
    for ci, comp in enumerate(case.comps):
        want = comp.oracle_canvas()
        if name == GS.THREE_COMPOSITES:  # made by achip_composite_setup: the oracle's own composite applies
            assert np.array_equal(want, orc.composite([s.rgb() for s in comp.slots], *comp.term)), (name, ci)
        assert want.any()
        over_tiles, over_whole = _canvas(rewritten[ci], comp.canvas), _canvas(p.whole[ci], comp.canvas)
        assert np.array_equal(over_tiles, over_whole) and np.array_equal(over_tiles, want), (name, ci)
        for mode in (MODE_TRUE_FG, MODE_HB_TRUE, MODE_MONO):
            frames = [GS.comp_frame(comp, C.addressof(rewritten[ci]), mode), GS.comp_frame(comp, C.addressof(p.whole[ci]), mode)]
            got = emu.render_frames(mode, frames, PAL, 3)
            assert got[0] == got[1] and got[0] == GS.oracle_text(want, comp.term, mode), (name, ci, MODE_NAMES[mode])
            assert len(got[0]) > 100


def test_cases_cover_what_they_claim():
    for fmt in YS.FORMATS:
        n = YR.NAMES[fmt]
        t = CASES[f"{n} 16x8 -> tile 5x3: three whole lanes and a three-pixel tail"].tiles[0]
        assert (t.tile_w, t.tile_h) == (5, 3) and 5 * 3 == 3 * 4 + 3
        y, u, v = YR.samples(t.source.ref, *np.mgrid[0:16, 0:8])
        assert {0, 255} <= set(y.reshape(-1).tolist()) and 0 in u and 255 in v  # the extremes of Y, U and V
        d = CASES[f"{n} 4x2 -> tile 9x5, both ratios doubled: into the clamp"].tiles[0]
        assert (5 * d.x_ratio) >> 16 > 3 and (3 * d.y_ratio) >> 16 > 1 and 8 * d.x_ratio < 1 << 32  # the second half: clamped, not wrapped
        assert (d.x_ratio, d.y_ratio) == (2 * GR.ratio(4, 9), 2 * GR.ratio(2, 5))
    assert 299 % 4 and 37 * 29 > 4 * 256 and 37 * 29 % 4 == 1
    s = CASES["I420 strides 24 / 13 / 11 -> tile 5x3"].tiles[0].source
    assert s.ref.strides == [24, 13, 11] and [a % 16 for a in s.at] == [1, 3, 2]
    grid = CASES[GS.GRID_3X3]
    comp = grid.comps[0]
    assert comp.n_src == 8 and comp.slots[6] is None and not comp.slots[4].yuv and len(grid.tiles) == 6
    assert {t.source.format for t in grid.tiles} == set(YS.FORMATS) and len({(t.tile_w, t.tile_h) for t in grid.tiles}) == 6
    assert any(3 * t.tile_w * t.tile_h % 16 for t in grid.tiles)  # the rounding of an offset shows
    three = CASES[GS.THREE_COMPOSITES]
    assert three.max_tiles == 64 and len(three.comps) == 3 and len({c.canvas for c in three.comps}) == 3 and len(three.tiles) == 18
    assert [sum(c.is_yuv(k) for k in range(9)) for c in three.comps] == [9, 0, 9]
    assert {id(t.source) for t in three.tiles[:9]} == {id(t.source) for t in three.tiles[9:]}  # the same nine sources
    assert not CASES[GS.NO_YUV].tiles and CASES[GS.NO_YUV].layout() == ([], 0)
    big = CASES[GS.NINE_1080P]
    assert len(big.tiles) == 9 and all((t.src_w, t.src_h, t.source.format) == (1920, 1080, YS.NV12) for t in big.tiles)
    assert big.comps[0].canvas == (160, 96) and all(t.tile_w <= 54 and t.tile_h <= 32 for t in big.tiles)


# ---- the host side, through yuvgrid.c over the mock runtime -------------------------------------------------------------------------
def _host_slab(case):
    buf, start = GS.slab(case)
    return buf.ctypes.data + start, lambda: (buf, start)


def test_refusals_at_their_limits_and_a_refused_set_changes_nothing():
    GS.check_refusals(GS.mock_library(), GS.place_on_host, _host_slab)


def test_the_handle_through_the_mock_runtime():
    """set, tiles_bytes, run, composites of yuvgrid.c itself: the 3x3 case, then a set per tick with other plane pointers keeps
    every tile where it was, then a set without YUV slots"""
    L = GS.mock_library()
    case = CASES[GS.GRID_3X3]
    g = GS.Handle(L, 9)
    try:
        for tick in range(2):
            p = GS.place_on_host(case)  # (fresh copies: other plane pointers)
            buf, start = GS.slab(case)
            assert g.set(p) == 0 and g.tiles_bytes() == case.layout()[1]
            assert g.run(buf.ctypes.data + start) == 0
            GS.check_slab(f"tick {tick}", case, buf, start)
            rc, out = g.composites(buf.ctypes.data + start, 1)
            assert rc == 0
            GS.check_rewrite(f"tick {tick}", case, p.comps, out, buf.ctypes.data + start)
        none = CASES[GS.NO_YUV]
        p = GS.place_on_host(none)
        assert g.set(p) == 0 and g.tiles_bytes() == 0 and g.run(None) == 0  # nothing to launch
        rc, out = g.composites(None, 1)
        assert rc == 0 and bytes(out[0]) == bytes(p.comps[0])
    finally:
        g.close()


# ---- what the library exports ---------------------------------------------------------------------------------------------------------
def test_yuvgrid_library_exports_only_its_interface():
    assert os.path.exists(LIB), "libasciichat_yuvgrid.so has not been built (make -C ascii-chat_amd)"
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[-1] for l in nm.splitlines() if l.strip())
    names = ("device_count", "last_error", "create", "set", "tiles_bytes", "run", "composites", "destroy")
    assert syms == sorted("asciichat_yuvgrid_" + n for n in names), syms
    needed = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libasciichat" not in needed  # it needs none of the other three libraries
    assert "libasciichat_yuvgrid.so" in open(os.path.join(PKG, "Makefile")).read()


def test_the_package_exports_the_binding():
    """YuvGrid leaves the package where yuv.py's names do"""
    assert '__all__ = ["YuvGrid"' in open(os.path.join(PKG, "yuvgrid.py")).read()
    init = open(os.path.join(PKG, "__init__.py")).read()
    assert "from .yuv import *" in init and "from .yuvgrid import *" in init


# ---- the host code under the sanitizers, as a program of its own ------------------------------------------------------------------
def test_host_code_is_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "yuvgrid_fuzz")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ascii-chat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fuzz", "yuvgrid_fuzz.c"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([exe, "10000"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "yuvgrid fuzz ok" in out.stdout, out.stderr[-3000:]
