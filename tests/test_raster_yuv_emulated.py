"""The rasteriser's YUV 4:2:0 output without a GPU: draw_yuv_kernel under the CPU emulator against the restatement (bytes equal,
nothing stored outside an image), the conversion arithmetic over every input, what libasciichat_raster.so decides before it
needs a device, and what the two libraries export."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import raster_support as RS
import raster_yuv_ref as YR
import raster_yuv_support as YS

CASES = YS.cases()
INVALID = 86


# ---- the kernel under the emulator ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(YS.LAYOUTS))
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_restatement(name, layout):
    case = CASES[name]
    planes, start, pitch, status = YS.emu_run(case, YS.LAYOUTS[layout])
    YS.check(name, case, YS.LAYOUTS[layout], planes, start, pitch, status)


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("name", ["yuv division pin", "yuv cell 32x64 2x2", "yuv three cell rows 2x4", "yuv tile edges 514x4"])
def test_kernel_with_a_given_number_of_workgroups_per_strip(name, split):
    """a small batch spreads a strip's slots over as many workgroups as they fill, so no thread gets a second slot; here one
    workgroup walks them all as in a large batch, and three share them unevenly"""
    case = CASES[name]
    planes, start, pitch, status = YS.emu_run(case, YR.I420, split=split)
    YS.check(name, case, YR.I420, planes, start, pitch, status)


def test_cases_cover_what_they_claim():
    T = YS.tile_px()
    sizes = {name: YS.size_px(c) for name, c in CASES.items()}
    assert all(w % 2 == 0 and h % 2 == 0 for w, h in sizes.values())
    assert sizes["yuv smallest image"] == (2, 2) and sizes["yuv odd plane starts"] == (6, 2) and 6 * 2 * 5 // 4 == 15
    assert sizes["yuv chroma across four cells"] == (20, 14)
    assert sizes["yuv three cell rows 2x4"] == (10, 28) and sizes["yuv three cell rows 2x2"] == (10, 14)
    assert sizes["yuv odd width, even height"] == (20, 24) and sizes["yuv even width, odd height"] == (24, 22)
    # a second and a third tile, a last lane with one block, and one tile not filled
    assert {T + 2, 2 * T + 2, T - 2} == {w for n, (w, _) in sizes.items() if n.startswith("yuv tile edges")}
    assert (T + 2) % 4 == 2 and 2 * T + 2 <= 1024
    # the flag frames set every flag, and NO_FRAME is in the batch
    st = {s for _, s in YS.expected("yuv flags", CASES["yuv flags"], YR.I420)}
    assert {1, 2, 4, 8, 16} <= st
    assert None in CASES["yuv batch of 40"].frames and b"" in CASES["yuv batch of 40"].frames
    # the staged atlas and the atlas read through memory both occur
    assert any(c.l2 for c in CASES.values()) and RS.ATLASES["big"].coverage.size > 32768 >= RS.ATLASES["synth58"].coverage.size


# ---- the conversion, through the driver -------------------------------------------------------------------------------------
def _convert(r, g, b):
    out = (C.c_int32 * 3)()
    YS.emulator().emu_raster_yuv_convert(r, g, b, out)
    return tuple(out)


def test_conversion_over_every_input():
    n = 1 << 24
    y, u, v = (np.empty(n, dtype=np.int32) for _ in range(3))
    YS.emulator().emu_raster_yuv_all(y.ctypes.data, u.ctypes.data, v.ctypes.data)
    i = np.arange(n, dtype=np.int64)
    r, g, b = i >> 16, (i >> 8) & 255, i & 255
    assert np.array_equal(y, YR.luma(r, g, b))
    ru, rv = YR.chroma(r, g, b)  # (with the reference's clamps: equal to the unclamped device values only if they never act)
    assert np.array_equal(u, ru) and np.array_equal(v, rv)
    assert (int(y.min()), int(y.max())) == (16, 235)
    assert (int(u.min()), int(u.max())) == (16, 240) and (int(v.min()), int(v.max())) == (16, 240)


@pytest.mark.parametrize("rgb, yuv", [((0, 0, 0), (16, 128, 128)),        # 128 >> 8 = 0 everywhere
                                      ((255, 255, 255), (235, 128, 128)),  # (220 * 255 + 128) >> 8 = 219; the chroma weights sum to 0
                                      ((255, 0, 0), (82, 90, 240)),        # 16958 >> 8 = 66; -9562 >> 8 = -38; 28688 >> 8 = 112
                                      ((0, 255, 0), (144, 54, 34)),        # 33023 >> 8 = 128; -18742 >> 8 = -74; -23842 >> 8 = -94
                                      ((0, 0, 255), (41, 240, 110))])      # 6503 >> 8 = 25; 28688 >> 8 = 112; -4462 >> 8 = -18
def test_conversion_by_hand(rgb, yuv):
    assert _convert(*rgb) == yuv
    img = np.array([[list(rgb) + [7]] * 2] * 2, dtype=np.uint8)  # a 2x2 image of the colour; the alpha plays no part
    assert YR.yuv420(img, YR.I420).tolist() == [yuv[0]] * 4 + [yuv[1], yuv[2]]
    assert YR.yuv420(img, YR.NV12).tolist() == [yuv[0]] * 4 + [yuv[1], yuv[2]]


def test_block_average_truncates():
    avg = YS.emulator().emu_raster_yuv_avg
    assert [avg(s) for s in (0, 1, 2, 3, 4, 1019, 1020)] == [0, 0, 0, 0, 1, 254, 255]
    block = np.array([[255, 255], [255, 254]], dtype=np.int64)
    assert YR.block_average(block).tolist() == [[254]] and YR.block_average(np.array([[1, 1], [1, 0]])).tolist() == [[0]]


def test_restatement_layouts_by_hand():
    # 4x2: left block red, right block blue -> Y rows, then U U V V (I420) or U V U V (NV12)
    img = np.zeros((2, 4, 4), dtype=np.uint8)
    img[:, :2, 0], img[:, 2:, 2] = 255, 255
    assert YR.yuv420(img, YR.I420).tolist() == [82, 82, 41, 41] * 2 + [90, 240] + [240, 110]
    assert YR.yuv420(img, YR.NV12).tolist() == [82, 82, 41, 41] * 2 + [90, 240, 240, 110]


# ---- the host, before it needs a device -------------------------------------------------------------------------------------
def _lib():
    L = C.CDLL(RS.LIB)
    L.asciichat_raster_yuv420_bytes.restype = C.c_size_t
    L.asciichat_raster_yuv420_bytes.argtypes = [C.c_int, C.c_int]
    L.asciichat_raster_yuv420_pitch.restype = C.c_size_t
    L.asciichat_raster_yuv420_pitch.argtypes = [C.c_void_p]
    vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
    L.asciichat_raster_run_yuv420.restype = ci
    L.asciichat_raster_run_yuv420.argtypes = [vp, vp, sz, vp, ci, vp, sz, ci, vp, vp]
    L.asciichat_raster_draw_yuv420.restype = ci
    L.asciichat_raster_draw_yuv420.argtypes = [vp, ci, vp, sz, ci, vp]
    return L


def test_sizes_and_null_handles_need_no_device():
    L = _lib()
    size = L.asciichat_raster_yuv420_bytes
    assert size(2, 2) == 6 and size(20, 14) == 420
    assert [size(w, h) for w, h in ((3, 2), (2, 3), (0, 2), (1, 1), (-2, 2), (2, -2))] == [0] * 6
    assert size(32768, 32768) == 32768 * 32768 * 3 // 2  # the largest image a handle can have: no 32-bit product
    assert L.asciichat_raster_yuv420_pitch(None) == 0
    buf = (C.c_uint8 * 64)()
    assert L.asciichat_raster_run_yuv420(None, buf, 16, buf, 1, buf, 8, YR.I420, buf, None) == INVALID
    assert L.asciichat_raster_draw_yuv420(None, 1, buf, 8, YR.NV12, None) == INVALID


# ---- what the libraries export ----------------------------------------------------------------------------------------------
def _exports(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in nm.splitlines() if l.strip())


def test_raster_library_exports_its_interface_with_the_yuv_entries():
    syms = _exports(RS.LIB)
    assert syms and all(s.startswith("asciichat_raster_") for s in syms), syms
    for name in ("yuv420_bytes", "yuv420_pitch", "run_yuv420", "draw_yuv420"):
        assert "asciichat_raster_" + name in syms


def test_hip_library_exports_what_it_exported_before():
    with open(os.path.join(RS.ROOT, "tests", "golden", "hip_exports.txt")) as f:
        before = f.read().split()
    assert _exports(RS.HIP_LIB) == before
