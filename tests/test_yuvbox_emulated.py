"""YUV sources box-averaged straight from their planes, without a GPU: the kernel of libasciichat_yuvbox.so under the CPU
emulator against the composition of the two restatements (tests/yuvbox_ref.py = box_ref over yuv_ref) over the shared case table
-- bytes equal, nothing stored outside an image --, again under DESC, LATE and RANDOM wave schedules and other workgroup orders,
hand-derived known answers, the host walk of the rule, every refusal at its limit and the handle's ticks through yuvbox.c itself
(over the mock HIP runtime), the rendered text against the oracle, what the library and the package export, and the host code
under the sanitizers as a program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu
import orc
import yuv_ref as YR
import yuv_support as YS
import yuvbox_ref as BR
import yuvbox_support as BS
from achip_ctypes import MODE_CAPS, MODE_HB_TRUE, MODE_NAMES, MODE_TRUE_FG, Frame
from emu_schedule import DEFAULT, Schedule, scheduled

ROOT = BS.emubuild.ROOT
PKG = os.path.join(ROOT, "ascii-chat_amd")
LIB = os.path.join(PKG, "libasciichat_yuvbox.so")
BUILD_IT = "libasciichat_yuvbox.so has not been built (make -C ascii-chat_amd)"
CASES = BS.cases()


# ---- the rule by hand ----------------------------------------------------------------------------------------------------------
# (235, 90, 240): R = (298 * 219 + 409 * 112 + 128) >> 8 = 111198 >> 8 = 434 -> 255 (the clamp), G = (65262 + 3800 - 23296 + 128) >> 8
# = 179, B = (65262 - 19608 + 128) >> 8 = 178;  (16, 90, 240): R = 45936 >> 8 = 179, G and B negative -> 0
A, B = (255, 179, 178), (179, 0, 0)
BLACK, WHITE = (0, 0, 0), (255, 255, 255)  # (16, 128, 128) and (235, 128, 128)


def _by_hand(fmt):
    """-> (yuv_ref.Source of a 2x2 image written out byte by byte, its four pixels, its 1x1 average)"""
    if fmt in YS.PLANAR:  # one chroma sample for the block: A B / B A
        chroma = [np.array([90], np.uint8), np.array([240], np.uint8)] if fmt == YR.I420 else [np.array([90, 240], np.uint8)]
        src = YR.Source(fmt, 2, 2, [np.array([235, 16, 16, 235], np.uint8)] + chroma, [2, 1, 1] if fmt == YR.I420 else [2, 2])
        # R = (255 + 179 + 179 + 255 + 2) / 4 = 217, G = (179 + 179 + 2) / 4 = 90, B = (178 + 178 + 2) / 4 = 89
        return src, [[A, B], [B, A]], (217, 90, 89)
    # a chroma sample per row: A B / black white
    rows = [90, 235, 240, 16, 128, 16, 128, 235] if fmt == YR.UYVY else [235, 90, 16, 240, 16, 128, 235, 128]
    src = YR.Source(fmt, 2, 2, [np.array(rows, np.uint8)], [4])
    # R = (255 + 179 + 0 + 255 + 2) / 4 = 172, G = (179 + 0 + 0 + 255 + 2) / 4 = 109, B = (178 + 0 + 0 + 255 + 2) / 4 = 108
    return src, [[A, B], [BLACK, WHITE]], (172, 109, 108)


def _downscale(src, out_w, out_h, flip_x=False, flip_y=False):
    """a yuv_ref.Source through the emulated asciichat_yuvbox_downscale -> the image"""
    s = YS.CSource()
    s.format, s.width, s.height = src.format, src.width, src.height
    keep = [np.ascontiguousarray(p) for p in src.planes]
    for k, p in enumerate(keep):
        s.plane[k], s.stride[k] = p.ctypes.data, src.strides[k]
    out = np.full(3 * out_w * out_h + 32, BS.FILL, np.uint8)
    assert BS.emulator().emu_yuvbox_downscale(C.byref(s), out.ctypes.data, out_w, out_h, int(flip_x), int(flip_y)) == 0
    assert (out[3 * out_w * out_h:] == BS.FILL).all()
    return out[:3 * out_w * out_h].reshape(out_h, out_w, 3).tolist()


@pytest.mark.parametrize("fmt", YS.FORMATS, ids=[YR.NAMES[f] for f in YS.FORMATS])
def test_hand_known_answers(fmt):
    assert tuple(YR.rule(235, 90, 240)) == A and tuple(YR.rule(16, 90, 240)) == B
    assert tuple(YR.rule(16, 128, 128)) == BLACK and tuple(YR.rule(235, 128, 128)) == WHITE
    src, pixels, mean = _by_hand(fmt)
    as_lists = [[list(p) for p in row] for row in pixels]
    assert YR.convert_whole(src).tolist() == as_lists
    for got in (BR.image(src, 1, 1).tolist(), _downscale(src, 1, 1)):
        assert got == [[list(mean)]]
    assert _downscale(src, 2, 2) == as_lists  # the identity is the conversion
    assert _downscale(src, 2, 2, flip_x=True) == [row[::-1] for row in as_lists]
    assert _downscale(src, 2, 2, flip_y=True) == as_lists[::-1]
    # 2x2 -> 2x1: each column's two pixels; -> 1x2: each row's
    col = lambda x: [(pixels[0][x][c] + pixels[1][x][c] + 1) // 2 for c in range(3)]  # noqa: E731
    row = lambda y: [(pixels[y][0][c] + pixels[y][1][c] + 1) // 2 for c in range(3)]  # noqa: E731
    assert _downscale(src, 2, 1) == [[col(0), col(1)]] and _downscale(src, 1, 2) == [[row(0)], [row(1)]]
    if fmt in YS.PLANAR:
        assert col(0) == [217, 90, 89] and row(1) == [217, 90, 89]
    else:
        assert col(0) == [128, 90, 89] and col(1) == [217, 128, 128] and row(0) == [217, 90, 89] and row(1) == [128, 128, 128]


# ---- the kernel under the emulator -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_images_match_the_restatement(name):
    case = CASES[name]
    buf, start, pitch = BS.emu_run(case)
    BS.check_images(name, case, buf, start, pitch)


# every case has the kernel's one barrier between the column sums and the box sums: four waves a workgroup
SCHEDULES = ([Schedule.desc()] + [Schedule.late(w, k, after) for w, k, after in ((0, 1, 0), (3, 30, 0), (1, 300, 0), (0, 30, 1), (2, 300, 1))]
             + [Schedule.random(s) for s in range(3)]
             + [Schedule().workgroups("desc"), Schedule().workgroups("shuffle", 1), Schedule.desc().workgroups("shuffle", 2),
                Schedule.random(3).workgroups("shuffle", 7)])


@pytest.mark.parametrize("name", list(CASES))
def test_images_under_other_schedules(name):
    case = CASES[name]
    for s in SCHEDULES:
        try:
            with scheduled(BS.emulator(), s) as r:
                buf, start, pitch = BS.emu_run(case)
                BS.check_images(name, case, buf, start, pitch)
        except AssertionError as e:
            raise AssertionError(f"case [{name}] under [{s}]: {e}") from None
        assert r.naps == 0, "the kernel has no polling loop"
    assert DEFAULT not in SCHEDULES


@pytest.mark.parametrize("name", [n for n in CASES if "box edges" in n or "flips 3" in n or "odd width" in n] + [BS.MIXED])
def test_host_walk_equals_the_restatement(name):
    """yuvbox.h's yuvbox_host_image (what the fuzz program walks): the same bytes, the same guard"""
    buf, start, pitch = BS.emu_run(CASES[name], host=True)
    BS.check_images(name, CASES[name], buf, start, pitch)


def test_cases_cover_what_they_claim():
    import box_ref
    for fmt in YS.FORMATS:
        n = YR.NAMES[fmt]
        s, ow, oh, _ = CASES[f"{n} 10x6 -> 4x4 box edges inside chroma blocks"].items[0]
        assert [box_ref.bounds(10, 4, x) for x in range(4)] == [(0, 2), (2, 5), (5, 7), (7, 10)]  # 5 and 7 split a pair
        assert [box_ref.bounds(6, 4, y) for y in range(4)] == [(0, 1), (1, 3), (3, 4), (4, 6)]  # rows 0|1 and 3|4 share chroma rows
        s = CASES[f"{n} 16x8 -> 5x3 the extremes of Y, U and V"].items[0][0]
        y, u, v = YR.samples(s.ref, *np.mgrid[0:16, 0:8])
        assert {0, 255} <= set(y.reshape(-1).tolist()) and 0 in u and 255 in v
        s, ow, oh, _ = CASES[f"{n} 6x4 -> 6x4 identity"].items[0]
        assert (ow, oh) == (s.width, s.height) and np.array_equal(CASES[f"{n} 6x4 -> 6x4 identity"].expected()[0], s.whole())
        flips = [CASES[f"{n} 18x7 -> 5x3 flips {fl}"] for fl in range(4)]
        assert [c.items[0][3] for c in flips] == [0, 1, 2, 3] and len({c.expected()[0].tobytes() for c in flips}) == 4
        assert np.array_equal(flips[3].expected()[0], flips[0].expected()[0][::-1, ::-1])
        for off in range(4):
            s = CASES[f"{n} 20x6 -> 5x3 planes +{off} strides +4"].items[0][0]
            assert all(a % 16 == off for a in s.at) and all(st % (2 if fmt == YR.I420 and k else 4) == 0 and st > YR.row_bytes(fmt, k, 20)
                                                        for k, st in enumerate(s.ref.strides))  # (the access: I420's chroma loads are halfwords)
        s = CASES[f"{n} 20x6 -> 5x3 planes +0 strides +1"].items[0][0]
        assert all(a % 16 == 0 for a in s.at) and all(st % 2 == 1 for st in s.ref.strides)  # an aligned base, an unaligned stride
        deep = CASES[f"{n} {BS.DEEP_WHITE}"]
        assert box_ref.bounds(600, 2, 0) == (0, 300) and 300 > 256 and 300 * 255 > 65535  # no 16-bit sum holds a box's column
        assert (deep.items[0][0].whole() == 255).all() and (deep.expected()[0] == 255).all()
        assert CASES[f"{n} 4x2160 -> 1x1"].items[0][0].height == BS.MAX_H
        assert {CASES[f"{n} 3840x2 -> {o} the widest stage"].items[0][0].width for o in ("80x1", "1x1")} == {BS.MAX_W}
    for fmt in YS.PLANAR:
        n = YR.NAMES[fmt]
        assert {w % 4 for w in (9, 10, 11)} == {1, 2, 3} and all(f"{n} {w}x4 -> 3x2 width 4k+{w % 4}" in CASES for w in (9, 10, 11))
        assert CASES[f"{n} 1031x3 -> 7x2 a second group per lane"].items[0][0].width // 4 > 256 and 1031 % 4 == 3
        up = CASES[f"{n} 3x2 -> 7x5 upscale"]
        assert all(hi - lo == 1 for lo, hi in [box_ref.bounds(3, 7, x) for x in range(7)] + [box_ref.bounds(2, 5, y) for y in range(5)])
        assert len({tuple(p) for p in up.expected()[0].reshape(-1, 3).tolist()}) <= 6  # pixels replicated
    for fmt in YR.PACKED:
        n = YR.NAMES[fmt]
        assert CASES[f"{n} 1030x2 -> 5x1 a second group per lane"].items[0][0].width // 4 > 256 and 1030 % 4 == 2
        assert all(hi - lo == 1 for lo, hi in [box_ref.bounds(4, 9, x) for x in range(9)])
    mixed = CASES[BS.MIXED]
    assert {i[0].format for i in mixed.items} == set(YS.FORMATS) and len({(i[0].width, i[0].height) for i in mixed.items}) == 4
    assert len(mixed.items) == 8 < mixed.max_frames == 12 and mixed.pitch() % 128 == 48 and {i[3] for i in mixed.items} == {0, 1, 2, 3}
    assert any(a % 4 for i in mixed.items for a in i[0].at)


# ---- the host side, through yuvbox.c over the mock runtime ----------------------------------------------------------------------------
def _host_images(case):
    buf, start, pitch = YS.image_buffer(case)
    return buf.ctypes.data + start, pitch, lambda: (buf, start)


def test_refusals_at_their_limits_and_a_refused_set_changes_nothing():
    BS.check_refusals(BS.mock_library(), BS.place_on_host, _host_images)


def test_set_check_names_the_entry():
    """yuvbox.h's check as the emulator driver exposes it: the entry, and whether the refusal is the unsupported one"""
    case = BS.refusal_case()
    keep, sources = BS.place_on_host([i[0] for i in case.items])
    frames = case.frames()

    def check(srcs, frs, n=2, max_frames=2):
        sa, fa = (YS.CSource * len(srcs))(*srcs), (Frame * len(frs))(*frs)
        bad, unsupported, why = C.c_int(-5), C.c_int(-5), C.c_char_p()
        rc = BS.emulator().emu_yuvbox_set_check(C.cast(sa, C.c_void_p), C.cast(fa, C.c_void_p), n, max_frames, C.byref(bad), C.byref(unsupported), C.byref(why))
        assert (rc == 0) == (why.value is None)
        return rc, bad.value, unsupported.value

    assert check(sources, frames) == (0, -1, 0)
    assert check(sources, [frames[0], BS.changed(frames[1], comp=1)]) == (1, 1, 1)
    assert check(sources, [BS.changed(frames[0], out_h=BS.MAX_OUT + 1), frames[1]]) == (1, 0, 0)
    assert check([sources[0], BS.changed(sources[1], width=17)], frames) == (1, 1, 0)
    assert check(sources, frames, n=3) == (1, -1, 0) and check(sources, frames, n=2, max_frames=1) == (1, -1, 0)


def test_the_handle_through_the_mock_runtime():
    """set, image_pitch, run, render_frames of yuvbox.c itself: two ticks set, run, set, run queued on one stream, the second
    with other sources at other addresses and other flips; then the mixed batch in a handle of twelve"""
    L = BS.mock_library()
    ticks = [BS.Case([(YS.Src(BS.FORMATS[i % 4], 18, 8, 800 + 10 * k + i), 5, 3, (i + k) % 4) for i in range(6)], max_frames=8) for k in range(2)]
    g = BS.Handle(L, 8)
    try:
        for k, case in enumerate(ticks):
            keep, sources = BS.place_on_host([i[0] for i in case.items])
            frames = case.frames()
            images, pitch, read = _host_images(case)
            assert g.set(sources, frames) == 0 and g.pitch() == 128 == pitch
            assert g.run(images, pitch) == 0
            BS.check_images(f"tick {k}", case, *read(), pitch)
            rc, out = g.render_frames(images, pitch, 6)
            assert rc == 0
            BS.check_render_frames(case, frames, out, images, pitch)
    finally:
        g.close()
    case = CASES[BS.MIXED]
    g = BS.Handle(L, case.max_frames)
    try:
        keep, sources = BS.place_on_host([i[0] for i in case.items])
        images, pitch, read = _host_images(case)
        assert g.set(sources, case.frames()) == 0 and g.pitch() == pitch - case.pitch_extra
        assert g.run(images, pitch) == 0
        BS.check_images(BS.MIXED, case, *read(), pitch)
    finally:
        g.close()


def test_render_frames_keeps_paddings_and_the_other_bits_of_ops():
    L = BS.mock_library()
    case = BS.refusal_case()
    keep, sources = BS.place_on_host([i[0] for i in case.items])
    frames = case.frames()
    frames[0].pad_left, frames[0].pad_top, frames[0].ops = 3, 2, 3 | 4 | 0x112233 << 8
    frames[1].ops = 2 | 64 | 16
    images, pitch, _ = _host_images(case)
    g = BS.Handle(L, 2)
    try:
        assert g.set(sources, frames) == 0
        rc, out = g.render_frames(images, pitch + 16, 2)
        assert rc == 0
        BS.check_render_frames(case, frames, out, images, pitch + 16)
        assert (out[0].pad_left, out[0].pad_top, out[0].ops, out[1].ops) == (3, 2, 4 | 0x112233 << 8, 64 | 16)
    finally:
        g.close()


# ---- end to end: the renderers over the pass's images ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [MODE_TRUE_FG, MODE_HB_TRUE], ids=["TRUE_FG", "HB_TRUE"])
def test_render_over_the_images_is_the_oracles_text_over_the_restatement(mode):
    """the oracle's text over yuvbox_ref's image equals the emulated render, under render_frames' descriptors, over the image
    the emulated pass leaves"""
    W, H = 20, 6
    cl, rm = MODE_CAPS[mode]
    out_h = 2 * H if rm == 2 else H
    case = BS.Case([(YS.Src(fmt, 64, 36, 600 + fmt), W, out_h, fmt % 4) for fmt in YS.FORMATS])
    L = BS.mock_library()
    keep, sources = BS.place_on_host([i[0] for i in case.items])
    images, pitch, read = _host_images(case)
    g = BS.Handle(L, 4)
    try:
        assert g.set(sources, case.frames()) == 0 and g.run(images, pitch) == 0
        rc, dense = g.render_frames(images, pitch, 4)
        assert rc == 0
    finally:
        g.close()
    got = emu.render_frames(mode, dense, orc.PALETTE_STANDARD, 3)
    for i, want in enumerate(case.expected()):
        text = orc.convert_with_caps(want, W, H, cl, rm, False, False, False, orc.PALETTE_STANDARD)
        assert got[i] == text and len(text) > W * H, (MODE_NAMES[mode], YR.NAMES[case.items[i][0].format])


# ---- what the library and the package export -----------------------------------------------------------------------------------------
def test_yuvbox_library_exports_only_its_interface():
    assert os.path.exists(LIB), BUILD_IT
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[-1] for l in nm.splitlines() if l.strip())
    names = ("device_count", "last_error", "create", "set", "image_pitch", "run", "render_frames", "downscale", "destroy")
    assert syms == sorted("asciichat_yuvbox_" + n for n in names), syms
    needed = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libasciichat" not in needed  # it needs none of the other four libraries
    assert "libasciichat_yuvbox.so" in open(os.path.join(PKG, "Makefile")).read()


def test_the_package_exports_the_binding():
    """YuvBox, yuvbox_downscale and yuvbox_lib leave the package where yuv.py's names do"""
    text = open(os.path.join(PKG, "yuvbox.py")).read()
    assert '__all__ = ["YuvBox", "yuvbox_downscale", "yuvbox_lib"' in text
    assert "from .yuvbox import *" in open(os.path.join(PKG, "__init__.py")).read()


# ---- the host code under the sanitizers, as a program of its own ------------------------------------------------------------------
def test_host_code_is_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "yuvbox_fuzz")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ascii-chat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fuzz", "yuvbox_fuzz.c"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([exe, "10000"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "yuvbox fuzz ok" in out.stdout, out.stderr[-3000:]
