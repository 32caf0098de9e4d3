"""Packed RGB sources (RGB24, RGBA, BGR24, BGRA) without a GPU: the three kernels of libasciichat_pix.so under the CPU emulator
against the NumPy restatement (tests/pix_ref.py) over the shared case table -- bytes equal, nothing stored outside an image --,
the box cases again under DESC, LATE and RANDOM wave schedules and other workgroup orders, hand-written known answers, the host
walks of the rule, every refusal at its limit and the handle's ticks through pix.c itself (over the mock HIP runtime), the
rendered text against the oracle, what the library and the package export, and the host code under the sanitizers as a program
of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import box_ref
import emu
import orc
import pix_ref as PR
import pix_support as PS
from achip_ctypes import MODE_CAPS, MODE_HB_TRUE, MODE_NAMES, MODE_TRUE_FG, Frame
from emu_schedule import DEFAULT, Schedule, scheduled

ROOT = PS.emubuild.ROOT
PKG = os.path.join(ROOT, "ascii-chat_amd")
LIB = os.path.join(PKG, "libasciichat_pix.so")
BUILD_IT = "libasciichat_pix.so has not been built (make -C ascii-chat_amd)"
CASES = PS.cases()
WHOLE = PS.whole_cases()
FMT_IDS = [PR.NAMES[f] for f in PR.FORMATS]


# ---- the rule by hand ----------------------------------------------------------------------------------------------------------
# a 2 x 2 image: (10, 20, 30) (200, 100, 50) / (255, 0, 1) (7, 8, 9), written out byte by byte in each layout; alpha bytes that
# would show were they read
BY_HAND = {
    PR.RGB: [10, 20, 30, 200, 100, 50, 255, 0, 1, 7, 8, 9],
    PR.RGBA: [10, 20, 30, 0xAA, 200, 100, 50, 0xBB, 255, 0, 1, 0xCC, 7, 8, 9, 0xDD],
    PR.BGR: [30, 20, 10, 50, 100, 200, 1, 0, 255, 9, 8, 7],
    PR.BGRA: [30, 20, 10, 0xAA, 50, 100, 200, 0xBB, 1, 0, 255, 0xCC, 9, 8, 7, 0xDD],
}
PIXELS = [[[10, 20, 30], [200, 100, 50]], [[255, 0, 1], [7, 8, 9]]]
MEAN = [118, 32, 23]  # (10 + 200 + 255 + 7 + 2) / 4 = 118, (20 + 100 + 0 + 8 + 2) / 4 = 32, (30 + 50 + 1 + 9 + 2) / 4 = 23
COLS = [[133, 10, 16], [104, 54, 30]]  # 2x2 -> 2x1: (10 + 255 + 1) / 2, (20 + 0 + 1) / 2, (30 + 1 + 1) / 2; (200 + 7 + 1) / 2, 54, 30
ROWS = [[105, 60, 40], [131, 4, 5]]  # 2x2 -> 1x2: (10 + 200 + 1) / 2, (120 + 1) / 2, (80 + 1) / 2; (255 + 7 + 1) / 2, (8 + 1) / 2, (10 + 1) / 2


def _hand_source(fmt):
    """-> (array to keep alive, the structure over exactly the bytes of BY_HAND)"""
    data = np.array(BY_HAND[fmt], dtype=np.uint8)
    s = PS.CSource()
    s.format, s.width, s.height, s.pixels, s.stride = fmt, 2, 2, data.ctypes.data, 0
    return data, s


def _downscale(s, out_w, out_h, flip_x=False, flip_y=False):
    out = np.full(3 * out_w * out_h + 32, PS.FILL, np.uint8)
    assert PS.emulator().emu_pix_downscale(C.byref(s), out.ctypes.data, out_w, out_h, int(flip_x), int(flip_y)) == 0
    assert (out[3 * out_w * out_h:] == PS.FILL).all()
    return out[:3 * out_w * out_h].reshape(out_h, out_w, 3).tolist()


@pytest.mark.parametrize("fmt", PR.FORMATS, ids=FMT_IDS)
def test_hand_known_answers(fmt):
    data, s = _hand_source(fmt)
    assert PR.whole(data, fmt, 2, 2).tolist() == PIXELS
    for run in PS.RUNS:
        out = np.full(12 + 32, PS.FILL, np.uint8)
        assert PS.emulator(run).emu_pix_convert(C.byref(s), out.ctypes.data, 0) == 0
        assert out[:12].reshape(2, 2, 3).tolist() == PIXELS and (out[12:] == PS.FILL).all()
    assert PR.box(np.array(PIXELS, np.uint8), 1, 1).tolist() == [[MEAN]] and _downscale(s, 1, 1) == [[MEAN]]
    assert _downscale(s, 2, 2) == PIXELS  # the identity is the conversion
    assert _downscale(s, 2, 2, flip_x=True) == [row[::-1] for row in PIXELS]
    assert _downscale(s, 2, 2, flip_y=True) == PIXELS[::-1]
    assert _downscale(s, 2, 1) == [COLS] and _downscale(s, 1, 2) == [[ROWS[0]], [ROWS[1]]]
    assert _downscale(s, 2, 1, flip_x=True) == [COLS[::-1]] and _downscale(s, 1, 2, flip_y=True) == [[ROWS[1]], [ROWS[0]]]
    # the sampled pass: identity, and each flip of the descriptor
    for fl, want in ((0, PIXELS), (1, [row[::-1] for row in PIXELS]), (2, PIXELS[::-1]), (3, [row[::-1] for row in PIXELS[::-1]])):
        f = Frame()
        f.src_w, f.src_h, f.out_w, f.out_h, f.x_ratio, f.y_ratio, f.ops = 2, 2, 2, 2, 65537, 65537, fl
        out = np.full(64 + 16, PS.FILL, np.uint8)
        at = (-out.ctypes.data) % 16
        assert PS.emulator().emu_pix_run(C.addressof(s), C.addressof(f), 1, 1, out.ctypes.data + at, 16, 0, 0) == 0
        assert out[at:at + 12].reshape(2, 2, 3).tolist() == want and (out[at + 12:] == PS.FILL).all(), fl


def test_box_bounds_are_the_box_passes():
    """pix_math.h restates achip_box_bounds: pinned against box_ref.bounds, which tests/test_box_emulated.py pins against that"""
    lo, hi = C.c_uint32(), C.c_uint32()
    for src, out in ((1, 1), (2, 5), (5, 2), (30, 7), (64, 1), (3840, 80), (3840, 16384), (2160, 24), (1080, 1080), (7, 7), (3, 16384)):
        for i in sorted({0, 1, out // 2, out - 2, out - 1} & set(range(out))):
            PS.emulator().emu_pix_bounds(src, out, i, C.byref(lo), C.byref(hi))
            assert (lo.value, hi.value) == box_ref.bounds(src, out, i), (src, out, i)


# ---- the kernels under the emulator -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_sampled_images_match_the_restatement(name):
    buf, start, pitch = PS.emu_run(CASES[name], "run")
    PS.check_images(name, CASES[name], "run", buf, start, pitch)


@pytest.mark.parametrize("name", list(CASES))
def test_box_images_match_the_restatement(name):
    buf, start, pitch = PS.emu_run(CASES[name], "box")
    PS.check_images(name, CASES[name], "box", buf, start, pitch)


@pytest.mark.parametrize("run", PS.RUNS)
@pytest.mark.parametrize("fmt", PR.FORMATS, ids=FMT_IDS)
def test_whole_conversions_match_the_restatement(fmt, run):
    for name, case in WHOLE[fmt].items():
        buf, start = PS.emu_convert(case, run)
        PS.check_whole(f"{PR.NAMES[fmt]} {name} (runs of {run})", case.src, buf, start, case.row_stride())


@pytest.mark.parametrize("run", PS.RUNS)
def test_run_whole_of_a_mixed_batch(run):
    srcs = PS.whole_batch()
    buf, start, pitch = PS.emu_run_whole(srcs, run, max_frames=len(srcs) + 3)
    PS.check_batch(f"run_whole (runs of {run})", srcs, buf, start, pitch)
    assert {s.format for s in srcs} == set(PR.FORMATS) and start % 4 == 3


# every box case has the kernel's one barrier between the column sums and the box sums: four waves a workgroup
SCHEDULES = ([Schedule.desc()] + [Schedule.late(w, k, after) for w, k, after in ((0, 1, 0), (3, 30, 0), (1, 300, 0), (0, 30, 1), (2, 300, 1))]
             + [Schedule.random(s) for s in range(3)]
             + [Schedule().workgroups("desc"), Schedule().workgroups("shuffle", 1), Schedule.desc().workgroups("shuffle", 2),
                Schedule.random(3).workgroups("shuffle", 7)])


@pytest.mark.parametrize("name", list(CASES))
def test_box_images_under_other_schedules(name):
    case = CASES[name]
    for s in SCHEDULES:
        try:
            with scheduled(PS.emulator(), s) as r:
                buf, start, pitch = PS.emu_run(case, "box")
                PS.check_images(name, case, "box", buf, start, pitch)
        except AssertionError as e:
            raise AssertionError(f"case [{name}] under [{s}]: {e}") from None
        assert r.naps == 0, "the kernel has no polling loop"
    assert DEFAULT not in SCHEDULES


HOST_WALKED = [n for n in CASES if "flips 3" in n or "base +3" in n or "upscale" in n or "ramp in channel 0 256x1 -> 64x1" in n] + [PS.MIXED]


@pytest.mark.parametrize("name", HOST_WALKED)
def test_host_walks_equal_the_restatement(name):
    """pix.h's pix_host_sample and pix_host_box (what the fuzz program walks): the same bytes, the same guard"""
    for kind in ("run", "box"):
        buf, start, pitch = PS.emu_run(CASES[name], kind, host=True)
        PS.check_images(name, CASES[name], kind, buf, start, pitch)


def test_host_walk_of_the_whole_conversion():
    srcs = PS.whole_batch()
    buf, start, pitch = PS.emu_run_whole(srcs, host=True)
    PS.check_batch("pix_host_whole", srcs, buf, start, pitch)


def test_run_whole_then_box_ref_is_run_box():
    """the definition of run_box, with the kernels on both sides: box_ref over what run_whole leaves equals what run_box leaves"""
    case = CASES[PS.MIXED]
    srcs = case.sources()
    wbuf, wstart, wpitch = PS.emu_run_whole(srcs)
    bbuf, bstart, bpitch = PS.emu_run(case, "box")
    for i, (s, ow, oh, fl) in enumerate(case.items):
        whole = wbuf[wstart + i * wpitch:wstart + i * wpitch + 3 * s.width * s.height].reshape(s.height, s.width, 3)
        want = box_ref.box_ref(whole, ow, oh, bool(fl & 1), bool(fl & 2))
        assert np.array_equal(bbuf[bstart + i * bpitch:bstart + i * bpitch + want.size], want.reshape(-1)), i


def test_cases_cover_what_they_claim():
    for fmt in PR.FORMATS:
        n, bpp = PR.NAMES[fmt], PR.BPP[fmt]
        assert {w % 4 for w in (4, 5, 6, 7)} == {0, 1, 2, 3} and all(f"{n} {w}x2 -> 3x2 width 4k+{w % 4}" in CASES for w in (4, 5, 6, 7))
        paths = set()
        for off, kind in PS.ALIGNMENTS:
            s = CASES[f"{n} 20x3 -> 7x2 base +{off} stride {kind}"].items[0][0]
            assert s.at % 16 == off and s.stride > bpp * 20 and s.stride % 16 == {"16": 0, "4": 4, "1": 1}[kind]
            both = s.at | s.stride
            paths.add("16" if both % 16 == 0 else "4" if both % 4 == 0 else "1")
        assert paths == {"16", "4", "1"} and {o for o, _ in PS.ALIGNMENTS} == set(range(16))
        flips = [CASES[f"{n} 30x17 -> 7x4 flips {fl}"] for fl in range(4)]
        for kind in ("run", "box"):
            assert len({c.expected(kind)[0].tobytes() for c in flips}) == 4
        assert np.array_equal(flips[3].expected("box")[0], flips[0].expected("box")[0][::-1, ::-1]) and 30 % 7
        ident = CASES[f"{n} 6x4 -> 6x4 identity"]
        assert all(np.array_equal(ident.expected(k)[0], ident.items[0][0].whole()) for k in ("run", "box"))
        assert all(hi - lo == 1 for lo, hi in [box_ref.bounds(5, 11, x) for x in range(11)] + [box_ref.bounds(3, 7, y) for y in range(7)])
        assert CASES[f"{n} 3840x2 -> 80x1 the widest stage"].items[0][0].width == PS.BOX_W
        assert CASES[f"{n} 1031x3 -> 7x2 a second group per lane"].items[0][0].width // 4 > 256 and 1031 % 4 == 3
        assert 37 * 29 > 4 * 256  # more samples than one workgroup's lanes take
        for ch in range(3):
            w = CASES[f"{n} ramp in channel {ch} 256x1 -> 256x1"].items[0][0]
            assert w.whole()[0, :, ch].tolist() == list(range(256)) and all((w.whole()[0, :, c] == (0x11, 0x22, 0x33)[c]).all() for c in range(3) if c != ch)
            if bpp == 4:
                assert (w.image[w.at + 3:w.at + 4 * 256:4] == 0x44).all()
    counts = {(i[1] * i[2]) % 4 for c in CASES.values() for i in c.items}
    assert counts == {0, 1, 2, 3}  # an image whose pixel count is 0, 1, 2 and 3 mod 4
    mixed = CASES[PS.MIXED]
    assert {i[0].format for i in mixed.items} == set(PR.FORMATS) and len({(i[0].width, i[0].height) for i in mixed.items}) == 4
    assert len(mixed.items) == 8 < mixed.max_frames == 12 and mixed.pitch() % 128 == 48 and {i[3] for i in mixed.items} == {0, 1, 2, 3}
    for fmt in PR.FORMATS:
        names = list(WHOLE[fmt])
        assert {int(x.split("dst +")[1].split()[0]) % 4 for x in names if "dst +" in x} == {0, 1, 2, 3} and any("rgb_stride 55" in x for x in names)


# ---- the host side, through pix.c over the mock runtime ----------------------------------------------------------------------------
def _host_images(case):
    buf, start, pitch = PS.image_buffer(case)
    return buf.ctypes.data + start, pitch, lambda: (buf, start)


def test_refusals_at_their_limits_and_a_refused_set_changes_nothing():
    PS.check_refusals(PS.mock_library(), PS.place_on_host, _host_images)


def test_a_source_too_large_for_the_box_pass_is_refused_by_run_box_alone():
    g, keep, wide = PS.check_too_large_for_the_box(PS.mock_library(), PS.place_on_host, _host_images)
    try:
        buf, start, pitch = PS.batch_buffer(wide.sources())
        assert g.whole_pitch() == pitch - 48 and g.run_whole(buf.ctypes.data + start, pitch) == 0
        PS.check_batch("3841x1 run_whole", wide.sources(), buf, start, pitch)
    finally:
        g.close()


def test_set_check_names_the_entry():
    """pix_math.h's check as the emulator driver exposes it: the entry, and whether the refusal is the unsupported one"""
    case = PS.refusal_case()
    keep, sources = PS.place_on_host(case.sources())
    frames = case.frames()

    def check(srcs, frs, n=2, max_frames=2):
        sa = (PS.CSource * len(srcs))(*srcs)
        fa = (Frame * len(frs))(*frs) if frs is not None else None
        bad, unsupported, why = C.c_int(-5), C.c_int(-5), C.c_char_p()
        rc = PS.emulator().emu_pix_set_check(C.cast(sa, C.c_void_p), C.cast(fa, C.c_void_p) if fa is not None else None, n, max_frames, C.byref(bad),
                                             C.byref(unsupported), C.byref(why))
        assert (rc == 0) == (why.value is None)
        return rc, bad.value, unsupported.value

    assert check(sources, frames) == (0, -1, 0) and check(sources, None) == (0, -1, 0)
    assert check(sources, [frames[0], PS.changed(frames[1], comp=1)]) == (1, 1, 1)
    assert check(sources, [PS.changed(frames[0], out_h=0), frames[1]]) == (1, 0, 0)
    assert check([sources[0], PS.changed(sources[1], width=0)], frames) == (1, 1, 0)
    assert check(sources, frames, n=3) == (1, -1, 0) and check(sources, frames, n=2, max_frames=1) == (1, -1, 0)


def test_the_handle_through_the_mock_runtime():
    """set, the pitches, run, run_box, run_whole, render_frames of pix.c itself: two ticks queued on one stream, the second with
    other sources at other addresses and other flips; then the mixed batch in a handle of twelve"""
    L = PS.mock_library()
    ticks = [PS.Case([(PS.Src(PR.FORMATS[i % 4], 18, 8, 800 + 10 * k + i, off=(i + k) % 16), 5, 3, (i + k) % 4) for i in range(6)], max_frames=8) for k in range(2)]
    g = PS.Handle(L, 8)
    try:
        for k, case in enumerate(ticks):
            keep, sources = PS.place_on_host(case.sources())
            frames = case.frames()
            assert g.set(sources, frames) == 0
            for kind in ("run", "box"):
                images, pitch, read = _host_images(case)
                assert g.pitch() == 128 == pitch and g.run(images, pitch, kind) == 0
                PS.check_images(f"tick {k}", case, kind, *read(), pitch)
                rc, out = g.render_frames(images, pitch, 6)
                assert rc == 0
                PS.check_render_frames(frames, out, images, pitch)
            buf, start, wpitch = PS.batch_buffer(case.sources())
            assert g.whole_pitch() == 512 and g.run_whole(buf.ctypes.data + start, wpitch) == 0
            PS.check_batch(f"tick {k} whole", case.sources(), buf, start, wpitch)
    finally:
        g.close()
    case = CASES[PS.MIXED]
    g = PS.Handle(L, case.max_frames)
    try:
        keep, sources = PS.place_on_host(case.sources())
        assert g.set(sources, case.frames()) == 0 and g.pitch() == case.pitch() - case.pitch_extra
        for kind in ("run", "box"):
            images, pitch, read = _host_images(case)
            assert g.run(images, pitch, kind) == 0
            PS.check_images(PS.MIXED, case, kind, *read(), pitch)
    finally:
        g.close()


def test_render_frames_keeps_paddings_and_the_other_bits_of_ops():
    L = PS.mock_library()
    case = PS.refusal_case()
    keep, sources = PS.place_on_host(case.sources())
    frames = case.frames()
    frames[0].pad_left, frames[0].pad_top, frames[0].ops = 3, 2, 3 | 4 | 0x112233 << 8
    frames[1].ops = 2 | 64 | 16
    images, pitch, _ = _host_images(case)
    g = PS.Handle(L, 2)
    try:
        assert g.set(sources, frames) == 0
        rc, out = g.render_frames(images, pitch + 16, 2)
        assert rc == 0
        PS.check_render_frames(frames, out, images, pitch + 16)
        assert (out[0].pad_left, out[0].pad_top, out[0].ops, out[1].ops) == (3, 2, 4 | 0x112233 << 8, 64 | 16)
    finally:
        g.close()


# ---- end to end: the renderers over the pass's images ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [MODE_TRUE_FG, MODE_HB_TRUE], ids=["TRUE_FG", "HB_TRUE"])
def test_render_over_the_sampled_images_is_the_oracles_text_over_the_converted_frame(mode):
    """the conversion commutes with the sampling: the emulated render, under render_frames' descriptors, over the images the
    emulated run leaves equals the oracle's text over the wholly converted frame; and over run_box's images the oracle's text
    over the restatement's averaged image"""
    W, H = 20, 6
    cl, rm = MODE_CAPS[mode]
    out_h = 2 * H if rm == 2 else H
    case = PS.Case([(PS.Src(fmt, 64, 36, 600 + fmt, stride=PR.BPP[fmt] * 64 + 4 * fmt, off=fmt), W, out_h) for fmt in PR.FORMATS])
    L = PS.mock_library()
    keep, sources = PS.place_on_host(case.sources())
    g = PS.Handle(L, 4)
    try:
        assert g.set(sources, case.frames()) == 0
        for kind in ("run", "box"):
            images, pitch, read = _host_images(case)
            assert g.run(images, pitch, kind) == 0
            rc, dense = g.render_frames(images, pitch, 4)
            assert rc == 0
            got = emu.render_frames(mode, dense, orc.PALETTE_STANDARD, 3)
            for i, (s, _, _, _) in enumerate(case.items):
                img = s.whole() if kind == "run" else case.expected("box")[i]
                text = orc.convert_with_caps(img, W, H, cl, rm, False, False, False, orc.PALETTE_STANDARD)
                assert got[i] == text and len(text) > W * H, (MODE_NAMES[mode], kind, PR.NAMES[s.format])
    finally:
        g.close()


# ---- what the library and the package export -----------------------------------------------------------------------------------------
def test_pix_library_exports_only_its_interface():
    assert os.path.exists(LIB), BUILD_IT
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[-1] for l in nm.splitlines() if l.strip())
    assert syms == sorted("asciichat_pix_" + n for n in PS.EXPORTS), syms
    needed = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libasciichat" not in needed  # it needs none of the other six libraries
    assert "libasciichat_pix.so" in open(os.path.join(PKG, "Makefile")).read()


def test_the_package_exports_the_binding():
    """Pix, PixSource, pix_convert, pix_downscale and pix_lib leave the package where yuv.py's names do"""
    text = open(os.path.join(PKG, "pix.py")).read()
    assert '__all__ = ["Pix", "PixSource", "pix_source", "pix_convert", "pix_downscale", "pix_lib"' in text
    assert "from .pix import *" in open(os.path.join(PKG, "__init__.py")).read()
    header = open(os.path.join(ROOT, "include", "asciichat_pix.h")).read()
    for name in PS.EXPORTS:
        assert "asciichat_pix_" + name + "(" in header, name
    assert "handlers.c:813" in header and "capture.c:299" in header  # the wire's own disagreement is stated, nothing about it claimed


# ---- the host code under the sanitizers, as a program of its own ------------------------------------------------------------------
def test_host_code_is_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pix_fuzz")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ascii-chat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fuzz", "pix_fuzz.c"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([exe, "10000"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "pix fuzz ok" in out.stdout, out.stderr[-3000:]
