"""YUV sources without a GPU: the kernels of libasciichat_yuv.so under the CPU emulator against the NumPy restatement
(tests/yuv_ref.py) over the shared case table -- bytes equal, nothing stored outside an image --, the arithmetic of yuv_math.h
over all 2^24 (Y, U, V), the hand known answers, every refusal of the pure-C checks at its limit, the claim that conversion
commutes with the renderers' sampling (the oracle's text, every mode), what the library exports, and the host code under the
sanitizers as a program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orc
import yuv_ref as YR
import yuv_support as YS
from achip_ctypes import ALL_MODES, MODE_CAPS, MODE_NAMES, MODE_TRUE_BG, Frame

SAMPLE = YS.sample_cases()
WHOLE = YS.whole_cases()
ROOT = YS.emubuild.ROOT
YUV_LIB = os.path.join(ROOT, "ascii-chat_amd", "libasciichat_yuv.so")


# ---- the restatement itself, by hand ------------------------------------------------------------------------------------------
def test_hand_known_answers():
    L = YS.emulator()
    for (y, u, v), rgb in YR.KNOWN.items():
        assert tuple(YR.rule(y, u, v)) == rgb, (y, u, v)
        p = L.emu_yuv_rgb(y, u, v)
        assert (p & 0xFF, (p >> 8) & 0xFF, (p >> 16) & 0xFF) == rgb and p >> 24 == 0, (y, u, v)


def test_layouts_by_hand():
    """one 4x2 image per format written out byte by byte: the table of asciichat_yuv.h"""
    Y = np.array([[10, 11, 12, 13], [20, 21, 22, 23]], dtype=np.uint8)

    def yuv_at(src):
        sy, sx = np.mgrid[0:2, 0:4]
        return [a.tolist() for a in YR.samples(src, sx, sy)]

    i420 = YR.Source(YR.I420, 4, 2, [Y.reshape(-1), np.array([100, 101], np.uint8), np.array([200, 201], np.uint8)], [4, 2, 2])
    nv12 = YR.Source(YR.NV12, 4, 2, [Y.reshape(-1), np.array([100, 200, 101, 201], np.uint8)], [4, 4])
    want = [Y.tolist(), [[100, 100, 101, 101]] * 2, [[200, 200, 201, 201]] * 2]
    assert yuv_at(i420) == want and yuv_at(nv12) == want
    uyvy = YR.Source(YR.UYVY, 4, 2, [np.array([100, 10, 200, 11, 101, 12, 201, 13, 102, 20, 202, 21, 103, 22, 203, 23], np.uint8)], [8])
    yuyv = YR.Source(YR.YUYV, 4, 2, [np.array([10, 100, 11, 200, 12, 101, 13, 201, 20, 102, 21, 202, 22, 103, 23, 203], np.uint8)], [8])
    want = [Y.tolist(), [[100, 100, 101, 101], [102, 102, 103, 103]], [[200, 200, 201, 201], [202, 202, 203, 203]]]
    assert yuv_at(uyvy) == want and yuv_at(yuyv) == want
    # pack() writes those very bytes
    for src, fmt in ((uyvy, YR.UYVY), (yuyv, YR.YUYV)):
        planes, strides = YR.pack(fmt, Y, np.array(want[1], np.uint8)[:, ::2], np.array(want[2], np.uint8)[:, ::2])
        assert strides == [8] and np.array_equal(planes[0], src.planes[0])
    planes, strides = YR.pack(YR.NV12, Y, np.array([[100, 101]], np.uint8), np.array([[200, 201]], np.uint8))
    assert strides == [4, 4] and np.array_equal(planes[1], nv12.planes[1])


# ---- the arithmetic over every input -------------------------------------------------------------------------------------------
def test_arithmetic_over_all_2_24_inputs():
    got = np.empty(3 << 24, dtype=np.uint8)
    YS.emulator().emu_yuv_rgb_all(got.ctypes.data)
    got = got.reshape(256, 256, 256, 3)
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for y in range(256):
        want = YR.rule(y, u, v)
        assert np.array_equal(got[y], want), f"Y {y}: first difference at (U, V) {np.argwhere((got[y] != want).any(axis=-1))[0]}"


# ---- the kernels under the emulator ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SAMPLE))
def test_sampled_pass_matches_the_restatement(name):
    case = SAMPLE[name]
    buf, start, pitch = YS.emu_run(case)
    YS.check_images(name, case, buf, start, pitch)


@pytest.mark.parametrize("fmt", YS.FORMATS, ids=[YR.NAMES[f] for f in YS.FORMATS])
def test_whole_conversion_matches_the_restatement(fmt):
    for name, case in WHOLE[fmt].items():
        buf, start = YS.emu_convert(case)
        YS.check_whole(f"{YR.NAMES[fmt]} {name}", case.src, buf, start, case.row_stride())


def test_run_whole_of_a_mixed_batch():
    srcs = YS.whole_batch()
    keep = [YS.host_copy(s) for s in srcs]
    n = len(srcs)
    arr = (YS.CSource * n)(*[s.c_source(k[1]) for s, k in zip(srcs, keep)])
    pitch = max(3 * s.width * s.height for s in srcs) + 7  # (any pitch at least the largest image, any alignment)
    buf = np.full(64 + 3 + n * pitch + 128, YS.FILL, dtype=np.uint8)
    start = 64 + (-(buf.ctypes.data + 64)) % 16 + 3
    assert YS.emulator().emu_yuv_run_whole(C.cast(arr, C.c_void_p), n, n + 2, buf.ctypes.data + start, pitch) == 0
    assert (buf[:start] == YS.FILL).all() and (buf[start + n * pitch:] == YS.FILL).all()
    for i, s in enumerate(srcs):
        nb = 3 * s.width * s.height
        slot = buf[start + i * pitch:start + (i + 1) * pitch]
        assert np.array_equal(slot[:nb], s.whole().reshape(-1)), f"image {i} ({YR.NAMES[s.format]} {s.width}x{s.height})"
        assert (slot[nb:] == YS.FILL).all(), f"image {i}: a store beyond the image"


def test_cases_cover_what_they_claim():
    f = SAMPLE["I420 4x2 -> 9x5 into the clamp"].frames()[0]
    assert (8 * f.x_ratio) >> 16 > 3 and (4 * f.y_ratio) >> 16 > 1 and 8 * f.x_ratio < 1 << 32  # past the source: clamped, not wrapped
    case = SAMPLE["NV12 64x48 -> 37x29: two workgroups, one pixel in the last lane"]
    assert 37 * 29 > 4 * 256 and 37 * 29 % 4 == 1
    assert 299 % 4 and (3 * 5 * 3) % 4  # rows straddled by a lane, a tail of bytes
    mixed = SAMPLE["batch of 40 in a handle of 64"]
    assert {i[0].format for i in mixed.items} == set(YS.FORMATS) and len({(i[0].width, i[0].height) for i in mixed.items}) > 4
    assert len(SAMPLE["33 of 40 frames set"].items) == 33 and SAMPLE["33 of 40 frames set"].max_frames == 40
    s = SAMPLE["I420 strides 24 / 13 / 11"].items[0][0]
    assert s.ref.strides == [24, 13, 11] and [a % 16 for a in s.at] == [1, 3, 2]
    for fmt in YS.FORMATS:
        offs = {(c.dst_off, bool(c.rgb_stride)) for c in WHOLE[fmt].values()}
        assert offs == {(o, p) for o in range(4) for p in (False, True)}
        widths = {c.src.width for c in WHOLE[fmt].values()}
        assert widths >= ({2, 6, 14, 15, 16, 18} if fmt in YS.PLANAR else {2, 6, 14, 16, 18})
        assert any(a % 4 for c in WHOLE[fmt].values() for a in c.src.at) and any(s % 4 for c in WHOLE[fmt].values() for s in c.src.ref.strides)


def test_host_addressing_equals_the_restatement():
    """yuv_math.h's yuv_pixel (what the edge paths of the kernels and the fuzz program walk) over every pixel of padded sources"""
    L = YS.emulator()
    for fmt in YS.FORMATS:
        src = YS.Src(fmt, 6, 5, 500 + fmt, strides=(17, 9 if fmt == YR.I420 else 11 if fmt == YR.NV12 else 0, 7 if fmt == YR.I420 else 0),
                     offs=(1, 2, 3))
        keep, addr = YS.host_copy(src)
        s = src.c_source(addr)
        want = src.whole()
        for y in range(5):
            for x in range(6):
                p = L.emu_yuv_host_pixel(C.byref(s), x, y)
                assert [p & 0xFF, (p >> 8) & 0xFF, (p >> 16) & 0xFF] == want[y, x].tolist(), (YR.NAMES[fmt], x, y)


# ---- every refusal at its limit ---------------------------------------------------------------------------------------------------
_BUF = np.zeros(64, dtype=np.uint8)


def _src(fmt=YR.I420, w=16, h=8, planes=None, strides=(0, 0, 0)):
    s = YS.CSource()
    s.format, s.width, s.height = fmt, w, h
    if planes is None:
        planes = [1] * YR.planes_of(fmt) if 0 <= fmt <= 3 else [1]
    for k in range(3):
        s.plane[k] = _BUF.ctypes.data if k < len(planes) and planes[k] else None  # (never read: the checks look at NULL or not)
        s.stride[k] = strides[k]
    return s


def _source_ok(s):
    why = C.c_char_p()
    rc = YS.emulator().emu_yuv_source_check(C.byref(s), C.byref(why))
    assert (rc == 0) == (why.value is None)
    return rc == 0


def test_source_refusals_at_their_limits():
    assert not YS.emulator().emu_yuv_source_check(None, None) == 0
    assert [_source_ok(_src(f)) for f in (-1, 0, 1, 2, 3, 4)] == [False, True, True, True, True, False]
    for fmt in YS.FORMATS:
        n = YR.planes_of(fmt)
        for k in range(n):  # a NULL plane
            assert not _source_ok(_src(fmt, planes=[j != k for j in range(n)])), (fmt, k)
        for k in range(n, 3):  # a plane the format does not use: the third plane on NV12, the second and third on the packed ones
            assert not _source_ok(_src(fmt, planes=[1] * n + [j == k for j in range(n, 3)])), (fmt, k)
        for side in ("w", "h"):  # size 0 and 8193 (8192 for a width: even)
            assert [_source_ok(_src(fmt, **{side: v})) for v in (0, 2, 8192, 8193, 8194)] == [False, True, True, False, False], (fmt, side)
        assert _source_ok(_src(fmt, h=1)) and _source_ok(_src(fmt, h=7))
        assert _source_ok(_src(fmt, w=15)) == (fmt in YS.PLANAR) and _source_ok(_src(fmt, w=1)) == (fmt in YS.PLANAR)  # an odd packed width
        for w in (16, 15) if fmt in YS.PLANAR else (16,):
            for k in range(n):  # each stride one short, exact, 0, at 2^24 - 1, at 2^24, negative
                need = YR.row_bytes(fmt, k, w)

                def with_stride(v):
                    st = [0, 0, 0]
                    st[k] = v
                    return _source_ok(_src(fmt, w=w, strides=st))

                assert [with_stride(v) for v in (need - 1, need, 0, (1 << 24) - 1, 1 << 24, -1)] == [False, True, True, True, False, False], (fmt, k, w)
    assert YR.row_bytes(YR.NV12, 1, 15) == 16 and YR.row_bytes(YR.I420, 2, 15) == 8


def _frames_check(sources, frames, n=None, max_frames=4):
    sa = (YS.CSource * max(1, len(sources)))(*sources)
    fa = (Frame * max(1, len(frames)))(*frames) if frames is not None else None
    bad, unsupported, why = C.c_int(-5), C.c_int(-5), C.c_char_p()
    rc = YS.emulator().emu_yuv_frames_check(C.cast(sa, C.c_void_p) if sources else None, C.cast(fa, C.c_void_p) if fa is not None else None,
                                            len(sources) if n is None else n, max_frames, C.byref(bad), C.byref(unsupported), C.byref(why))
    assert (rc == 0) == (why.value is None) and (rc != 0 or (bad.value, unsupported.value) == (-1, 0))
    return rc == 0, bad.value, unsupported.value


def _desc(w=16, h=8, ow=5, oh=3, **kw):
    f = Frame()
    f.src_w, f.src_h, f.out_w, f.out_h = w, h, ow, oh
    f.x_ratio, f.y_ratio = (w << 16) // ow + 1, (h << 16) // oh + 1
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def test_set_refusals_at_their_limits():
    ok = lambda *a, **kw: _frames_check(*a, **kw)[0]  # noqa: E731
    assert ok([_src()], [_desc()]) and ok([_src()], None)
    # the number of sources
    four = [_src() for _ in range(4)]
    assert ok(four, [_desc()] * 4) and not ok(four + [_src()], [_desc()] * 5) and ok(four, None, n=1, max_frames=1)
    assert not ok(four, None, n=0) and not ok([], None, n=1)
    # a bad source is named
    assert _frames_check([_src(), _src(w=8193)], None)[:2] == (False, 1)
    # the size of the descriptor is the source's
    for kw in (dict(src_w=15), dict(src_w=17), dict(src_h=7), dict(src_h=9)):
        assert _frames_check([_src(), _src()], [_desc(), _desc(**kw)])[:2] == (False, 1), kw
    # comp: refused as unsupported, nothing else is
    assert _frames_check([_src()], [_desc(comp=1)]) == (False, 0, 1)
    assert _frames_check([_src()], [_desc(out_w=0)]) == (False, 0, 0)
    # src and src_stride are not read; paddings, tints, the override and dither bits pass through
    assert ok([_src()], [_desc(src=None, src_stride=-7, pad_left=3, pad_top=2, ops=3 | 4 | 0x112233 << 8)]) and ok([_src()], [_desc(ops=64 | 16)])
    # an image size below 1
    for field in ("out_w", "out_h"):
        assert ok([_src()], [_desc(**{field: 1})]) and not ok([_src()], [_desc(**{field: 0})]) and not ok([_src()], [_desc(**{field: -1})])
    # a wrapping ratio: (out - 1) * ratio below 2^32
    top = (1 << 32) - 1
    assert ok([_src()], [_desc(ow=16, x_ratio=top // 15)]) and not ok([_src()], [_desc(ow=16, x_ratio=top // 15 + 1)])
    assert ok([_src()], [_desc(oh=4, y_ratio=top // 3)]) and not ok([_src()], [_desc(oh=4, y_ratio=top // 3 + 1)])


# ---- conversion commutes with the renderers' sampling ---------------------------------------------------------------------------
def _oracle_text(img, mode, W, H, palette):
    if mode == MODE_TRUE_BG:
        return orc.print_truecolor_bg(orc.resize_nn(img, W, H), palette)
    cl, rm = MODE_CAPS[mode]
    return orc.convert_with_caps(img, W, H, cl, rm, False, False, False, palette)


@pytest.mark.parametrize("mode", ALL_MODES, ids=MODE_NAMES)
def test_conversion_commutes_with_sampling(mode):
    """the oracle's text over the sampled image under the rewritten (identity) descriptor equals its text over the wholly
    converted frame under the original one"""
    W, H = 20, 6
    half_block = MODE_CAPS.get(mode, (3, 0))[1] == 2
    out_h = 2 * H if half_block else H
    for fmt in YS.FORMATS:
        src = YS.Src(fmt, 64, 36, 600 + fmt)
        sampled = YR.sample(src.ref, YS.frame(src, W, out_h))
        assert sampled.shape == (out_h, W, 3)
        whole_text = _oracle_text(src.whole(), mode, W, H, orc.PALETTE_STANDARD)
        assert _oracle_text(sampled, mode, W, H, orc.PALETTE_STANDARD) == whole_text, (MODE_NAMES[mode], YR.NAMES[fmt])
        assert len(whole_text) > W * H


# ---- what the library exports -----------------------------------------------------------------------------------------------------
def test_yuv_library_exports_only_its_interface():
    assert os.path.exists(YUV_LIB), "libasciichat_yuv.so has not been built (make -C ascii-chat_amd)"
    nm = subprocess.run(["nm", "-D", "--defined-only", YUV_LIB], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[-1] for l in nm.splitlines() if l.strip())
    names = ("device_count", "last_error", "convert", "create", "set", "image_pitch", "run", "render_frames", "whole_pitch", "run_whole", "destroy")
    assert syms == sorted("asciichat_yuv_" + n for n in names), syms
    needed = subprocess.run(["readelf", "-d", YUV_LIB], capture_output=True, text=True, check=True).stdout
    assert "libasciichat_hip" not in needed and "libasciichat_raster" not in needed  # it needs neither other library


# ---- the host code under the sanitizers, as a program of its own ----------------------------------------------------------------
def test_host_code_is_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "yuv_fuzz")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ascii-chat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fuzz", "yuv_fuzz.c"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([exe, "20000"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "yuv fuzz ok" in out.stdout, out.stderr[-3000:]
