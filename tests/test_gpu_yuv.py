"""YUV sources on the GPU: every shared case of yuv_support.py through libasciichat_yuv.so into guard-filled buffers against the
NumPy restatement (tests/yuv_ref.py); Yuv.run + Plan.render of render_frames' descriptors against Plan.render over the uploaded
whole conversion with the original descriptors, and against the oracle; the device's arithmetic over all 2^24 (Y, U, V); two
ticks queued on one stream; the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orc  # noqa: E402
import yuv_ref as YR  # noqa: E402
import yuv_support as YS  # noqa: E402

SAMPLE = YS.sample_cases()
WHOLE = YS.whole_cases()
# mode -> the oracle's render_mode for frame_setup
RENDER_MODE = {1: 0, 5: 2, 9: 1}


@pytest.fixture(scope="module")
def pkg():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from __graft_entry__ import load_package

    p = load_package()
    assert torch.cuda.is_available() and p.yuv_lib().asciichat_yuv_device_count() > 0
    return p


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a, dtype=np.uint8, order="C")).cuda()  # (a copy: shared inputs stay read-only)
    assert t.data_ptr() % 16 == 0
    return t


def _sources(pkg, srcs):
    """-> (device tensors to keep alive, [YuvSource])"""
    devs = [_dev(s.image) for s in srcs]
    return devs, [s.c_source(d.data_ptr(), pkg.YuvSource) for s, d in zip(srcs, devs)]


# ---- the case table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SAMPLE))
def test_sampled_cases(pkg, name):
    import torch
    case = SAMPLE[name]
    devs, sources = _sources(pkg, [i[0] for i in case.items])
    size = YS.image_buffer(case)[0].size
    images = torch.full((size,), YS.FILL, dtype=torch.uint8, device="cuda")
    _, start, pitch = YS.image_buffer(case, base=images.data_ptr())
    y = pkg.Yuv(case.max_frames)
    try:
        y.set(sources, case.frames(pkg.Frame), stream=_stream())
        assert y.pitch == (max(3 * i[1] * i[2] for i in case.items) + 127) // 128 * 128
        y.run(images.data_ptr() + start, pitch, stream=_stream())
        torch.cuda.synchronize()
    finally:
        y.close()
    YS.check_images(name, case, images.cpu().numpy(), start, pitch)


@pytest.mark.parametrize("fmt", YS.FORMATS, ids=[YR.NAMES[f] for f in YS.FORMATS])
def test_convert_cases(pkg, fmt):
    import torch
    for name, case in WHOLE[fmt].items():
        devs, (source,) = _sources(pkg, [case.src])
        size = YS.whole_buffer(case)[0].size
        rgb = torch.full((size,), YS.FILL, dtype=torch.uint8, device="cuda")
        _, start, _ = YS.whole_buffer(case, base=rgb.data_ptr())
        pkg.yuv_convert(source, rgb.data_ptr() + start, case.rgb_stride, stream=_stream())
        torch.cuda.synchronize()
        YS.check_whole(f"{YR.NAMES[fmt]} {name}", case.src, rgb.cpu().numpy(), start, case.row_stride())


def test_run_whole_of_a_mixed_batch(pkg):
    import torch
    srcs = YS.whole_batch()
    devs, sources = _sources(pkg, srcs)
    n = len(srcs)
    y = pkg.Yuv(n + 2)
    try:
        y.set(sources, None, stream=_stream())
        largest = max(3 * s.width * s.height for s in srcs)
        assert y.whole_pitch == (largest + 127) // 128 * 128 and y.pitch == 0
        pitch, start = largest + 7, 3  # (any pitch at least the largest image, any alignment)
        rgb = torch.full((start + n * pitch + 128,), YS.FILL, dtype=torch.uint8, device="cuda")
        y.run_whole(rgb.data_ptr() + start, pitch, stream=_stream())
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="86"):  # a set without descriptors serves run_whole only
            y.run(rgb.data_ptr(), 128, stream=_stream())
        with pytest.raises(RuntimeError, match="86"):
            y.render_frames(rgb.data_ptr(), 128)
    finally:
        y.close()
    got = rgb.cpu().numpy()
    assert (got[:start] == YS.FILL).all() and (got[start + n * pitch:] == YS.FILL).all()
    for i, s in enumerate(srcs):
        nb = 3 * s.width * s.height
        slot = got[start + i * pitch:start + (i + 1) * pitch]
        assert np.array_equal(slot[:nb], s.whole().reshape(-1)), f"image {i} ({YR.NAMES[s.format]} {s.width}x{s.height})"
        assert (slot[nb:] == YS.FILL).all(), f"image {i}: a store beyond the image"


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _render(pkg, mode, frames):
    """-> the frames' bytes"""
    import torch
    plan = pkg.Plan(mode, orc.PALETTE_STANDARD, frames)
    n = len(frames)
    out = torch.zeros(n * plan.stride, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    plan.render(out.data_ptr(), plan.stride, ln.data_ptr(), _stream())
    torch.cuda.synchronize()
    host, lens = out.cpu().numpy(), ln.cpu().numpy()
    res = [bytes(host[i * plan.stride:i * plan.stride + (int(lens[i]) & 0xFFFFFFFF)]) for i in range(n)]
    plan.close()
    return res


_e2e = {}


def _e2e_source(fmt):
    if fmt not in _e2e:
        _e2e[fmt] = YS.Src(fmt, 320, 180, 700 + fmt, strides=(0, 0, 0) if fmt % 2 else (YR.row_bytes(fmt, 0, 320) + 8, 0, 0), extremes=True)
    return _e2e[fmt]


def _e2e_frames(pkg, src, rgb_ptr, mode):
    """three descriptors over one source as frame_setup makes them: plain, padded with the aspect kept, flipped and tinted"""
    rm = RENDER_MODE[mode]
    frames = [pkg.frame_setup(rgb_ptr, src.width, src.height, 60, 20, rm, False, False, False),
              pkg.frame_setup(rgb_ptr, src.width, src.height, 60, 20, rm, True, True, False),
              pkg.frame_setup(rgb_ptr, src.width, src.height, 41, 13, rm, False, False, False)]
    assert all(f is not None for f in frames) and (frames[1].pad_left > 0 or frames[1].pad_top > 0)
    assert pkg.lib().achip_frame_set_display_ops(C.byref(frames[2]), True, True, 0 if mode == 9 else 7) == 0
    return frames


@pytest.mark.parametrize("mode", list(RENDER_MODE), ids=["TRUE_FG", "HB_TRUE", "16_DITHER_BG"])
@pytest.mark.parametrize("fmt", YS.FORMATS, ids=[YR.NAMES[f] for f in YS.FORMATS])
def test_render_of_sampled_images_equals_render_of_the_whole_conversion(pkg, fmt, mode):
    import torch
    src = _e2e_source(fmt)
    rgb = _dev(src.whole())
    frames = _e2e_frames(pkg, src, rgb.data_ptr(), mode)
    want = _render(pkg, mode, frames)
    devs, sources = _sources(pkg, [src] * 3)
    for f in frames:  # set() reads neither
        f.src, f.src_stride = None, 12345
    y = pkg.Yuv(3)
    try:
        y.set(sources, frames, stream=_stream())
        images = torch.full((3 * y.pitch,), YS.FILL, dtype=torch.uint8, device="cuda")
        dense = y.render_frames(images.data_ptr())
        for d, f in zip(dense, frames):
            assert (d.src_w, d.src_h, d.x_ratio, d.y_ratio, d.src_stride, d.comp) == (f.out_w, f.out_h, 65537, 65537, 3 * f.out_w, None)
            assert (d.out_w, d.out_h, d.pad_left, d.pad_top, d.ops) == (f.out_w, f.out_h, f.pad_left, f.pad_top, f.ops & ~3)
        assert dense[2].ops != frames[2].ops and [d.src for d in dense] == [images.data_ptr() + i * y.pitch for i in range(3)]
        y.run(images.data_ptr(), stream=_stream())
        got = _render(pkg, mode, dense)
    finally:
        y.close()
    for i in range(3):
        assert got[i] == want[i] and len(got[i]) > 60, f"{YR.NAMES[fmt]} mode {mode} frame {i}: {len(got[i])} vs {len(want[i])} bytes"


@pytest.mark.parametrize("fmt", YS.FORMATS, ids=[YR.NAMES[f] for f in YS.FORMATS])
def test_true_fg_against_the_oracle(pkg, fmt):
    import torch
    src = _e2e_source(fmt)
    frames = [pkg.frame_setup(None, src.width, src.height, 60, 20, 0, pad, pad, False) for pad in (False, True)]
    devs, sources = _sources(pkg, [src] * 2)
    y = pkg.Yuv(2)
    try:
        y.set(sources, frames, stream=_stream())
        images = torch.full((2 * y.pitch,), YS.FILL, dtype=torch.uint8, device="cuda")
        dense = y.render_frames(images.data_ptr())
        y.run(images.data_ptr(), stream=_stream())
        got = _render(pkg, 1, dense)
    finally:
        y.close()
    for i, pad in enumerate((False, True)):
        assert got[i] == orc.convert_with_caps(src.whole(), 60, 20, 3, 0, pad, pad, False), f"{YR.NAMES[fmt]} padded={pad}"


def test_two_ticks_queued_on_one_stream(pkg):
    """set, run and render of tick 2 queued behind tick 1 with no host wait in between: tick 2's text comes from tick 2's sources"""
    import torch
    n, w, h, ow, oh = 24, 64, 36, 20, 6
    ticks = [[YS.Src(YS.FORMATS[i % 4], w, h, 800 + 100 * k + i) for i in range(n)] for k in range(2)]
    placed = [_sources(pkg, t) for t in ticks]
    frames = [pkg.frame_setup(None, w, h, ow, oh, 0, False, False, False) for _ in range(n)]
    stream = _stream()
    y = pkg.Yuv(n)
    try:
        y.set(placed[0][1], frames, stream=stream)
        images = torch.full((n * y.pitch,), YS.FILL, dtype=torch.uint8, device="cuda")
        plan = pkg.Plan(1, orc.PALETTE_STANDARD, y.render_frames(images.data_ptr()))
        outs = [torch.zeros(n * plan.stride, dtype=torch.uint8, device="cuda") for _ in range(2)]
        lens = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
        for k in range(2):
            if k:
                y.set(placed[k][1], frames, stream=stream)
            y.run(images.data_ptr(), stream=stream)
            plan.render(outs[k].data_ptr(), plan.stride, lens[k].data_ptr(), stream)
        torch.cuda.synchronize()
        for k in range(2):
            host, ln = outs[k].cpu().numpy(), lens[k].cpu().numpy()
            for i in range(n):
                got = bytes(host[i * plan.stride:i * plan.stride + (int(ln[i]) & 0xFFFFFFFF)])
                assert got == orc.convert_with_caps(ticks[k][i].whole(), ow, oh, 3, 0), f"tick {k} frame {i}"
        plan.close()
    finally:
        y.close()


# ---- the device's arithmetic ------------------------------------------------------------------------------------------------------
def test_device_arithmetic_over_all_2_24_inputs(pkg):
    """One 4096 x 4096 I420 image: chroma sample c (row-major in the 2048 x 2048 planes) holds pair c % 65536 = U << 8 | V, and the
    four pixels of its block hold Y = 4 * (c / 65536) + 2 * dy + dx -- every (Y, U, V) once."""
    import torch
    c = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    U, V = ((c % 65536) >> 8).astype(np.uint8), (c % 256).astype(np.uint8)
    Y = np.empty((4096, 4096), dtype=np.uint8)
    for dy in range(2):
        for dx in range(2):
            Y[dy::2, dx::2] = 4 * (c // 65536) + 2 * dy + dx
    seen = np.zeros(1 << 24, dtype=bool)
    seen[(Y.astype(np.int64) << 16) | (np.repeat(np.repeat(U, 2, 0), 2, 1).astype(np.int64) << 8) | np.repeat(np.repeat(V, 2, 0), 2, 1)] = True
    assert seen.all()
    planes = [_dev(Y), _dev(U), _dev(V)]
    source = pkg.yuv_source(pkg.YUV_I420, 4096, 4096, [p.data_ptr() for p in planes])
    rgb = torch.empty((4096 * 4096 * 3,), dtype=torch.uint8, device="cuda")
    pkg.yuv_convert(source, rgb.data_ptr(), 0, stream=_stream())
    torch.cuda.synchronize()
    got = rgb.cpu().numpy().reshape(4096, 4096, 3)
    for y0 in range(0, 4096, 512):  # (in bands: the restatement works in 32-bit integers)
        want = YR.rule(Y[y0:y0 + 512], np.repeat(np.repeat(U[y0 // 2:y0 // 2 + 256], 2, 0), 2, 1), np.repeat(np.repeat(V[y0 // 2:y0 // 2 + 256], 2, 0), 2, 1))
        assert np.array_equal(got[y0:y0 + 512], want), f"rows {y0}..{y0 + 511}"


# ---- the refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(pkg):
    import torch
    case = SAMPLE["I420 16x8 -> 5x3: a tail of bytes"]
    src = case.items[0][0]
    devs, (good,) = _sources(pkg, [src])
    frame = case.frames(pkg.Frame)[0]
    images = torch.full((1024,), YS.FILL, dtype=torch.uint8, device="cuda")

    def refused(code, fn, *args, **kw):
        with pytest.raises(RuntimeError, match=rf"\({code}\)"):
            fn(*args, **kw)

    def changed(obj, **kw):
        c = type(obj).from_buffer_copy(bytes(obj))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    with pytest.raises(RuntimeError, match="86"):
        pkg.Yuv(0)
    y = pkg.Yuv(2)
    try:
        # before any set
        refused(86, y.run, images.data_ptr(), 128, stream=_stream())
        refused(86, y.run_whole, images.data_ptr(), 1024, stream=_stream())
        refused(86, y.render_frames, images.data_ptr(), 128)
        assert y.pitch == 0 and y.whole_pitch == 0
        # the set itself
        refused(86, y.set, [], [], stream=_stream())
        refused(86, y.set, [good] * 3, [frame] * 3, stream=_stream())
        refused(86, y.set, [changed(good, format=4)], [frame], stream=_stream())
        refused(86, y.set, [changed(good, width=8193)], [frame], stream=_stream())
        refused(86, y.set, [changed(good, format=pkg.YUV_NV12)], [frame], stream=_stream())  # a third plane on NV12
        refused(86, y.set, [good, changed(good, format=pkg.YUV_UYVY, width=15)], [frame] * 2, stream=_stream())
        refused(86, y.set, [good], [changed(frame, src_w=15)], stream=_stream())
        refused(86, y.set, [good], [changed(frame, x_ratio=(1 << 32) - 1)], stream=_stream())
        refused(30, y.set, [good], [changed(frame, comp=1)], stream=_stream())
        refused(86, y.run, images.data_ptr(), 128, stream=_stream())  # still nothing set
        y.set([good], [frame], stream=_stream())
        refused(30, y.set, [good, good], [frame, changed(frame, comp=1)], stream=_stream())  # the earlier set stays: one frame
        assert y.pitch == 128 and y.whole_pitch == 384
        # the runs
        refused(86, y.run, 0, 128, stream=_stream())
        refused(86, y.run, images.data_ptr() + 8, 128, stream=_stream())
        refused(86, y.run, images.data_ptr(), 120, stream=_stream())
        refused(86, y.run, images.data_ptr(), 32, stream=_stream())  # below the image's 45 bytes
        refused(86, y.render_frames, images.data_ptr(), 32)
        refused(86, y.run_whole, 0, 384, stream=_stream())
        refused(86, y.run_whole, images.data_ptr(), 383, stream=_stream())
        refused(86, pkg.yuv_convert, good, 0, 0, stream=_stream())
        refused(86, pkg.yuv_convert, good, images.data_ptr(), 47, stream=_stream())
        refused(86, pkg.yuv_convert, changed(good, height=0), images.data_ptr(), 0, stream=_stream())
        torch.cuda.synchronize()
        assert (images.cpu().numpy() == YS.FILL).all()  # nothing was launched
        # and the handle still works, with the set it was left with
        y.run(images.data_ptr(), 48, stream=_stream())
        torch.cuda.synchronize()
        got = images.cpu().numpy()
        assert np.array_equal(got[:45], case.expected()[0].reshape(-1)) and (got[45:] == YS.FILL).all()
    finally:
        y.close()
