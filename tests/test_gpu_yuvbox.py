"""YUV sources box-averaged straight from their planes, on the GPU: every shared case of yuvbox_support.py through
libasciichat_yuvbox.so into guard-filled buffers against the composition of the two restatements (tests/yuvbox_ref.py);
yuvbox_downscale per format; two ticks queued on one stream; the cross-library claim -- Yuv.run_whole followed by Box.run leaves
the images YuvBox.run leaves, and Plan.render over either's render_frames the same text --; the device's arithmetic over all 2^24
(Y, U, V) through identity-size runs; the refusals."""
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
import yuvbox_ref as BR  # noqa: E402
import yuvbox_support as BS  # noqa: E402

CASES = BS.cases()
FLIP_X = BS.FLIP_X


@pytest.fixture(scope="module")
def pkg():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from __graft_entry__ import load_package

    p = load_package()
    assert hasattr(p, "yuvbox_lib"), "the package has no yuvbox binding (ascii-chat_amd/yuvbox.py)"
    assert torch.cuda.is_available() and p.yuvbox_lib().asciichat_yuvbox_device_count() > 0  # (a missing library: build first)
    return p


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a, dtype=np.uint8, order="C")).cuda()  # (a copy: shared inputs stay read-only)
    assert t.data_ptr() % 16 == 0
    return t


def _sources(pkg, srcs, cls=None):
    """-> (device tensors to keep alive, [source structures])"""
    devs = [_dev(s.image) for s in srcs]
    return devs, [s.c_source(d.data_ptr(), cls or pkg.YuvSource) for s, d in zip(srcs, devs)]


def _images(case):
    """-> (guard-filled device tensor, start, pitch)"""
    import torch
    size = YS.image_buffer(case)[0].size
    images = torch.full((size,), BS.FILL, dtype=torch.uint8, device="cuda")
    _, start, pitch = YS.image_buffer(case, base=images.data_ptr())
    return images, start, pitch


def _run_case(pkg, name, case):
    import torch
    devs, sources = _sources(pkg, [i[0] for i in case.items])
    images, start, pitch = _images(case)
    b = pkg.YuvBox(case.max_frames)
    try:
        b.set(sources, case.frames(pkg.Frame), stream=_stream())
        assert b.pitch == (max(3 * i[1] * i[2] for i in case.items) + 127) // 128 * 128
        b.run(images.data_ptr() + start, pitch, stream=_stream())
        torch.cuda.synchronize()
    finally:
        b.close()
    BS.check_images(name, case, images.cpu().numpy(), start, pitch)


# ---- the case table (the mixed batch -- four formats, four sizes, every flip, 8 frames in a handle of 12, a padded pitch -- among
# them): exactly 3 * out_w * out_h bytes of every slot change ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_cases(pkg, name):
    _run_case(pkg, name, CASES[name])


@pytest.mark.parametrize("fmt", YS.FORMATS, ids=[YR.NAMES[f] for f in YS.FORMATS])
def test_downscale(pkg, fmt):
    """one source by value in the kernel arguments, to a destination at any alignment, with and without flips"""
    import torch
    src = YS.Src(fmt, 30, 17, 400 + fmt, strides=BS._padded(fmt, 30, 3), offs=(1, 2, 3), extremes=True)
    devs, (source,) = _sources(pkg, [src])
    for k, (ow, oh, fx, fy) in enumerate(((7, 4, False, False), (30, 17, True, False), (1, 1, False, True), (45, 20, True, True))):
        nb = 3 * ow * oh
        dst = torch.full((64 + nb + 64,), BS.FILL, dtype=torch.uint8, device="cuda")
        pkg.yuvbox_downscale(source, dst.data_ptr() + 64 + k, ow, oh, fx, fy, stream=_stream())
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert (got[:64 + k] == BS.FILL).all() and (got[64 + k + nb:] == BS.FILL).all(), (YR.NAMES[fmt], ow, oh)
        assert np.array_equal(got[64 + k:64 + k + nb].reshape(oh, ow, 3), BR.image(src.ref, ow, oh, fx, fy)), (YR.NAMES[fmt], ow, oh, fx, fy)


# ---- two ticks ---------------------------------------------------------------------------------------------------------------------
def test_two_ticks_queued_on_one_stream(pkg):
    """set and run of tick 2 queued behind tick 1 with no host wait in between: tick 2's images come from tick 2's sources"""
    import torch
    n, w, h, ow, oh = 24, 64, 36, 9, 5
    ticks = [BS.Case([(YS.Src(YS.FORMATS[i % 4], w, h, 800 + 100 * k + i), ow, oh, (i + k) % 4) for i in range(n)]) for k in range(2)]
    placed = [_sources(pkg, [i[0] for i in t.items]) for t in ticks]
    stream = _stream()
    b = pkg.YuvBox(n)
    try:
        outs = []
        for k, t in enumerate(ticks):
            images, start, pitch = _images(t)
            b.set(placed[k][1], t.frames(pkg.Frame), stream=stream)
            b.run(images.data_ptr() + start, pitch, stream=stream)
            outs.append((images, start, pitch))
        torch.cuda.synchronize()
        for k, (images, start, pitch) in enumerate(outs):
            BS.check_images(f"tick {k}", ticks[k], images.cpu().numpy(), start, pitch)
    finally:
        b.close()
    assert not np.array_equal(ticks[0].expected()[0], ticks[1].expected()[0])


# ---- the cross-library claim ------------------------------------------------------------------------------------------------------
def _two_routes(pkg, srcs, frames):
    """srcs through Yuv.run_whole + Box.run and through YuvBox.run under the same descriptors (their src set to the whole
    conversions for the first route) -> (images of the route, images of the pass, pitch, the two lists of render descriptors,
    what to keep alive)"""
    import torch
    n = len(srcs)
    devs, sources = _sources(pkg, srcs)
    stream = _stream()
    y = pkg.Yuv(n)
    y.set(sources, None, stream=stream)
    whole = torch.empty((n * y.whole_pitch,), dtype=torch.uint8, device="cuda")
    y.run_whole(whole.data_ptr(), stream=stream)
    for i, f in enumerate(frames):
        f.src, f.src_stride = whole.data_ptr() + i * y.whole_pitch, 0
    box = pkg.Box(frames)
    route = torch.full((n * box.pitch,), BS.FILL, dtype=torch.uint8, device="cuda")
    box.run(route.data_ptr(), stream=stream)
    route_frames = box.render_frames(route.data_ptr())
    b = pkg.YuvBox(n)
    for f in frames:  # set() reads neither
        f.src, f.src_stride = None, 12345
    b.set(sources, frames, stream=stream)
    assert b.pitch == box.pitch
    fused = torch.full((n * b.pitch,), BS.FILL, dtype=torch.uint8, device="cuda")
    b.run(fused.data_ptr(), stream=stream)
    fused_frames = b.render_frames(fused.data_ptr())
    torch.cuda.synchronize()
    pitch = b.pitch
    y.close(), box.close(), b.close()
    return route, fused, pitch, route_frames, fused_frames, (devs, whole)


@pytest.mark.parametrize("fmt", YS.FORMATS, ids=[YR.NAMES[f] for f in YS.FORMATS])
def test_the_pass_leaves_what_run_whole_and_box_run_leave(pkg, fmt):
    src = YS.Src(fmt, 64, 48, 500 + fmt, extremes=True)
    frames = [YS.frame(src, 7, 5, fl, cls=pkg.Frame) for fl in (FLIP_X, 0, 3)]
    route, fused, pitch, route_frames, fused_frames, keep = _two_routes(pkg, [src] * 3, frames)
    a, b = route.cpu().numpy(), fused.cpu().numpy()
    assert np.array_equal(a, b), YR.NAMES[fmt]  # images and untouched guard bytes alike
    for i, fl in enumerate((FLIP_X, 0, 3)):
        assert np.array_equal(b[i * pitch:i * pitch + 105].reshape(5, 7, 3), BR.image(src.ref, 7, 5, bool(fl & 1), bool(fl & 2))), (YR.NAMES[fmt], fl)
        assert (b[i * pitch + 105:(i + 1) * pitch] == BS.FILL).all()
    for r, f in zip(route_frames, fused_frames):  # the same descriptors but for the images' place and how "tight" is written
        assert r.src_stride in (0, 3 * r.out_w) and f.src_stride == 3 * f.out_w
        r.src, r.src_stride = f.src, f.src_stride
        assert bytes(r) == bytes(f)


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


@pytest.mark.parametrize("mode,rm", [(1, 0), (5, 2)], ids=["TRUE_FG", "HB_TRUE"])
def test_render_is_byte_identical_between_the_two_routes(pkg, mode, rm):
    """Plan.render over render_frames of either route's images: the same text, and the oracle's over the restatement's image"""
    srcs = [YS.Src(fmt, 64, 48, 520 + fmt) for fmt in YS.FORMATS]
    frames = [pkg.frame_setup(None, 64, 48, 20, 6, rm, False, False, False) for _ in srcs]
    assert all(f is not None and (f.out_w, f.out_h) == (20, 12 if rm == 2 else 6) for f in frames)
    frames[1].ops |= FLIP_X
    route, fused, pitch, route_frames, fused_frames, keep = _two_routes(pkg, srcs, frames)
    want, got = _render(pkg, mode, route_frames), _render(pkg, mode, fused_frames)
    for i, s in enumerate(srcs):
        img = BR.image(s.ref, frames[i].out_w, frames[i].out_h, i == 1, False)
        assert got[i] == want[i] and len(got[i]) > 120, (YR.NAMES[s.format], len(got[i]), len(want[i]))
        assert got[i] == orc.convert_with_caps(img, 20, 6, 3, rm, False, False, False), YR.NAMES[s.format]


# ---- the device's arithmetic ------------------------------------------------------------------------------------------------------
def test_device_arithmetic_over_all_2_24_inputs(pkg):
    """Four 2048 x 2048 I420 sources in one set, each averaged to its own size -- every box one pixel, the image the conversion.
    Chroma sample c (over the four sources, row-major in each 1024 x 1024 plane) holds pair c % 65536 = U << 8 | V, and the four
    pixels of its block hold Y = 4 * (c / 65536) + 2 * dy + dx: every (Y, U, V) once."""
    import torch
    side, half = 2048, 1024
    seen = np.zeros(1 << 24, dtype=bool)
    planes, sources, inputs = [], [], []
    for k in range(4):
        c = np.arange(k * half * half, (k + 1) * half * half, dtype=np.int64).reshape(half, half)
        U, V = ((c % 65536) >> 8).astype(np.uint8), (c % 256).astype(np.uint8)
        Y = np.empty((side, side), dtype=np.uint8)
        for dy in range(2):
            for dx in range(2):
                Y[dy::2, dx::2] = 4 * (c // 65536) + 2 * dy + dx
        up = lambda a: np.repeat(np.repeat(a, 2, 0), 2, 1)  # noqa: E731
        seen[(Y.astype(np.int64) << 16) | (up(U).astype(np.int64) << 8) | up(V)] = True
        planes.append([_dev(Y), _dev(U), _dev(V)])
        sources.append(pkg.yuv_source(pkg.YUV_I420, side, side, [p.data_ptr() for p in planes[-1]]))
        inputs.append((Y, U, V))
    assert seen.all()
    frames = []
    for _ in range(4):  # (written out: achip_frame_setup is for terminal sizes)
        f = pkg.Frame()
        f.src_w, f.src_h, f.out_w, f.out_h, f.x_ratio, f.y_ratio = side, side, side, side, 65537, 65537
        frames.append(f)
    b = pkg.YuvBox(4)
    try:
        b.set(sources, frames, stream=_stream())
        assert b.pitch == 3 * side * side
        rgb = torch.empty((4 * b.pitch,), dtype=torch.uint8, device="cuda")
        b.run(rgb.data_ptr(), stream=_stream())
        torch.cuda.synchronize()
    finally:
        b.close()
    got = rgb.cpu().numpy().reshape(4, side, side, 3)
    for k, (Y, U, V) in enumerate(inputs):
        for y0 in range(0, side, 512):  # (in bands: the restatement works in 32-bit integers)
            cu, cv = U[y0 // 2:y0 // 2 + 256], V[y0 // 2:y0 // 2 + 256]
            want = YR.rule(Y[y0:y0 + 512], np.repeat(np.repeat(cu, 2, 0), 2, 1), np.repeat(np.repeat(cv, 2, 0), 2, 1))
            assert np.array_equal(got[k, y0:y0 + 512], want), f"source {k} rows {y0}..{y0 + 511}"


# ---- the refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(pkg):
    """every refusal returns its code, launches nothing and leaves a working handle (yuvbox_support.check_refusals, through a
    binding of its own over the same library)"""
    import torch
    pkg.yuvbox_lib()
    L = BS.bind(C.CDLL(pkg.YUVBOX_LIB_PATH))
    kept = []

    def place(srcs):
        return _sources(pkg, srcs, BS.CSource)

    def new_images(case):
        images, start, pitch = _images(case)
        kept.append(images)
        return images.data_ptr() + start, pitch, lambda: (images.cpu().numpy(), start)

    BS.check_refusals(L, place, new_images, stream=_stream(), synchronize=torch.cuda.synchronize)
    with pytest.raises(RuntimeError, match=r"\(86\)"):
        pkg.YuvBox(0)
    b = pkg.YuvBox(1)
    try:
        with pytest.raises(RuntimeError, match=r"\(86\)"):
            b.run(kept[0].data_ptr(), 128, stream=_stream())
        with pytest.raises(ValueError):
            b.set([], None)
    finally:
        b.close()
