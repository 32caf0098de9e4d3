"""Cells straight from frame descriptors on the GPU: every shared case of raster_images_support.py through Raster.run_images
into a guard-filled buffer, against the existing chain on the CPU (the oracle's text, parsed and painted by the restatement) and
against the device's own chain -- Plan.render of the same descriptors into a slab, then Raster.run --, pixels and status equal;
the YUV entries against run_yuv420 over Plan.render's frames; the stage alone; two sets on one handle; the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orc  # noqa: E402
import raster_images_support as RI  # noqa: E402
import raster_support as RS  # noqa: E402

CASES = RI.cases()
YUV_CASES = ["true_fg pad_left 8", "256_fg 48x16 -> 16x4", "true_bg 48x16 -> 16x4", "hb_256 16x4 frame into 8x2", "hb_mono 48x16 -> 16x4",
             "mono 48x16 -> 16x4"]


@pytest.fixture(scope="module")
def pkg():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from __graft_entry__ import load_package

    p = load_package()
    assert torch.cuda.is_available() and p.raster_lib().asciichat_raster_device_count() > 0
    return p


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _font(pkg, font):
    return RS.c_font(font, pkg.RasterFont, pkg.RasterGlyph)


def _expected(pkg, name):
    return RI.expected(name, CASES[name], pkg.lib(), pkg.Frame)


def _on_device(pkg, case):
    """-> (the sources' device copies, the descriptors over them)"""
    import torch
    bufs = [torch.from_numpy(s.buf).cuda() for s in case.frames]
    return bufs, RI.descriptors(pkg.lib(), pkg.Frame, case, [b.data_ptr() for b in bufs])


def _text_path(pkg, case, frames, r, pixels_ptr, pitch, status_ptr):
    """the device's own chain for the frames the case runs: Plan.render into a slab, then Raster.run"""
    import torch
    n = case.n
    plan = pkg.Plan(case.mode, case.palette, frames[:n])
    slab = torch.zeros(n * plan.stride, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(n, dtype=torch.int32, device="cuda")
    plan.render(slab.data_ptr(), plan.stride, lens.data_ptr(), _stream())
    r.run(slab.data_ptr(), plan.stride, lens.data_ptr(), n, pixels_ptr, status_ptr, image_pitch=pitch, stream=_stream())
    torch.cuda.synchronize()
    plan.close()
    return slab, lens


@pytest.mark.parametrize("name", list(CASES))
def test_shared_cases(pkg, name):
    import torch
    case = CASES[name]
    bufs, frames = _on_device(pkg, case)
    size = RI.pixel_buffer(case)[0].size
    pixels = [torch.full((size,), RI.FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    assert pixels[0].data_ptr() % 16 == pixels[1].data_ptr() % 16
    _, start, pitch = RI.pixel_buffer(case, base=pixels[0].data_ptr())
    status = [torch.full((len(case.frames),), 0xABABABAB - (1 << 32), dtype=torch.int32, device="cuda") for _ in range(2)]
    r = pkg.Raster(_font(pkg, case.font), case.cols, case.rows, case.max_frames)
    try:
        r.set_images(case.mode, case.palette, frames, stream=_stream())
        r.run_images(case.n, pixels[0].data_ptr() + start, status[0].data_ptr(), image_pitch=pitch, stream=_stream())
        torch.cuda.synchronize()
        _text_path(pkg, case, frames, r, pixels[1].data_ptr() + start, pitch, status[1].data_ptr())
    finally:
        r.close()
    got, st = pixels[0].cpu().numpy(), status[0].cpu().numpy().view(np.uint32)
    RI.check(name, case, _expected(pkg, name), got, start, pitch, st)
    assert np.array_equal(got, pixels[1].cpu().numpy()), f"{name}: run_images and Plan.render -> run differ"
    assert np.array_equal(st, status[1].cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("layout", ["I420", "NV12"])
@pytest.mark.parametrize("name", YUV_CASES)
def test_yuv_planes_equal_the_text_paths(pkg, name, layout):
    import torch
    case = CASES[name]
    n, lay = case.n, getattr(pkg, "RASTER_YUV_" + layout)
    bufs, frames = _on_device(pkg, case)
    r = pkg.Raster(_font(pkg, case.font), case.cols, case.rows, case.max_frames)
    try:
        pitch = (r.yuv_pitch + 3) // 4 * 4 + 8
        planes = [torch.full((n * pitch + 64,), RI.FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
        status = [torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
        r.set_images(case.mode, case.palette, frames, stream=_stream())
        r.run_images_yuv420(n, planes[0].data_ptr(), status[0].data_ptr(), lay, image_pitch=pitch, stream=_stream())
        plan = pkg.Plan(case.mode, case.palette, frames[:n])
        slab = torch.zeros(n * plan.stride, dtype=torch.uint8, device="cuda")
        lens = torch.zeros(n, dtype=torch.int32, device="cuda")
        plan.render(slab.data_ptr(), plan.stride, lens.data_ptr(), _stream())
        r.run_yuv420(slab.data_ptr(), plan.stride, lens.data_ptr(), n, planes[1].data_ptr(), status[1].data_ptr(), lay, image_pitch=pitch,
                     stream=_stream())
        torch.cuda.synchronize()
        plan.close()
        got = planes[0].cpu().numpy()
        assert np.array_equal(got, planes[1].cpu().numpy()) and np.array_equal(status[0].cpu().numpy(), status[1].cpu().numpy())
        used = got[:n * pitch].reshape(n, pitch)
        assert (used[:, r.yuv_pitch:] == RI.FILL).all() and (got[n * pitch:] == RI.FILL).all() and (used[:, :r.yuv_pitch] != RI.FILL).any()
        assert [int(s) for s in status[0].cpu().numpy().view(np.uint32)] == [e[1] for e in _expected(pkg, name)]
    finally:
        r.close()


def test_the_stage_alone_then_draw_equals_run_images(pkg):
    import torch
    name = "batch of 40 in a handle of 64"
    case = CASES[name]
    bufs, frames = _on_device(pkg, case)
    r = pkg.Raster(_font(pkg, case.font), case.cols, case.rows, case.max_frames)
    n = case.n
    pixels = [torch.full((n * r.pitch,), RI.FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    status = [torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    try:
        r.set_images(case.mode, case.palette, frames, stream=_stream())
        r.run_images(n, pixels[0].data_ptr(), status[0].data_ptr(), stream=_stream())
        r.cells_from_images(n, status[1].data_ptr(), stream=_stream())
        r.draw(n, pixels[1].data_ptr(), stream=_stream())
        torch.cuda.synchronize()
    finally:
        r.close()
    assert np.array_equal(pixels[0].cpu().numpy(), pixels[1].cpu().numpy()) and np.array_equal(status[0].cpu().numpy(), status[1].cpu().numpy())
    RI.check(name, case, _expected(pkg, name), pixels[0].cpu().numpy(), 0, r.pitch, status[0].cpu().numpy().view(np.uint32))


def test_a_second_set_leaves_nothing_of_the_first(pkg):
    """set -> run -> set with other frames, another mode and another palette -> run, with no host wait in between; then parse()'s
    text path on the same handle"""
    import torch
    first, second = "true_fg pad_left 8", "hb_256 pad_top"
    a, b = CASES[first], CASES[second]
    assert (a.cols, a.rows, a.atlas) == (b.cols, b.rows, b.atlas)
    bufs_a, frames_a = _on_device(pkg, a)
    bufs_b, frames_b = _on_device(pkg, b)
    r = pkg.Raster(_font(pkg, a.font), a.cols, a.rows, 2)
    pixels = [torch.full((r.pitch + 64,), RI.FILL, dtype=torch.uint8, device="cuda") for _ in range(3)]
    status = [torch.full((1,), 0xABABABAB - (1 << 32), dtype=torch.int32, device="cuda") for _ in range(3)]
    try:
        r.set_images(a.mode, a.palette, frames_a, stream=_stream())
        r.run_images(1, pixels[0].data_ptr(), status[0].data_ptr(), stream=_stream())
        r.set_images(b.mode, b.palette, frames_b, stream=_stream())
        r.run_images(1, pixels[1].data_ptr(), status[1].data_ptr(), stream=_stream())
        torch.cuda.synchronize()
        _text_path(pkg, a, frames_a, r, pixels[2].data_ptr(), r.pitch, status[2].data_ptr())
    finally:
        r.close()
    for name, case, k in ((first, a, 0), (second, b, 1), (first, a, 2)):
        RI.check(name, case, _expected(pkg, name), pixels[k].cpu().numpy(), 0, r.pitch + 64, status[k].cpu().numpy().view(np.uint32))


def test_refusals_on_the_device(pkg):
    import torch
    case = CASES["true_fg 48x16 -> 16x4"]
    bufs, frames = _on_device(pkg, case)
    good = frames[0]
    r = pkg.Raster(_font(pkg, case.font), case.cols, case.rows, 2)
    pitch = (r.yuv_pitch + 3) // 4 * 4
    pixels = torch.full((2 * r.pitch + 64,), RI.FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((2,), 0xABABABAB - (1 << 32), dtype=torch.int32, device="cuda")
    std = orc.PALETTE_STANDARD

    def refused(fn, *args, **kw):
        with pytest.raises(RuntimeError, match="86"):
            fn(*args, stream=_stream(), **kw)

    def changed(**kw):
        f = pkg.Frame()
        C.memmove(C.byref(f), C.byref(good), C.sizeof(f))
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    try:
        # before any set
        refused(r.cells_from_images, 1, status.data_ptr())
        refused(r.run_images, 1, pixels.data_ptr(), status.data_ptr())
        refused(r.run_images_yuv420, 1, pixels.data_ptr(), status.data_ptr(), pkg.RASTER_YUV_I420)
        # the set itself: nothing refused replaces an earlier set, and there is none yet
        for mode in (-1, 9, 10):
            refused(r.set_images, mode, std, [good])
        for pal in (b"", b"a\xe2\x96", b"\xc0\x80", b"a\x1b[0m"):
            refused(r.set_images, 1, pal, [good])
        refused(r.set_images, 1, std, [])
        refused(r.set_images, 1, std, [good] * 3)
        for kw in (dict(comp=1), dict(src=None), dict(src_w=0), dict(out_h=0), dict(pad_left=-1), dict(x_ratio=(1 << 32) - 1),
                   dict(src_stride=1 << 24), dict(ops=16), dict(ops=32), dict(ops=4 | 64)):
            refused(r.set_images, 1, std, [good, changed(**kw)])
        refused(r.run_images, 1, pixels.data_ptr(), status.data_ptr())  # still nothing set
        r.set_images(case.mode, std, [good], stream=_stream())
        refused(r.set_images, 9, std, [good, good])  # a refused set leaves the earlier one in place: still one frame
        # the runs
        for n in (0, 2, 3):
            refused(r.cells_from_images, n, status.data_ptr())
            refused(r.run_images, n, pixels.data_ptr(), status.data_ptr())
            refused(r.run_images_yuv420, n, pixels.data_ptr(), status.data_ptr(), pkg.RASTER_YUV_NV12)
        refused(r.cells_from_images, 1, 0)
        refused(r.run_images, 1, pixels.data_ptr(), 0)
        refused(r.run_images, 1, 0, status.data_ptr())
        refused(r.run_images, 1, pixels.data_ptr() + 2, status.data_ptr())
        refused(r.run_images, 1, pixels.data_ptr(), status.data_ptr(), image_pitch=r.pitch - 4)
        refused(r.run_images, 1, pixels.data_ptr(), status.data_ptr(), image_pitch=r.pitch + 2)
        refused(r.run_images_yuv420, 1, pixels.data_ptr(), status.data_ptr(), 3)
        refused(r.run_images_yuv420, 1, pixels.data_ptr(), status.data_ptr(), pkg.RASTER_YUV_I420, image_pitch=pitch - 4)
        refused(r.run_images_yuv420, 1, pixels.data_ptr() + 2, status.data_ptr(), pkg.RASTER_YUV_I420)
        refused(r.run_images_yuv420, 1, pixels.data_ptr(), 0, pkg.RASTER_YUV_I420)
        torch.cuda.synchronize()
        assert (pixels.cpu().numpy() == RI.FILL).all()  # nothing was launched
        assert (status.cpu().numpy().view(np.uint32) == 0xABABABAB).all()
        # and the handle still works
        r.run_images(1, pixels.data_ptr(), status.data_ptr(), stream=_stream())
        torch.cuda.synchronize()
        name = "true_fg 48x16 -> 16x4"
        RI.check(name, case, _expected(pkg, name), pixels.cpu().numpy(), 0, r.pitch, status.cpu().numpy().view(np.uint32))
    finally:
        r.close()
