"""Cells straight from frame descriptors in the Floyd-Steinberg mode on the GPU: every shared case of raster_dither_support.py
through Raster.set_images_dithered and Raster.run_images into a guard-filled buffer, sources as device tensors and composites
uploaded by asciichat_hip_composite_upload, against the oracle's dithered text parsed and painted by the restatement and against
the device's own chain -- Plan.render of the same descriptors in mode 9 into a slab, then Raster.run --, pixels and status equal;
the YUV entry against raster_yuv_ref over the expected pixels; sets of the three entries replacing each other on one handle; the
refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orc  # noqa: E402
import raster_composites_support as RC  # noqa: E402
import raster_dither_support as RD  # noqa: E402
import raster_images_support as RI  # noqa: E402
import raster_support as RS  # noqa: E402
import raster_yuv_ref as YR  # noqa: E402

CASES = RD.cases()
YUV_CASES = ["background 48x16 -> 16x4", RD.COMPOSITE]  # (even pixel sizes: the face's cell is 6 x 11, so an even number of rows)


@pytest.fixture(scope="module")
def pkg():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from __graft_entry__ import load_package

    p = load_package()
    assert torch.cuda.is_available() and p.raster_lib().asciichat_raster_device_count() > 0
    return p


class _World:
    """the source buffers and the composites the cases use, on the device once"""

    def __init__(self, pkg):
        self.pkg, self.keep, self.dev, self.src = pkg, {}, {}, {}

    def comp(self, k):
        import torch
        if k.name not in self.dev:
            t = [None if i is None else torch.from_numpy(i).cuda() for i in k.imgs]
            host = k.descriptor(self.pkg.lib(), [None if x is None else x.data_ptr() for x in t], self.pkg.Composite)
            d = C.c_void_p()
            assert self.pkg.lib().asciichat_hip_composite_upload(C.byref(host), C.byref(d)) == 0 and d.value
            self.keep[k.name], self.dev[k.name] = t, d
        return self.dev[k.name].value

    def source(self, s):
        import torch
        if id(s) not in self.src:
            self.src[id(s)] = (s, torch.from_numpy(s.buf).cuda())
        return self.src[id(s)][1].data_ptr()

    def frames(self, case):
        case.size(self.pkg.lib(), self.pkg.Frame)
        return RD.descriptors(self.pkg.lib(), self.pkg.Frame, case, self.comp, self.source)

    def close(self):
        for d in self.dev.values():
            self.pkg.lib().asciichat_hip_free(d)


@pytest.fixture(scope="module")
def world(pkg):
    w = _World(pkg)
    yield w
    w.close()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _font(pkg, font):
    return RS.c_font(font, pkg.RasterFont, pkg.RasterGlyph)


def _expected(pkg, name, case=None):
    return RD.expected(name, case or CASES[name], pkg.lib(), pkg.Frame)


def _render(pkg, case, frames):
    """Plan.render of the frames the case runs, in mode 9 -> (plan, slab, lengths); the caller closes the plan"""
    import torch
    plan = pkg.Plan(RD.MODE, case.palette, frames[:case.n])
    slab = torch.zeros(case.n * plan.stride, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(case.n, dtype=torch.int32, device="cuda")
    plan.render(slab.data_ptr(), plan.stride, lens.data_ptr(), _stream())
    return plan, slab, lens


@pytest.mark.parametrize("name", list(CASES))
def test_shared_cases(pkg, world, name):
    """run_images of the set into one guard-filled buffer, Plan.render -> Raster.run into a second: the first is the
    expectation's, the second is the first's"""
    import torch
    case = CASES[name]
    frames = world.frames(case)
    size = RD.pixel_buffer(case)[0].size
    pixels = [torch.full((size,), RD.FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    assert pixels[0].data_ptr() % 16 == pixels[1].data_ptr() % 16
    _, start, pitch = RD.pixel_buffer(case, base=pixels[0].data_ptr())
    status = [torch.full((len(case.frames),), 0xABABABAB - (1 << 32), dtype=torch.int32, device="cuda") for _ in range(2)]
    r = pkg.Raster(_font(pkg, case.font), case.cols, case.rows, case.max_frames)
    try:
        r.set_images_dithered(case.palette, frames, stream=_stream())
        r.run_images(case.n, pixels[0].data_ptr() + start, status[0].data_ptr(), image_pitch=pitch, stream=_stream())
        torch.cuda.synchronize()
        plan, slab, lens = _render(pkg, case, frames)
        r.run(slab.data_ptr(), plan.stride, lens.data_ptr(), case.n, pixels[1].data_ptr() + start, status[1].data_ptr(), image_pitch=pitch,
              stream=_stream())
        torch.cuda.synchronize()
        plan.close()
    finally:
        r.close()
    got, st = pixels[0].cpu().numpy(), status[0].cpu().numpy().view(np.uint32)
    RD.check(name, case, _expected(pkg, name, case), got, start, pitch, st)
    assert np.array_equal(got, pixels[1].cpu().numpy()), f"{name}: run_images and Plan.render -> run differ"
    assert np.array_equal(st, status[1].cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("layout", ["I420", "NV12"])
@pytest.mark.parametrize("name", YUV_CASES)
def test_yuv_planes(pkg, world, name, layout):
    import torch
    case = CASES[name]
    n, lay = case.n, getattr(pkg, "RASTER_YUV_" + layout)
    frames = world.frames(case)
    assert case.rows % 2 == 0 and isinstance(case.frames[0], RC.Comp) == (name == RD.COMPOSITE)
    r = pkg.Raster(_font(pkg, case.font), case.cols, case.rows, case.max_frames)
    try:
        assert r.yuv_pitch > 0
        pitch = (r.yuv_pitch + 3) // 4 * 4 + 8
        planes = torch.full((n * pitch + 64,), RD.FILL, dtype=torch.uint8, device="cuda")
        status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        r.set_images_dithered(case.palette, frames, stream=_stream())
        r.run_images_yuv420(n, planes.data_ptr(), status.data_ptr(), lay, image_pitch=pitch, stream=_stream())
        torch.cuda.synchronize()
        got = planes.cpu().numpy()
        exp = _expected(pkg, name)
        for i, (img, st, _) in enumerate(exp):
            want = YR.yuv420(img, YR.I420 if layout == "I420" else YR.NV12)
            assert want.size == r.yuv_pitch and np.array_equal(got[i * pitch:i * pitch + r.yuv_pitch], want), (name, layout, i)
            assert (got[i * pitch + r.yuv_pitch:(i + 1) * pitch] == RD.FILL).all()
            assert int(status.cpu().numpy().view(np.uint32)[i]) == st
        assert (got[n * pitch:] == RD.FILL).all()
    finally:
        r.close()


def test_sets_of_the_three_entries_replace_each_other(pkg, world):
    """on one handle, with no host wait in between: images_set in mode 1, run; images_set_dithered, run; images_set again, run;
    images_set_composites, run; images_set_dithered again, run -- each run shows the current set"""
    import torch
    plain_name, dith_name = "true_fg 48x16 -> 16x4", "foreground 48x16 -> 16x4"
    plain, dith = RI.cases()[plain_name], CASES[dith_name]
    assert (plain.cols, plain.rows, plain.atlas) == (dith.cols, dith.rows, dith.atlas)
    plain_frames = [RI.descriptor(pkg.lib(), pkg.Frame, plain.mode, s, world.source(s)) for s in plain.frames]
    dith_frames = world.frames(dith)
    r = pkg.Raster(_font(pkg, dith.font), dith.cols, dith.rows, 2)
    pixels = [torch.full((r.pitch + 64,), RD.FILL, dtype=torch.uint8, device="cuda") for _ in range(5)]
    status = [torch.full((1,), 0xABABABAB - (1 << 32), dtype=torch.int32, device="cuda") for _ in range(5)]
    try:
        for k, dithered in enumerate((False, True, False, None, True)):
            if dithered:
                r.set_images_dithered(dith.palette, dith_frames, stream=_stream())
            elif dithered is None:
                r.set_images_composites(plain.mode, plain.palette, plain_frames, stream=_stream())
            else:
                r.set_images(plain.mode, plain.palette, plain_frames, stream=_stream())
            r.run_images(1, pixels[k].data_ptr(), status[k].data_ptr(), stream=_stream())
        torch.cuda.synchronize()
    finally:
        r.close()
    exp_plain = RI.expected(plain_name, plain, pkg.lib(), pkg.Frame)
    for k, dithered in enumerate((False, True, False, None, True)):
        host, st = pixels[k].cpu().numpy(), status[k].cpu().numpy().view(np.uint32)
        if dithered:
            RD.check(dith_name, dith, _expected(pkg, dith_name), host, 0, r.pitch + 64, st)
        else:
            RI.check(plain_name, plain, exp_plain, host, 0, r.pitch + 64, st)
    assert not np.array_equal(pixels[0].cpu().numpy(), pixels[1].cpu().numpy())


def test_refusals_on_the_device(pkg, world):
    import torch
    name = "background 48x16 -> 16x4"
    case = CASES[name]
    good = world.frames(case)[0]
    comp = world.frames(CASES[RD.COMPOSITE])[0]
    r = pkg.Raster(_font(pkg, case.font), case.cols, case.rows, 2)
    pixels = torch.full((2 * r.pitch + 64,), RD.FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((2,), 0xABABABAB - (1 << 32), dtype=torch.int32, device="cuda")
    std = orc.PALETTE_STANDARD
    L = pkg.raster_lib()

    def refused(fn, *args, **kw):
        with pytest.raises(RuntimeError, match="86"):
            fn(*args, stream=_stream(), **kw)

    def changed(base=good, **kw):
        f = pkg.Frame()
        C.memmove(C.byref(f), C.byref(base), C.sizeof(f))
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    def every_refusal():
        arr = (pkg.Frame * 1)(good)
        assert L.asciichat_raster_images_set_dithered(None, std.encode(), C.cast(arr, C.c_void_p), 1, _stream()) == 86  # no handle
        assert L.asciichat_raster_images_set_dithered(r._h, None, C.cast(arr, C.c_void_p), 1, _stream()) == 86  # no palette
        assert L.asciichat_raster_images_set_dithered(r._h, std.encode(), None, 1, _stream()) == 86  # no frames
        for pal in (b"", b"a\xe2\x96", b"a\x1b[0m", b"a\x07"):
            refused(r.set_images_dithered, pal, [good])
        refused(r.set_images_dithered, std, [])
        refused(r.set_images_dithered, std, [good] * 3)
        for kw in (dict(ops=32), dict(ops=32 | 3), dict(out_w=1025), dict(ops=4 | 64), dict(ops=4 | 64 | 16), dict(src=None), dict(src_w=0),
                   dict(out_h=0), dict(pad_top=-1), dict(x_ratio=(1 << 32) - 1), dict(src_stride=1 << 24)):
            refused(r.set_images_dithered, std, [good, changed(**kw)])
        refused(r.set_images_dithered, std, [changed(comp, comp=None)])  # neither a source nor a composite
        # the other two entries still refuse the mode and the dither bits
        refused(r.set_images, 9, std, [good])
        refused(r.set_images_composites, 9, std, [good])
        refused(r.set_images, 1, std, [changed(ops=16)])
        refused(r.set_images_composites, 1, std, [changed(ops=48)])

    try:
        assert good.src and not good.comp and comp.comp and not comp.src
        every_refusal()
        refused(r.run_images, 1, pixels.data_ptr(), status.data_ptr())  # nothing was set by any of them
        r.set_images_dithered(std, [good], stream=_stream())
        every_refusal()  # a refused set leaves the earlier one in place: one frame, this one
        for n in (0, 2):
            refused(r.cells_from_images, n, status.data_ptr())
            refused(r.run_images, n, pixels.data_ptr(), status.data_ptr())
        torch.cuda.synchronize()
        assert (pixels.cpu().numpy() == RD.FILL).all() and (status.cpu().numpy().view(np.uint32) == 0xABABABAB).all()  # nothing was launched
        r.run_images(1, pixels.data_ptr(), status.data_ptr(), stream=_stream())
        torch.cuda.synchronize()
        host, st = pixels.cpu().numpy(), status.cpu().numpy().view(np.uint32)
        RD.check(name, case, _expected(pkg, name), host[:r.pitch + 64], 0, r.pitch + 64, st[:1])
        assert (host[r.pitch:] == RD.FILL).all() and st[1] == 0xABABABAB
    finally:
        r.close()
