"""Cells straight from grid composites on the GPU: every shared case of raster_composites_support.py through
Raster.set_images_composites and Raster.run_images into a guard-filled buffer, with the composites uploaded by
asciichat_hip_composite_upload and the sources as device tensors, against the oracle's text parsed and painted by the
restatement and against the device's own chain -- Plan.render of the same descriptors into a slab, then Raster.run --, pixels
and status equal; the YUV entries against run_yuv420 over Plan.render's frames; the stage alone; plain and composite frames in
one set; a plain set through either entry; the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orc  # noqa: E402
import raster_composites_support as RC  # noqa: E402
import raster_images_support as RI  # noqa: E402
import raster_support as RS  # noqa: E402

CASES = RC.cases()
# (even pixel sizes: the face's cell is 6 x 11, so an even number of rows)
YUV_CASES = [f"true_fg {RC.NINE}", "hb_256 a client without video in the middle"]
MIXED = ["true_fg mixed batch: 4 of 6 set, handle of 8", "hb_256 mixed batch: 4 of 6 set, handle of 8"]


@pytest.fixture(scope="module")
def pkg():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from __graft_entry__ import load_package

    p = load_package()
    assert torch.cuda.is_available() and p.raster_lib().asciichat_raster_device_count() > 0
    return p


class _World:
    """the sources of every composite the cases use, on the device once; its descriptor (premise asserted) uploaded once"""

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
        return RC.descriptors(self.pkg.lib(), self.pkg.Frame, case, self.comp, self.source)

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
    return RC.expected(name, case or CASES[name], pkg.lib(), pkg.Frame)


def _render(pkg, case, frames):
    """Plan.render of the frames the case runs -> (plan, slab, lengths); the caller closes the plan"""
    import torch
    plan = pkg.Plan(case.mode, case.palette, frames[:case.n])
    slab = torch.zeros(case.n * plan.stride, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(case.n, dtype=torch.int32, device="cuda")
    plan.render(slab.data_ptr(), plan.stride, lens.data_ptr(), _stream())
    return plan, slab, lens


def _both_paths(pkg, world, name, case, entry="set_images_composites"):
    """run_images of the set into one guard-filled buffer, Plan.render -> Raster.run into a second -> (pixels, status) of each,
    the first checked against the expectation"""
    import torch
    frames = world.frames(case)
    size = RC.pixel_buffer(case)[0].size
    pixels = [torch.full((size,), RC.FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    assert pixels[0].data_ptr() % 16 == pixels[1].data_ptr() % 16
    _, start, pitch = RC.pixel_buffer(case, base=pixels[0].data_ptr())
    status = [torch.full((len(case.frames),), 0xABABABAB - (1 << 32), dtype=torch.int32, device="cuda") for _ in range(2)]
    r = pkg.Raster(_font(pkg, case.font), case.cols, case.rows, case.max_frames)
    try:
        getattr(r, entry)(case.mode, case.palette, frames, stream=_stream())
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
    RC.check(name, case, _expected(pkg, name, case), got, start, pitch, st)
    assert np.array_equal(got, pixels[1].cpu().numpy()), f"{name}: run_images and Plan.render -> run differ"
    assert np.array_equal(st, status[1].cpu().numpy().view(np.uint32))
    return got, st


@pytest.mark.parametrize("name", [n for n in CASES if n not in MIXED])
def test_shared_cases(pkg, world, name):
    _both_paths(pkg, world, name, CASES[name])


@pytest.mark.parametrize("name", MIXED)
def test_mixed_batch(pkg, world, name):
    """plain, composite A, composite B, A again run of six set in a handle of eight: the frames not run and their status words
    stay untouched (RC.check)"""
    case = CASES[name]
    kinds = [isinstance(it, RC.Comp) for it in case.frames]
    assert kinds[:4] == [False, True, True, True] and case.n == 4 < len(case.frames) < case.max_frames
    _both_paths(pkg, world, name, case)


@pytest.mark.parametrize("layout", ["I420", "NV12"])
@pytest.mark.parametrize("name", YUV_CASES)
def test_yuv_planes_equal_the_text_paths(pkg, world, name, layout):
    import torch
    case = CASES[name]
    n, lay = case.n, getattr(pkg, "RASTER_YUV_" + layout)
    frames = world.frames(case)
    assert case.rows % 2 == 0 and (case.mode in RC.HALF_BLOCK) == name.startswith("hb_")
    r = pkg.Raster(_font(pkg, case.font), case.cols, case.rows, case.max_frames)
    try:
        assert r.yuv_pitch > 0
        pitch = (r.yuv_pitch + 3) // 4 * 4 + 8
        planes = [torch.full((n * pitch + 64,), RC.FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
        status = [torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
        r.set_images_composites(case.mode, case.palette, frames, stream=_stream())
        r.run_images_yuv420(n, planes[0].data_ptr(), status[0].data_ptr(), lay, image_pitch=pitch, stream=_stream())
        plan, slab, lens = _render(pkg, case, frames)
        r.run_yuv420(slab.data_ptr(), plan.stride, lens.data_ptr(), n, planes[1].data_ptr(), status[1].data_ptr(), lay, image_pitch=pitch,
                     stream=_stream())
        torch.cuda.synchronize()
        plan.close()
        got = planes[0].cpu().numpy()
        assert np.array_equal(got, planes[1].cpu().numpy()) and np.array_equal(status[0].cpu().numpy(), status[1].cpu().numpy())
        used = got[:n * pitch].reshape(n, pitch)
        assert (used[:, r.yuv_pitch:] == RC.FILL).all() and (got[n * pitch:] == RC.FILL).all() and (used[:, :r.yuv_pitch] != RC.FILL).any()
        assert [int(s) for s in status[0].cpu().numpy().view(np.uint32)] == [e[1] for e in _expected(pkg, name)]
    finally:
        r.close()


def test_the_stage_alone_then_draw_equals_run_images(pkg, world):
    import torch
    name = MIXED[0]
    case = CASES[name]
    frames = world.frames(case)
    r = pkg.Raster(_font(pkg, case.font), case.cols, case.rows, case.max_frames)
    n = case.n
    pixels = [torch.full((n * r.pitch,), RC.FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    status = [torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    try:
        r.set_images_composites(case.mode, case.palette, frames, stream=_stream())
        r.run_images(n, pixels[0].data_ptr(), status[0].data_ptr(), stream=_stream())
        r.cells_from_images(n, status[1].data_ptr(), stream=_stream())
        r.draw(n, pixels[1].data_ptr(), stream=_stream())
        torch.cuda.synchronize()
    finally:
        r.close()
    assert np.array_equal(pixels[0].cpu().numpy(), pixels[1].cpu().numpy()) and np.array_equal(status[0].cpu().numpy(), status[1].cpu().numpy())
    exp = _expected(pkg, name)
    host, st = pixels[0].cpu().numpy(), status[0].cpu().numpy().view(np.uint32)
    for i, (img, want, _) in enumerate(exp):
        assert np.array_equal(host[i * r.pitch:(i + 1) * r.pitch].reshape(img.shape), img) and int(st[i]) == want, (name, i)


def test_plain_sets_are_unchanged_and_replace_a_composite_set(pkg, world):
    """on one handle, with no host wait in between: a composite set, then a set without composites through images_set, then the
    same set through images_set_composites -- the two plain runs give the same bytes, those of the expectation, and nothing of
    the composite set is left; then a composite set again"""
    import torch
    comp_name = "true_fg a client without video in the middle"
    comp = CASES[comp_name].size(pkg.lib(), pkg.Frame)
    comp_frames = world.frames(comp)
    plain = RC.plain_only_case(RC.TRUE_FG)
    plain.cols, plain.rows, plain.sized = comp.cols, comp.rows, False
    plain_frames = world.frames(plain)
    assert not any(f.comp for f in plain_frames) and all(f.comp for f in comp_frames)
    r = pkg.Raster(_font(pkg, comp.font), comp.cols, comp.rows, 2)
    pixels = [torch.full((2 * r.pitch + 64,), RC.FILL, dtype=torch.uint8, device="cuda") for _ in range(4)]
    status = [torch.full((2,), 0xABABABAB - (1 << 32), dtype=torch.int32, device="cuda") for _ in range(4)]
    try:
        r.set_images_composites(comp.mode, comp.palette, comp_frames, stream=_stream())
        r.run_images(1, pixels[0].data_ptr(), status[0].data_ptr(), stream=_stream())
        r.set_images(plain.mode, plain.palette, plain_frames, stream=_stream())
        r.run_images(2, pixels[1].data_ptr(), status[1].data_ptr(), stream=_stream())
        r.set_images_composites(plain.mode, plain.palette, plain_frames, stream=_stream())
        r.run_images(2, pixels[2].data_ptr(), status[2].data_ptr(), stream=_stream())
        r.set_images_composites(comp.mode, comp.palette, comp_frames, stream=_stream())
        r.run_images(1, pixels[3].data_ptr(), status[3].data_ptr(), stream=_stream())
        torch.cuda.synchronize()
    finally:
        r.close()
    host = [p.cpu().numpy() for p in pixels]
    st = [s.cpu().numpy().view(np.uint32) for s in status]
    assert np.array_equal(host[1], host[2]) and np.array_equal(st[1], st[2])
    key = f"{RC.PLAIN_ONLY} in {comp.cols}x{comp.rows}"
    RC.check(key, plain, _expected(pkg, key, plain), host[1], 0, r.pitch, st[1])
    for k in (0, 3):
        RC.check(comp_name, comp, _expected(pkg, comp_name), host[k][:r.pitch + 64], 0, r.pitch + 64, st[k][:1])
        assert (host[k][r.pitch:] == RC.FILL).all() and st[k][1] == 0xABABABAB


def test_refusals_on_the_device(pkg, world):
    import torch
    name = "true_fg a client without video in the middle"
    case = CASES[name].size(pkg.lib(), pkg.Frame)
    good = world.frames(case)[0]
    r = pkg.Raster(_font(pkg, case.font), case.cols, case.rows, 2)
    pixels = torch.full((2 * r.pitch + 64,), RC.FILL, dtype=torch.uint8, device="cuda")
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

    def every_refusal():
        for mode in (-1, 9, 10):
            refused(r.set_images_composites, mode, std, [good])
        for pal in (b"", b"a\xe2\x96", b"a\x1b[0m"):
            refused(r.set_images_composites, 1, pal, [good])
        refused(r.set_images_composites, 1, std, [])
        refused(r.set_images_composites, 1, std, [good] * 3)
        for kw in (dict(comp=None), dict(src_w=0), dict(out_h=0), dict(pad_left=-1), dict(x_ratio=(1 << 32) - 1), dict(ops=16), dict(ops=32),
                   dict(ops=4 | 64)):
            refused(r.set_images_composites, 1, std, [good, changed(**kw)])
        refused(r.set_images, 1, std, [good])  # images_set itself still refuses a composite

    try:
        assert good.comp and not good.src
        every_refusal()
        refused(r.run_images, 1, pixels.data_ptr(), status.data_ptr())  # nothing was set by any of them
        r.set_images_composites(case.mode, std, [good], stream=_stream())
        every_refusal()  # a refused set leaves the earlier one in place: one frame, this one
        for n in (0, 2):
            refused(r.cells_from_images, n, status.data_ptr())
            refused(r.run_images, n, pixels.data_ptr(), status.data_ptr())
        torch.cuda.synchronize()
        assert (pixels.cpu().numpy() == RC.FILL).all() and (status.cpu().numpy().view(np.uint32) == 0xABABABAB).all()  # nothing was launched
        r.run_images(1, pixels.data_ptr(), status.data_ptr(), stream=_stream())
        torch.cuda.synchronize()
        host, st = pixels.cpu().numpy(), status.cpu().numpy().view(np.uint32)
        RC.check(name, case, _expected(pkg, name), host[:r.pitch + 64], 0, r.pitch + 64, st[:1])
        assert (host[r.pitch:] == RC.FILL).all() and st[1] == 0xABABABAB
    finally:
        r.close()
