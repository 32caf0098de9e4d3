"""The YUV tiles of grid composites box-averaged straight from their planes, on the GPU: every shared case of
yuvboxgrid_support.py through libasciichat_yuvboxgrid.so into a guard-filled slab against tests/yuvbox_ref.py; two ticks queued
on one stream; the cross-library claim of include/asciichat_yuvboxgrid.h per format -- asciichat_hip_box_composites over the
rewritten descriptors against asciichat_yuv_run_whole + asciichat_hip_box_composites, and a Plan over the uploaded rewritten
descriptor against a Plan over tiles asciichat_hip_box_downscale makes of the whole frames --; the refusals through the real
library."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_comp_support as CS  # noqa: E402
import orc  # noqa: E402
import yuv_ref as YR  # noqa: E402
import yuv_support as YS  # noqa: E402
import yuvgrid_support as GS  # noqa: E402
import yuvboxgrid_support as XS  # noqa: E402
from achip_ctypes import MODE_CAPS  # noqa: E402

CASES = XS.cases()
MODES = {1: "TRUE_FG", 5: "HB_TRUE"}


@pytest.fixture(scope="module")
def pkg():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from __graft_entry__ import load_package

    p = load_package()
    assert torch.cuda.is_available() and p.yuvboxgrid_lib().asciichat_yuvboxgrid_device_count() > 0
    return p


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a, dtype=np.uint8, order="C")).cuda()  # (a copy: shared inputs stay read-only)
    assert t.data_ptr() % 16 == 0
    return t


def _place(pkg, case, extra=None):
    """the case's sources and RGB24 images on the device.  extra: {id(array): address} of images that lie there already"""
    srcs = {id(s): _dev(s.image) for s in case.srcs()}
    rgbs = {id(a): _dev(a) for a in case.rgbs()}
    addresses = {k: t.data_ptr() for k, t in rgbs.items()}
    addresses.update(extra or {})
    p = XS.Placed(case, {k: t.data_ptr() for k, t in srcs.items()}, addresses, pkg.Composite, pkg.YuvSource, whole=extra is not None)
    p.keep = (srcs, rgbs)
    return p


def _slab(case):
    """-> (device tensor of guard bytes, byte index of tile 0)"""
    import torch
    size = XS.slab(case)[0].size
    t = torch.full((size,), XS.FILL, dtype=torch.uint8, device="cuda")
    return t, XS.slab(case, base=t.data_ptr())[1]


def _set(grid, p, stream):
    grid.set(p.comps, [list(a) for a in p.nines], stream=stream)


# ---- the case table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_cases(pkg, name):
    import torch
    case = CASES[name]
    p = _place(pkg, case)
    slab, start = _slab(case)
    tiles = slab.data_ptr() + start
    g = pkg.YuvBoxGrid(case.max_tiles)
    try:
        _set(g, p, _stream())
        assert g.tiles_bytes() == case.layout()[1]
        g.run(tiles, stream=_stream())
        torch.cuda.synchronize()
        out = g.composites(tiles)
    finally:
        g.close()
    XS.check_slab(name, case, slab.cpu().numpy(), start)
    XS.check_rewrite(name, case, p.comps, out, tiles)


def test_two_ticks_queued_on_one_stream(pkg):
    """set and run of tick 2 queued behind tick 1 with no host wait in between -- the pinned block is reused --: other planes,
    other formats, the same geometry; each tick's slab holds that tick's tiles"""
    import torch
    ticks = [XS.mixed_set(700), XS.mixed_set(1700, shift=1)]
    placed = [_place(pkg, t) for t in ticks]
    slabs = [_slab(t) for t in ticks]
    stream = _stream()
    g = pkg.YuvBoxGrid(20)
    try:
        for p, (slab, start) in zip(placed, slabs):
            _set(g, p, stream)
            g.run(slab.data_ptr() + start, stream=stream)
        torch.cuda.synchronize()
    finally:
        g.close()
    for k, (t, (slab, start)) in enumerate(zip(ticks, slabs)):
        XS.check_slab(f"tick {k}", t, slab.cpu().numpy(), start)
    assert not np.array_equal(ticks[0].expected()[0], ticks[1].expected()[0])


# ---- the cross-library claim ------------------------------------------------------------------------------------------------------
class _Uploaded:
    def __init__(self, pkg, comp):
        self.pkg, self.dev = pkg, C.c_void_p()
        assert pkg.lib().asciichat_hip_composite_upload(C.byref(comp), C.byref(self.dev)) == 0 and self.dev.value

    def close(self):
        self.pkg.lib().asciichat_hip_free(self.dev)


def _frame(pkg, comp, dev, mode):
    tw, th = comp.term
    rm = MODE_CAPS[mode][1]
    f = pkg.frame_setup(None, tw, 2 * th, tw, 2 * th if rm == 2 else th, rm, True, True, False)
    assert f is not None
    f.comp = dev.value
    return f


def _render(plan, stream):
    import torch
    out = torch.zeros(plan.stride, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(1, dtype=torch.int32, device="cuda")
    plan.render(out.data_ptr(), plan.stride, ln.data_ptr(), stream)
    return out, ln


def _text(out, ln):
    return bytes(out.cpu().numpy()[:int(ln.cpu().numpy()[0]) & 0xFFFFFFFF])


def _whole_frames(pkg, case, stream):
    """asciichat_yuv_run_whole of the case's YUV sources -> (tensor to keep, {id(whole conversion): its address})"""
    import torch
    srcs = case.srcs()
    devs = [_dev(s.image) for s in srcs]
    y = pkg.Yuv(len(srcs))
    try:
        y.set([s.c_source(d.data_ptr(), pkg.YuvSource) for s, d in zip(srcs, devs)], None, stream=stream)
        pitch = y.whole_pitch
        rgb = torch.zeros(len(srcs) * pitch, dtype=torch.uint8, device="cuda")
        y.run_whole(rgb.data_ptr(), pitch, stream=stream)
        torch.cuda.synchronize()
    finally:
        y.close()
    return rgb, {id(s.whole()): rgb.data_ptr() + i * pitch for i, s in enumerate(srcs)}


def _box_images(pkg, comp_desc, out_w, out_h, stream):
    """asciichat_hip_box_composites of one composite frame -> the guard-filled buffer it ran into, as an array"""
    import torch
    frame = pkg.Frame.from_buffer_copy(bytes(CS.frame_for(comp_desc, out_w, out_h)))
    box = pkg.Box([frame], comps=[comp_desc], stream=stream)
    try:
        images = torch.full((box.pitch + 256,), XS.FILL, dtype=torch.uint8, device="cuda")
        box.run(images.data_ptr(), stream=stream)
        torch.cuda.synchronize()
    finally:
        box.close()
    return images.cpu().numpy()


@pytest.mark.parametrize("fmt", YS.FORMATS, ids=[YR.NAMES[f] for f in YS.FORMATS])
def test_the_pass_replaces_run_whole_in_front_of_box_composites_and_of_the_renderers(pkg, fmt):
    """one composite of nine 64x48 sources (3x3, canvas 48x36), averaged to 24x18.
    Use (b): route A, Yuv.run_whole into a slab and box_composites over descriptors pointing into it; route B, YuvBoxGrid set /
    run / composites and box_composites over the rewritten descriptors -- images and guard bytes equal.
    Use (a): Plan.render over the uploaded rewritten descriptor equals the render over the same descriptor whose tiles
    asciichat_hip_box_downscale made of route A's whole frames, in the same slab layout."""
    import torch
    srcs = [YS.Src(fmt, 64, 48, 400 + 10 * fmt + i, offs=(i % 4, 0, (i + 1) % 4)) for i in range(9)]
    sizes = [(16, 12), (15, 12), (16, 11), (13, 9), (16, 12), (5, 3), (12, 12), (16, 10), (14, 7)]
    comp = XS.Comp((48, 36), (3, 3), (16, 12), [XS.Slot(s, tw, th, (k % 3) * 16 + (16 - tw) // 2, (k // 3) * 12 + (12 - th) // 2)
                                               for k, (s, (tw, th)) in enumerate(zip(srcs, sizes))])
    case = XS.BoxGridCase([comp])
    stream = _stream()
    rgb, whole_at = _whole_frames(pkg, case, stream)
    p = _place(pkg, case, extra=whole_at)
    slab, start = _slab(case)
    tiles = slab.data_ptr() + start
    twin, twin_start = _slab(case)  # the same layout, filled by box_downscale of the whole frames
    twin_tiles = twin.data_ptr() + twin_start
    g = pkg.YuvBoxGrid(9)
    ups = []
    try:
        _set(g, p, stream)
        g.run(tiles, stream=stream)
        rewritten, twin_desc = g.composites(tiles)[0], g.composites(twin_tiles)[0]
        torch.cuda.synchronize()
        XS.check_slab(YR.NAMES[fmt], case, slab.cpu().numpy(), start)
        # use (b)
        a = _box_images(pkg, p.whole[0], 24, 18, stream)
        b = _box_images(pkg, rewritten, 24, 18, stream)
        assert np.array_equal(a, b) and (a[3 * 24 * 18:] == XS.FILL).all() and len(set(a[:3 * 24 * 18].tolist())) > 50
        # use (a)
        for k, s in enumerate(comp.slots):
            d = twin_desc.s[k]
            pkg.box_downscale(whole_at[id(s.source.whole())], 64, 48, d.src, s.tile_w, s.tile_h, stream=stream)
        torch.cuda.synchronize()
        assert np.array_equal(twin.cpu().numpy(), slab.cpu().numpy())  # (step (1) of route A, tile by tile)
        ups = [_Uploaded(pkg, rewritten), _Uploaded(pkg, twin_desc)]
        for mode in MODES:
            plans = [pkg.Plan(mode, orc.PALETTE_STANDARD, [_frame(pkg, comp, u.dev, mode)]) for u in ups]
            results = [_render(pl, stream) for pl in plans]
            torch.cuda.synchronize()
            got, want = [_text(*r) for r in results]
            for pl in plans:
                pl.close()
            assert got == want and len(got) > 48 * 18, f"{MODES[mode]}: {len(got)} vs {len(want)} bytes"
    finally:
        g.close()
        for u in ups:
            u.close()


# ---- the refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(pkg):
    import torch

    def new_slab(case):
        slab, start = _slab(case)
        return slab.data_ptr() + start, lambda: (slab.cpu().numpy(), start)

    XS.check_refusals(XS.bind(pkg.yuvboxgrid_lib()), lambda case: _place(pkg, case), new_slab, _stream(), torch.cuda.synchronize)
