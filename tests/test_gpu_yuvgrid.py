"""YUV sources as the tiles of grid composites on the GPU: every shared case of yuvgrid_support.py through libasciichat_yuvgrid.so
into a guard-filled slab against the NumPy restatement (tests/yuvgrid_ref.py); a Plan over the uploaded rewritten descriptor
against the Plan over the uploaded original whose sources are asciichat_yuv_run_whole's frames, and against the oracle; two ticks
queued on one stream; the refusals through the real library."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orc  # noqa: E402
import yuv_support as YS  # noqa: E402
import yuvgrid_support as GS  # noqa: E402
from achip_ctypes import MODE_CAPS  # noqa: E402

CASES = GS.cases()
MODES = {1: "TRUE_FG", 5: "HB_TRUE", 9: "16_DITHER_BG"}


@pytest.fixture(scope="module")
def pkg():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from __graft_entry__ import load_package

    p = load_package()
    assert torch.cuda.is_available() and p.yuvgrid_lib().asciichat_yuvgrid_device_count() > 0
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
    p = GS.Placed(case, {k: t.data_ptr() for k, t in srcs.items()}, addresses, pkg.Composite, pkg.YuvSource, whole=extra is not None)
    p.keep = (srcs, rgbs)
    return p


def _slab(case):
    """-> (device tensor of guard bytes, byte index of tile 0)"""
    import torch
    size = GS.slab(case)[0].size
    t = torch.full((size,), GS.FILL, dtype=torch.uint8, device="cuda")
    return t, GS.slab(case, base=t.data_ptr())[1]


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
    g = pkg.YuvGrid(case.max_tiles)
    try:
        _set(g, p, _stream())
        assert g.tiles_bytes() == case.layout()[1]
        g.run(tiles if case.tiles else 0, stream=_stream())
        torch.cuda.synchronize()
        out = g.composites(tiles if case.tiles else 0)
    finally:
        g.close()
    GS.check_slab(name, case, slab.cpu().numpy(), start)
    GS.check_rewrite(name, case, p.comps, out, tiles)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
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
    """queue one render -> (out, lens) device tensors"""
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


@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES.values()))
def test_plan_over_the_tiles_equals_plan_over_run_whole(pkg, mode):
    """the 3x3 case: set, run, plan_render on one stream over the uploaded rewritten descriptor, against the plan over the
    uploaded original descriptor whose sources are run_whole's frames; TRUE_FG against the oracle's text too"""
    import torch
    case = CASES[GS.GRID_3X3]
    comp = case.comps[0]
    stream = _stream()
    rgb, whole_at = _whole_frames(pkg, case, stream)
    p = _place(pkg, case, extra=whole_at)
    slab, start = _slab(case)
    tiles = slab.data_ptr() + start
    g = pkg.YuvGrid(9)
    ups = []
    try:
        _set(g, p, stream)
        ups = [_Uploaded(pkg, g.composites(tiles)[0]), _Uploaded(pkg, p.whole[0])]
        plans = [pkg.Plan(mode, orc.PALETTE_STANDARD, [_frame(pkg, comp, u.dev, mode)]) for u in ups]
        g.run(tiles, stream=stream)
        results = [_render(pl, stream) for pl in plans]
        torch.cuda.synchronize()
        got, want = [_text(*r) for r in results]
        for pl in plans:
            pl.close()
    finally:
        g.close()
        for u in ups:
            u.close()
    assert got == want and len(got) > 100, f"{MODES[mode]}: {len(got)} vs {len(want)} bytes"
    if mode == 1:
        assert got == GS.oracle_text(comp.oracle_canvas(), comp.term, mode)


def test_two_ticks_queued_on_one_stream(pkg):
    """set, run and render of tick 2 queued behind tick 1 with no host wait in between -- the pinned block is reused --: each
    tick's text comes from that tick's sources"""
    import torch
    ticks = [GS.GridCase([GS.grid_3x3(seed)]) for seed in (900, 1900)]
    placed = [_place(pkg, t) for t in ticks]
    slab, start = _slab(ticks[0])
    tiles = slab.data_ptr() + start
    stream = _stream()
    g = pkg.YuvGrid(9)
    up = None
    try:
        _set(g, placed[0], stream)
        first = g.composites(tiles)[0]
        # the RGB24 slot of the rewritten descriptor points at tick 0's image: both ticks share it
        placed[1].comps[0].s[4].src = placed[0].comps[0].s[4].src
        up = _Uploaded(pkg, first)
        plan = pkg.Plan(1, orc.PALETTE_STANDARD, [_frame(pkg, ticks[0].comps[0], up.dev, 1)])
        results = []
        for k in range(2):
            if k:
                _set(g, placed[k], stream)
                assert bytes(g.composites(tiles)[0]) == bytes(first)  # new plane pointers keep every tile where it was
            g.run(tiles, stream=stream)
            results.append(_render(plan, stream))
        torch.cuda.synchronize()
        texts = [_text(*r) for r in results]
        plan.close()
    finally:
        g.close()
        if up:
            up.close()
    for k, t in enumerate(ticks):
        comp = t.comps[0]
        canvas = comp.oracle_canvas()
        if k:  # (slot 4 shows tick 0's RGB24 image in both)
            s = comp.slots[4]
            canvas[s.org_y:s.org_y + s.tile_h, s.org_x:s.org_x + s.tile_w] = orc.resize_nn(ticks[0].comps[0].slots[4].rgb(), s.tile_w, s.tile_h)
        assert texts[k] == GS.oracle_text(canvas, comp.term, 1), f"tick {k}"
    assert texts[0] != texts[1]


# ---- the refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(pkg):
    import torch

    def new_slab(case):
        slab, start = _slab(case)
        return slab.data_ptr() + start, lambda: (slab.cpu().numpy(), start)

    GS.check_refusals(GS.bind(pkg.yuvgrid_lib()), lambda case: _place(pkg, case), new_slab, _stream(), torch.cuda.synchronize)
