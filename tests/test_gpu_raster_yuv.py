"""The rasteriser's YUV 4:2:0 output on the GPU: the shared cases of raster_yuv_support.py through Raster.run_yuv420 in both
layouts against the restatement (tests/raster_yuv_ref.py over tests/raster_ref.py), bytes equal and nothing stored outside an
image; the planes against the conversion of the RGBA the device itself drew; refusals; and Plan.render frames end to end."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orc  # noqa: E402
import raster_support as RS  # noqa: E402
import raster_yuv_ref as YR  # noqa: E402
import raster_yuv_support as YS  # noqa: E402

CASES = YS.cases()
LAYOUTS = list(YS.LAYOUTS)


@pytest.fixture(scope="module")
def pkg():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from __graft_entry__ import load_package

    p = load_package()
    assert torch.cuda.is_available() and p.raster_lib().asciichat_raster_device_count() > 0
    assert (p.RASTER_YUV_I420, p.RASTER_YUV_NV12) == (YR.I420, YR.NV12)
    return p


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _font(pkg, font):
    return RS.c_font(font, pkg.RasterFont, pkg.RasterGlyph)


def _upload(case):
    import torch
    frames, stride, lens = RS.slab(case)
    return torch.from_numpy(frames).cuda(), stride, torch.from_numpy(lens.view(np.int32)).cuda()


def _run(pkg, name, case, layout, frames_ptr, stride, lens, max_frames=None):
    """Raster.run_yuv420 of the case's frames (already in device memory) into a guard-filled buffer, checked against the
    restatement"""
    import torch
    n = len(case.frames)
    planes = torch.full((YS.yuv_buffer(case)[0].size,), YS.FILL, dtype=torch.uint8, device="cuda")
    _, start, pitch = YS.yuv_buffer(case, base=planes.data_ptr())
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    r = pkg.Raster(_font(pkg, case.font), case.cols, case.rows, n if max_frames is None else max_frames)
    try:
        assert (r.width, r.height) == YS.size_px(case) and r.yuv_pitch == YS.image_bytes(case)
        r.run_yuv420(frames_ptr, stride, lens.data_ptr(), n, planes.data_ptr() + start, status.data_ptr(), YS.LAYOUTS[layout],
                     image_pitch=pitch, stream=_stream())
        torch.cuda.synchronize()
    finally:
        r.close()
    YS.check(name, case, YS.LAYOUTS[layout], planes.cpu().numpy(), start, pitch, status.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", [k for k, c in CASES.items() if not c.l2])  # (the library stages an atlas whenever it fits)
def test_shared_cases(pkg, name, layout):
    case = CASES[name]
    frames, stride, lens = _upload(case)
    _run(pkg, name, case, layout, frames.data_ptr(), stride, lens)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_batch_in_a_rasteriser_of_more_frames(pkg, layout):
    case = CASES["yuv batch of 40"]
    frames, stride, lens = _upload(case)
    _run(pkg, "yuv batch of 40", case, layout, frames.data_ptr(), stride, lens, max_frames=64)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["yuv chroma across four cells", "yuv three cell rows 2x4", "yuv even width, odd height", "yuv flags"])
def test_planes_are_the_conversion_of_the_rgba_the_device_drew(pkg, name, layout):
    """one handle, the same frames: run gives RGBA, run_yuv420 the planes of exactly those pixels, and so does parse followed
    by draw_yuv420"""
    import torch
    case = CASES[name]
    n = len(case.frames)
    (W, H), lay = YS.size_px(case), YS.LAYOUTS[layout]
    frames, stride, lens = _upload(case)
    r = pkg.Raster(_font(pkg, case.font), case.cols, case.rows, n)
    pitch = (r.yuv_pitch + 3) // 4 * 4
    rgba = torch.zeros(n * r.pitch, dtype=torch.uint8, device="cuda")
    planes = [torch.full((n * pitch,), YS.FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    status = [torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(3)]
    r.run(frames.data_ptr(), stride, lens.data_ptr(), n, rgba.data_ptr(), status[0].data_ptr(), stream=_stream())
    r.run_yuv420(frames.data_ptr(), stride, lens.data_ptr(), n, planes[0].data_ptr(), status[1].data_ptr(), lay, stream=_stream())
    r.parse(frames.data_ptr(), stride, lens.data_ptr(), n, status[2].data_ptr(), stream=_stream())
    r.draw_yuv420(n, planes[1].data_ptr(), lay, stream=_stream())
    torch.cuda.synchronize()
    r.close()
    img = rgba.cpu().numpy().reshape(n, H, W, 4)
    got = [p.cpu().numpy().reshape(n, pitch)[:, :r.yuv_pitch] for p in planes]
    for i in range(n):
        want = YR.yuv420(img[i], lay)
        assert np.array_equal(got[0][i], want), f"{name} frame {i}: run_yuv420, {YS.first_difference(got[0][i], want, W, H)}"
        assert np.array_equal(got[1][i], want), f"{name} frame {i}: draw_yuv420, {YS.first_difference(got[1][i], want, W, H)}"
    assert np.array_equal(status[0].cpu().numpy(), status[1].cpu().numpy()) and np.array_equal(status[0].cpu().numpy(), status[2].cpu().numpy())


def test_two_runs_of_one_rasteriser_share_no_state(pkg):
    """the pen and the cells of a run do not reach the next: a blank batch after a coloured one is blank"""
    import torch
    a = RS.Case("synth", 4, 2, [RS.fgc(9, 99, 199) + RS.bgc(1, 2, 3) + b"APLR\nBBBB"] * 2)
    b = RS.Case("synth", 4, 2, [b"A", b""])
    r = pkg.Raster(_font(pkg, RS.ATLASES["synth"]), 4, 2, 2)
    pitch = (r.yuv_pitch + 3) // 4 * 4
    for name, case in (("yuv first run", a), ("yuv second run", b)):
        frames, stride, lens = _upload(case)
        planes = torch.full((2 * pitch + 64,), YS.FILL, dtype=torch.uint8, device="cuda")
        status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        r.run_yuv420(frames.data_ptr(), stride, lens.data_ptr(), 2, planes.data_ptr(), status.data_ptr(), YR.I420, stream=_stream())
        torch.cuda.synchronize()
        YS.check(name, case, YR.I420, planes.cpu().numpy(), 0, pitch, status.cpu().numpy().view(np.uint32))
    r.close()


def test_refusals_on_the_device(pkg):
    import torch
    frames = torch.zeros(64, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(2, dtype=torch.int32, device="cuda")
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    planes = torch.full((4096,), YS.FILL, dtype=torch.uint8, device="cuda")
    args = (frames.data_ptr(), 32, lens.data_ptr())
    odd = pkg.Raster(_font(pkg, RS.ATLASES["synth"]), 3, 3, 2)  # 15 x 21
    assert odd.yuv_pitch == 0
    for lay in (YR.I420, YR.NV12):
        with pytest.raises(RuntimeError, match="86"):
            odd.run_yuv420(*args, 2, planes.data_ptr(), status.data_ptr(), lay, image_pitch=1024, stream=_stream())
        with pytest.raises(RuntimeError, match="86"):
            odd.draw_yuv420(2, planes.data_ptr(), lay, image_pitch=1024, stream=_stream())
    odd.close()
    r = pkg.Raster(_font(pkg, RS.ATLASES["synth"]), 4, 2, 2)  # 20 x 14: 420 bytes
    assert r.yuv_pitch == 420
    for bad in (dict(layout=0), dict(layout=3), dict(image_pitch=416), dict(image_pitch=422), dict(off=2), dict(n=0), dict(n=3)):
        with pytest.raises(RuntimeError, match="86"):
            r.run_yuv420(*args, bad.get("n", 2), planes.data_ptr() + bad.get("off", 0), status.data_ptr(), bad.get("layout", YR.I420),
                         image_pitch=bad.get("image_pitch"), stream=_stream())
        with pytest.raises(RuntimeError, match="86"):
            r.draw_yuv420(bad.get("n", 2), planes.data_ptr() + bad.get("off", 0), bad.get("layout", YR.I420),
                          image_pitch=bad.get("image_pitch"), stream=_stream())
    with pytest.raises(RuntimeError, match="86"):
        r.run_yuv420(0, 32, lens.data_ptr(), 2, planes.data_ptr(), status.data_ptr(), YR.I420, stream=_stream())
    torch.cuda.synchronize()
    assert (planes.cpu().numpy() == YS.FILL).all()  # nothing was launched
    r.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", ["TRUE_FG", "HB_TRUE"])
def test_plan_render_straight_into_the_planes(pkg, mode, layout):
    """16x4 frames with the `text` atlas: 96 x 44 pixels"""
    import torch
    mode_id, (cl, rm) = {"TRUE_FG": (1, (3, 0)), "HB_TRUE": (5, (3, 2))}[mode]
    img = orc.frame_hash_noise(48, 16, 3)
    img.setflags(write=False)
    dev = torch.from_numpy(np.array(img)).cuda()
    f = pkg.frame_setup(dev.data_ptr(), 48, 16, 16, 4, rm, False, False, False)
    plan = pkg.Plan(mode_id, orc.PALETTE_STANDARD, [f, f])
    out = torch.zeros(2 * plan.stride, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(2, dtype=torch.int32, device="cuda")
    plan.render(out.data_ptr(), plan.stride, ln.data_ptr(), _stream())
    exp = orc.convert_with_caps(img, 16, 4, cl, rm, False, False, False)
    case = RS.Case("text", 16, 4, [exp, exp], status=[0, 0])
    _run(pkg, f"yuv plan {mode}", case, layout, out.data_ptr(), plan.stride, ln)
    plan.close()
