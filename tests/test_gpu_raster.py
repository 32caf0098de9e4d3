"""The rasteriser on the GPU: the shared cases of raster_support.py through Raster.run against the Python restatement
(tests/raster_ref.py), bytes equal and nothing stored outside an image, and end to end -- what Plan.render, the rain pass and
ascii_create_grid produce, rasterised from device memory and compared with the restatement over the oracle's bytes."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orc  # noqa: E402
import rain_support as RN  # noqa: E402
import raster_ref as RR  # noqa: E402
import raster_support as RS  # noqa: E402

CASES = RS.cases()
# mode -> (plan mode, the oracle's (color_level, render_mode))
CAPS = {"TRUE_FG": (1, (3, 0)), "256_FG": (2, (2, 0)), "MONO": (0, (0, 0)), "HB_TRUE": (5, (3, 2))}


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


def _run(pkg, name, case, frames_ptr, stride, lens, max_frames=None):
    """Raster.run of the case's frames (already in device memory) into a guard-filled buffer, checked against the restatement"""
    import torch
    n = len(case.frames)
    size = RS.pixel_buffer(case)[0].size
    pixels = torch.full((size,), RS.FILL, dtype=torch.uint8, device="cuda")
    _, start, pitch = RS.pixel_buffer(case, base=pixels.data_ptr())
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    r = pkg.Raster(_font(pkg, case.font), case.cols, case.rows, n if max_frames is None else max_frames)
    try:
        assert (r.width, r.height, r.pitch) == (case.cols * case.font.cell_w, case.rows * case.font.cell_h, RS.image_bytes(case))
        r.run(frames_ptr, stride, lens.data_ptr(), n, pixels.data_ptr() + start, status.data_ptr(), image_pitch=pitch, stream=_stream())
        torch.cuda.synchronize()
    finally:
        r.close()
    RS.check(name, case, pixels.cpu().numpy(), start, pitch, status.cpu().numpy().view(np.uint32))


def _upload(case):
    import torch
    frames, stride, lens = RS.slab(case)
    return torch.from_numpy(frames).cuda(), stride, torch.from_numpy(lens.view(np.int32)).cuda()


@pytest.mark.parametrize("name", [k for k, c in CASES.items() if not c.l2])  # (the library stages an atlas whenever it fits)
def test_shared_cases(pkg, name):
    case = CASES[name]
    frames, stride, lens = _upload(case)
    _run(pkg, name, case, frames.data_ptr(), stride, lens)


def test_batch_in_a_rasteriser_of_more_frames(pkg):
    case = CASES["batch of 40"]
    frames, stride, lens = _upload(case)
    _run(pkg, "batch of 40", case, frames.data_ptr(), stride, lens, max_frames=64)


def test_two_runs_of_one_rasteriser_share_no_state(pkg):
    """the pen and the cells of a run do not reach the next: a blank batch after a coloured one is blank"""
    import torch
    font = RS.ATLASES["synth"]
    a = RS.Case("synth", 4, 2, [RS.fgc(9, 99, 199) + RS.bgc(1, 2, 3) + b"APLR\nBBBB"] * 2)
    b = RS.Case("synth", 4, 2, [b"A", b""])
    r = pkg.Raster(_font(pkg, font), 4, 2, 2)
    for name, case in (("first run", a), ("second run", b)):
        frames, stride, lens = _upload(case)
        pixels = torch.full((2 * r.pitch + 64,), RS.FILL, dtype=torch.uint8, device="cuda")
        status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        r.run(frames.data_ptr(), stride, lens.data_ptr(), 2, pixels.data_ptr(), status.data_ptr(), stream=_stream())
        torch.cuda.synchronize()
        RS.check(name, case, pixels.cpu().numpy(), 0, r.pitch, status.cpu().numpy().view(np.uint32))
    r.close()


def test_refusals_on_the_device(pkg):
    import torch
    r = pkg.Raster(_font(pkg, RS.ATLASES["synth"]), 3, 2, 2)
    frames = torch.zeros(64, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(2, dtype=torch.int32, device="cuda")
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    pixels = torch.full((2 * r.pitch + 64,), RS.FILL, dtype=torch.uint8, device="cuda")
    args = (frames.data_ptr(), 32, lens.data_ptr())
    for bad in (dict(n=3), dict(n=0), dict(image_pitch=r.pitch - 4), dict(image_pitch=r.pitch + 2), dict(off=2)):
        with pytest.raises(RuntimeError, match="86"):
            r.run(*args, bad.get("n", 2), pixels.data_ptr() + bad.get("off", 0), status.data_ptr(),
                  image_pitch=bad.get("image_pitch"), stream=_stream())
    with pytest.raises(RuntimeError, match="86"):
        r.run(0, 32, lens.data_ptr(), 2, pixels.data_ptr(), status.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    assert (pixels.cpu().numpy() == RS.FILL).all()  # nothing was launched
    r.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _source():
    img = orc.frame_hash_noise(48, 16, 3)
    img.setflags(write=False)
    return img


def _rasterise_device_frames(pkg, name, cols, rows, frames_ptr, stride, lens, expected_frames):
    case = RS.Case("text", cols, rows, expected_frames, status=[0] * len(expected_frames))
    _run(pkg, name, case, frames_ptr, stride, lens)


@pytest.mark.parametrize("mode", list(CAPS))
def test_plan_render_straight_into_the_rasteriser(pkg, mode):
    import torch
    mode_id, (cl, rm) = CAPS[mode]
    img = _source()
    dev = torch.from_numpy(np.array(img)).cuda()
    f = pkg.frame_setup(dev.data_ptr(), 48, 16, 16, 4, rm, False, False, False)
    plan = pkg.Plan(mode_id, orc.PALETTE_STANDARD, [f, f])
    out = torch.zeros(2 * plan.stride, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(2, dtype=torch.int32, device="cuda")
    plan.render(out.data_ptr(), plan.stride, ln.data_ptr(), _stream())
    exp = orc.convert_with_caps(img, 16, 4, cl, rm, False, False, False)
    _rasterise_device_frames(pkg, mode, 16, 4, out.data_ptr(), plan.stride, ln, [exp, exp])
    plan.close()


def _uploaded(frame):
    import torch
    stride = (len(frame) + 15) // 16 * 16
    buf = np.zeros(stride, dtype=np.uint8)
    buf[:len(frame)] = np.frombuffer(frame, dtype=np.uint8)
    return torch.from_numpy(buf).cuda(), stride, torch.tensor([len(frame)], dtype=torch.int32, device="cuda")


def test_a_digital_rain_frame(pkg):
    frame = orc.convert_with_caps(_source(), 16, 4, 3, 0, False, False, False)
    g, ref = pkg.Rain(16, 4), RN.Restated(16, 4)
    try:
        for _ in range(3):
            got, exp = g.apply(frame, 0.05), ref.apply(frame, 0.05)
    finally:
        g.close()
        ref.close()
    dev, stride, ln = _uploaded(got)
    _rasterise_device_frames(pkg, "rain", 16, 4, dev.data_ptr(), stride, ln, [exp])


def test_an_ascii_create_grid_string(pkg):
    import ctypes as C
    one = orc.convert_with_caps(_source(), 16, 4, 0, 0, False, False, False)
    exp = orc.create_grid([one, one], 40, 6)
    L = pkg.lib()
    arr = (pkg.FrameSource * 2)()
    for i in range(2):
        arr[i].frame_data, arr[i].frame_size = one, len(one)
    n = C.c_size_t()
    got = pkg.take_string(L.ascii_create_grid(arr, 2, 40, 6, C.byref(n)))
    dev, stride, ln = _uploaded(got)
    _rasterise_device_frames(pkg, "grid", 40, 6, dev.data_ptr(), stride, ln, [exp])
