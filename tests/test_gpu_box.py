"""The area-average downscale on the GPU: the kernel against the NumPy restatement (tests/box_ref.py) through
asciichat_hip_box_downscale and through Box, and end to end -- Box.run + Plan.render of the averaged images against the
oracle's renderers over box_ref(img) at that image's own size, byte for byte."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_ref as BR  # noqa: E402
import box_support as BS  # noqa: E402
import orc  # noqa: E402

CASES = BS.cases()
# mode -> the oracle's (color_level, render_mode)
CAPS = {"TRUE_FG": (1, (3, 0)), "256_FG": (2, (2, 0)), "MONO": (0, (0, 0)), "HB_TRUE": (5, (3, 2))}


@pytest.fixture(scope="module")
def pkg():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from __graft_entry__ import load_package

    p = load_package()
    assert torch.cuda.is_available() and p.lib().asciichat_hip_device_count() > 0
    return p


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a, dtype=np.uint8, order="C")).cuda()  # (a copy: shared inputs stay read-only)
    assert t.data_ptr() % 16 == 0
    return t


def _frame(pkg, addr, w, h, ow, oh, stride=0, flips=0):
    f = pkg.Frame()
    f.src, f.src_w, f.src_h, f.out_w, f.out_h, f.src_stride, f.ops = addr, w, h, ow, oh, stride, flips
    f.x_ratio, f.y_ratio = (w << 16) // ow + 1, (h << 16) // oh + 1
    return f


def _placed_cases(pkg):
    """every shared case on the device: [(name, frame, device tensor)]"""
    out = []
    for name, (img, ow, oh, stride, off, fl) in CASES.items():
        h, w = img.shape[:2]
        buf, start, _ = BS.place(img, stride, off, base=0)
        t = _dev(buf)
        out.append((name, _frame(pkg, t.data_ptr() + start, w, h, ow, oh, stride, fl), t))
    return out


def test_shared_cases_through_box_downscale(pkg):
    import torch
    for name, f, t in _placed_cases(pkg):
        nb = 3 * f.out_w * f.out_h
        images = torch.full((nb + 256,), BS.FILL, dtype=torch.uint8, device="cuda")
        pkg.box_downscale(f.src, f.src_w, f.src_h, images.data_ptr(), f.out_w, f.out_h, f.src_stride,
                          bool(f.ops & BS.FLIP_X), bool(f.ops & BS.FLIP_Y), _stream())
        torch.cuda.synchronize()
        BS.check_images(images.cpu().numpy(), nb + 256, [f], [BS.expected(name, CASES[name])], name)


def test_shared_cases_through_box_one_mixed_batch_and_one_each(pkg):
    import torch
    placed = _placed_cases(pkg)
    frames = [f for _, f, _ in placed]
    exp = [BS.expected(name, CASES[name]) for name, _, _ in placed]
    box = pkg.Box(frames)
    assert not box.uniform and box.pitch == BS.pitch_of(frames)
    images = torch.full((len(frames) * box.pitch + 256,), BS.FILL, dtype=torch.uint8, device="cuda")
    box.run(images.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    BS.check_images(images.cpu().numpy(), box.pitch, frames, exp, "mixed batch")
    box.close()
    for (name, f, _), e in zip(placed, exp):
        box = pkg.Box([f])
        assert box.uniform
        images = torch.full((box.pitch + 256,), BS.FILL, dtype=torch.uint8, device="cuda")
        box.run(images.data_ptr(), stream=_stream())
        torch.cuda.synchronize()
        BS.check_images(images.cpu().numpy(), box.pitch, [f], [e], name)
        box.close()


_big = {}


def _big_frames(w, h):
    if (w, h) not in _big:
        a = np.stack([orc.frame_hash_noise(w, h, 3), orc.frame_hash_noise(w, h, 4)])
        a.setflags(write=False)
        _big[(w, h)] = a
    return _big[(w, h)]


@pytest.mark.parametrize("w,h,ow,oh", [(1920, 1080, 80, 24), (3840, 2160, 200, 60), (3840, 2160, 400, 240)])
def test_two_large_frames(pkg, w, h, ow, oh):
    """(the 4K frames reach row offsets beyond 2^24 bytes)"""
    import torch
    src = _big_frames(w, h)
    t = _dev(src)
    frames = [_frame(pkg, t.data_ptr() + i * 3 * w * h, w, h, ow, oh) for i in range(2)]
    box = pkg.Box(frames)
    assert box.uniform
    images = torch.full((2 * box.pitch + 256,), BS.FILL, dtype=torch.uint8, device="cuda")
    box.run(images.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    BS.check_images(images.cpu().numpy(), box.pitch, frames, [BR.box_ref(src[i], ow, oh) for i in range(2)], f"{w}x{h}")
    box.close()


@pytest.mark.parametrize("out", [1, 2])
def test_white_4k_frame_averages_to_white(pkg, out):
    import torch
    t = torch.full((3840 * 2160 * 3,), 255, dtype=torch.uint8, device="cuda")
    images = torch.full((3 * out * out + 256,), BS.FILL, dtype=torch.uint8, device="cuda")
    pkg.box_downscale(t.data_ptr(), 3840, 2160, images.data_ptr(), out, out, stream=_stream())
    torch.cuda.synchronize()
    got = images.cpu().numpy()
    assert (got[:3 * out * out] == 255).all() and (got[3 * out * out:] == BS.FILL).all()


def _source_720p():
    img = orc.frame_smooth(1280, 720)
    img[100:400, 300:900] = orc.frame_hash_noise(600, 300, 9)
    img[500:700, 50:1200:2] = 0  # thin detail: what point sampling aliases
    return img


def _render(pkg, mode, frames, stream):
    """-> the frames' bytes"""
    import torch
    plan = pkg.Plan(mode, orc.PALETTE_STANDARD, frames)
    n = len(frames)
    out = torch.zeros(n * plan.stride, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    plan.render(out.data_ptr(), plan.stride, ln.data_ptr(), stream)
    torch.cuda.synchronize()
    host, lens = out.cpu().numpy(), ln.cpu().numpy()
    res = [bytes(host[i * plan.stride:i * plan.stride + (int(lens[i]) & 0xFFFFFFFF)]) for i in range(n)]
    variant = plan.variant
    plan.close()
    return res, variant


def _oracle_over(avg, f, cl, rm, color_filter=0):
    """the reference's renderer over the averaged image at its own size (its resize is the identity there), then the
    descriptor's padding as ascii_convert_with_capabilities applies it"""
    rows = f.out_h // 2 if rm == 2 else f.out_h
    body = orc.display_convert(avg, f.out_w, rows, cl, rm, False, False, False, False, color_filter)
    return orc.pad_height(orc.pad_width(body, f.pad_left), f.pad_top)


@pytest.mark.parametrize("mode", list(CAPS))
@pytest.mark.parametrize("padded", [False, True])
def test_end_to_end_against_the_oracle_over_the_averaged_image(pkg, mode, padded):
    import torch
    mode_id, (cl, rm) = CAPS[mode]
    img = _source_720p()
    t = _dev(img)
    f = pkg.frame_setup(t.data_ptr(), 1280, 720, 120, 40, rm, padded, padded, False)
    assert f is not None and (not padded or f.pad_left > 0 or f.pad_top > 0)
    box = pkg.Box([f, f])
    images = torch.full((2 * box.pitch,), BS.FILL, dtype=torch.uint8, device="cuda")
    dense = box.render_frames(images.data_ptr())
    box.run(images.data_ptr(), stream=_stream())
    got, _ = _render(pkg, mode_id, dense, _stream())
    exp = _oracle_over(BR.box_ref(img, f.out_w, f.out_h), f, cl, rm)
    assert got[0] == exp and got[1] == exp, f"{mode} padded={padded}: {len(got[0])} vs {len(exp)} bytes"
    assert exp != orc.convert_with_caps(img, 120, 40, cl, rm, padded, padded, False)  # not the parity result, by design
    box.close()


def test_end_to_end_with_both_flips_and_a_tint(pkg):
    import torch
    img = _source_720p()
    t = _dev(img)
    f = pkg.frame_setup(t.data_ptr(), 1280, 720, 120, 40, 0, False, False, False)
    assert pkg.lib().achip_frame_set_display_ops(C.byref(f), True, True, 7) == 0
    box = pkg.Box([f])
    images = torch.full((box.pitch,), BS.FILL, dtype=torch.uint8, device="cuda")
    dense = box.render_frames(images.data_ptr())
    assert dense[0].ops == f.ops & ~3 and dense[0].ops != 0
    box.run(images.data_ptr(), stream=_stream())
    got, _ = _render(pkg, 1, dense, _stream())
    assert got[0] == _oracle_over(BR.box_ref(img, f.out_w, f.out_h, True, True), f, 3, 0, color_filter=7)
    box.close()


def test_thirty_two_frames_two_ticks_on_one_stream(pkg):
    """update, run and render queued back to back: tick 2's images must come from tick 2's sources"""
    import torch
    n, w, h, ow, oh = 32, 160, 90, 40, 12
    ticks = [np.stack([BS.noise(w, h, 1000 * k + i) for i in range(n)]) for k in range(2)]
    devs = [_dev(a) for a in ticks]
    stream = _stream()

    def frames(k, ragged):
        fs = [pkg.frame_setup(devs[k].data_ptr() + i * 3 * w * h, w, h, ow, oh, 0, False, False, False) for i in range(n)]
        if ragged:  # one frame flipped: the batch takes the descriptor array, refreshed by update
            assert pkg.lib().achip_frame_set_display_ops(C.byref(fs[5]), True, False, 0) == 0
        return fs

    for ragged in (False, True):
        box = pkg.Box(frames(0, ragged))
        assert box.uniform == (not ragged)
        images = torch.full((n * box.pitch,), BS.FILL, dtype=torch.uint8, device="cuda")
        plan = pkg.Plan(1, orc.PALETTE_STANDARD, box.render_frames(images.data_ptr()))
        outs = [torch.zeros(n * plan.stride, dtype=torch.uint8, device="cuda") for _ in range(2)]
        lens = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
        for k in range(2):
            if k:
                box.update(frames(k, ragged), stream)
            box.run(images.data_ptr(), stream=stream)
            plan.render(outs[k].data_ptr(), plan.stride, lens[k].data_ptr(), stream)
        torch.cuda.synchronize()
        for k in range(2):
            host, ln = outs[k].cpu().numpy(), lens[k].cpu().numpy()
            for i in range(n):
                avg = BR.box_ref(ticks[k][i], ow, oh, ragged and i == 5, False)
                exp = orc.display_convert(avg, ow, oh, 3, 0)
                got = bytes(host[i * plan.stride:i * plan.stride + (int(ln[i]) & 0xFFFFFFFF)])
                assert got == exp, f"ragged={ragged} tick {k} frame {i}"
        plan.close()
        box.close()


def test_identity_size_gives_the_point_sampled_plans_bytes_and_its_geometry(pkg):
    import torch
    w, h, n = 120, 40, 4
    src = np.stack([BS.noise(w, h, 50 + i) for i in range(n)])
    t = _dev(src)
    ident = []
    for i in range(n):
        f = pkg.Frame()
        assert pkg.lib().achip_frame_identity(C.byref(f), t.data_ptr() + i * 3 * w * h, w, h) == 0
        ident.append(f)
    box = pkg.Box(ident)
    images = torch.full((n * box.pitch,), BS.FILL, dtype=torch.uint8, device="cuda")
    dense = box.render_frames(images.data_ptr())
    for i, (d, f) in enumerate(zip(dense, ident)):  # indistinguishable from identity descriptors of that size, but for src
        assert d.src == images.data_ptr() + i * box.pitch
        d2 = pkg.Frame.from_buffer_copy(bytes(d))
        d2.src = f.src
        assert bytes(d2) == bytes(f)
    box.run(images.data_ptr(), stream=_stream())
    for mode in (1, 0, 5):
        got, v_dense = _render(pkg, mode, dense, _stream())
        direct, v_ident = _render(pkg, mode, ident, _stream())
        assert got == direct and v_dense == v_ident, f"mode {mode}"
    box.close()


def test_refusals_on_the_device(pkg):
    import torch
    img, other = BS.noise(8, 4, 70), BS.noise(8, 4, 71)
    t, t2 = _dev(img), _dev(other)
    good = _frame(pkg, t.data_ptr(), 8, 4, 2, 2)
    box = pkg.Box([good])
    images = torch.full((box.pitch + 256,), BS.FILL, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        box.run(images.data_ptr(), pitch=8)  # below an image's 12 bytes
    torch.cuda.synchronize()
    assert (images.cpu().numpy() == BS.FILL).all()  # nothing was launched
    bad = _frame(pkg, t2.data_ptr(), 8, 4, 2, 2, stride=23)
    with pytest.raises(RuntimeError):
        box.update([bad])
    box.run(images.data_ptr(), stream=_stream())  # the refused update left the box as it was: the first source, averaged
    torch.cuda.synchronize()
    BS.check_images(images.cpu().numpy(), box.pitch, [good], [BR.box_ref(img, 2, 2)], "after a refused update")
    assert not np.array_equal(BR.box_ref(img, 2, 2), BR.box_ref(other, 2, 2))
    box.close()
    comp = _frame(pkg, t.data_ptr(), 8, 4, 2, 2)
    comp.comp = t.data_ptr()
    with pytest.raises(RuntimeError, match="30"):
        pkg.Box([comp])


def test_mixed_batch_first_run_on_a_non_blocking_stream(pkg):
    """create's descriptor upload is complete when it returns: a first run on a stream that does not wait for the null stream
    (no update in between) reads the descriptors of this batch"""
    import torch
    shapes = [(48, 9, 16, 3, 0), (33, 7, 5, 2, BS.FLIP_X), (130, 20, 9, 5, 0), (40, 10, 7, 3, BS.FLIP_Y)]
    imgs = [BS.noise(w, h, 300 + k) for k, (w, h, _, _, _) in enumerate(shapes)]
    devs = [_dev(i) for i in imgs]
    frames = [_frame(pkg, d.data_ptr(), w, h, ow, oh, 0, fl) for d, (w, h, ow, oh, fl) in zip(devs, shapes)]
    exp = [BR.box_ref(i, ow, oh, bool(fl & BS.FLIP_X), bool(fl & BS.FLIP_Y)) for i, (_, _, ow, oh, fl) in zip(imgs, shapes)]
    side = torch.cuda.Stream()  # hipStreamNonBlocking
    torch.cuda.synchronize()
    for _ in range(3):
        images = torch.full((len(frames) * BS.pitch_of(frames) + 256,), BS.FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        box = pkg.Box(frames)
        assert not box.uniform
        box.run(images.data_ptr(), stream=side.cuda_stream)
        side.synchronize()
        BS.check_images(images.cpu().numpy(), box.pitch, frames, exp, "first run on a side stream")
        box.close()
