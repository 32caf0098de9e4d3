"""Grid composites through the area-average pass on the GPU (asciichat_hip_box_composites): the shared scenes against the
NumPy restatement over box_ref (tests/box_comp_ref.py) byte for byte, two ticks queued on one stream with a scratch slab
that grows, and end to end -- Box.run + Plan.render of the averaged images against the oracle's renderers over the expected
averaged image."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_comp_support as CS  # noqa: E402
import box_ref as BR  # noqa: E402
import box_support as BS  # noqa: E402
import orc  # noqa: E402

SCENES = CS.scenes()
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


def _upload(buf):
    import torch
    t = torch.from_numpy(np.array(buf, dtype=np.uint8, order="C")).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr()


def _frames(pkg, frames):
    return [pkg.Frame.from_buffer_copy(bytes(f)) for f in frames]


def _run(pkg, frames, comps, what, exp, stream=None):
    import torch
    box = pkg.Box(_frames(pkg, frames), comps=comps, stream=stream or _stream())
    assert box.pitch == BS.pitch_of(frames)
    assert not box.uniform or all(c is None for c in comps)
    images = torch.full((len(frames) * box.pitch + 256,), BS.FILL, dtype=torch.uint8, device="cuda")
    box.run(images.data_ptr(), stream=stream or _stream())
    torch.cuda.synchronize()
    BS.check_images(images.cpu().numpy(), box.pitch, frames, exp, what)
    box.close()


def test_shared_scenes_one_mixed_batch_and_one_each(pkg):
    built = {name: sc.build(_upload) for name, sc in SCENES.items()}
    imgs = [BS.noise(33, 7, 60), BS.noise(48, 9, 61)]
    placed = [BS.place(imgs[0], 99, 3, base=0), BS.place(imgs[1], base=0)]
    dev = [_upload(b) for b, _, _ in placed]
    plain = [BS.frame_for(dev[0][1] + placed[0][1], 33, 7, 5, 2, 99, BS.FLIP_X), BS.frame_for(dev[1][1] + placed[1][1], 48, 9, 16, 3)]
    plain_exp = [BR.box_ref(imgs[0], 5, 2, True, False), BR.box_ref(imgs[1], 16, 3)]
    frames, comps, exp = [plain[0]], [None], [plain_exp[0]]
    for name, sc in SCENES.items():
        comp = built[name][0]
        for ow, oh, fl in sc.sizes:
            frames.append(CS.frame_for(comp, ow, oh, fl))
            comps.append(comp)
            exp.append(sc.expected(comp, ow, oh, fl))
    frames.append(plain[1])
    comps.append(None)
    exp.append(plain_exp[1])
    _run(pkg, frames, comps, "mixed batch", exp)
    for i, (f, c, e) in enumerate(zip(frames, comps, exp)):
        _run(pkg, [f], [c], f"frame {i} alone", [e])


def test_thirty_two_composite_frames_two_ticks_on_one_stream(pkg):
    """create, run, update and run queued on a stream that does not wait for the null stream: tick 2 has new source contents at
    new addresses and one target's terminal grown, so its tiles outgrow the scratch slab; both ticks' images are checked"""
    import torch
    n = 32
    sizes = [(64, 36), (48, 48), (20, 30)]
    terms = [(40, 12), (30, 10)]
    side = torch.cuda.Stream()
    ticks = []
    for k in range(2):
        scs = [CS.Scene([(BS.noise(w, h, 500 + 100 * k + 10 * t + i), 0, 0) for i, (w, h) in enumerate(sizes * 3)], [],
                        term=(90, 30) if (k == 1 and t == 1) else term) for t, term in enumerate(terms)]
        built = [sc.build(_upload) for sc in scs]
        frames, comps, exp = [], [], []
        for i in range(n):
            sc, (comp, _) = scs[i % 2], built[i % 2]
            ow, oh, fl = comp.canvas_w - (i % 5), comp.canvas_h // (1 + i % 2), i % 4
            frames.append(CS.frame_for(comp, ow, oh, fl))
            comps.append(comp)
            exp.append(sc.expected(comp, ow, oh, fl))
        ticks.append((frames, comps, exp, built))
    assert ticks[1][1][1].canvas_w == 90 and ticks[0][1][1].canvas_w == 30
    pitch = max(BS.pitch_of(t[0]) for t in ticks)
    images = [torch.full((n * pitch + 256,), BS.FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    box = pkg.Box(_frames(pkg, ticks[0][0]), comps=ticks[0][1], stream=side.cuda_stream)
    box.run(images[0].data_ptr(), pitch=pitch, stream=side.cuda_stream)
    box.update(_frames(pkg, ticks[1][0]), side.cuda_stream, comps=ticks[1][1])
    assert box.pitch == BS.pitch_of(ticks[1][0]) > BS.pitch_of(ticks[0][0])
    box.run(images[1].data_ptr(), pitch=pitch, stream=side.cuda_stream)
    side.synchronize()
    for k in range(2):
        BS.check_images(images[k].cpu().numpy(), pitch, ticks[k][0], ticks[k][2], f"tick {k}")
    # the update form of every frame plain again, and box_update on a box made for composites
    img = BS.noise(16, 8, 77)
    t, addr = _upload(img)
    plain = [BS.frame_for(addr, 16, 8, 4 + i % 3, 2, 0, i % 4) for i in range(n)]
    box.update(_frames(pkg, plain), side.cuda_stream)
    out = torch.full((n * pitch + 256,), BS.FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    box.run(out.data_ptr(), pitch=pitch, stream=side.cuda_stream)
    side.synchronize()
    BS.check_images(out.cpu().numpy(), pitch, plain, [BR.box_ref(img, f.out_w, 2, bool(f.ops & 1), bool(f.ops & 2)) for f in plain],
                    "plain again")
    # refused: a frame count that is not the box's, a descriptor the plan step refuses -- and the box is as it was
    arr = (pkg.Frame * n)(*_frames(pkg, ticks[0][0]))
    assert pkg.lib().asciichat_hip_box_composites(C.byref(box._h), arr, CS.comp_array(ticks[0][1]), n - 1, side.cuda_stream) == 86
    with pytest.raises(RuntimeError):
        box.update(_frames(pkg, ticks[0][0]), side.cuda_stream, comps=ticks[0][1][:n - 1] + [CS.Composite()])  # canvas 0x0
    out.fill_(BS.FILL)
    torch.cuda.synchronize()
    box.run(out.data_ptr(), pitch=pitch, stream=side.cuda_stream)
    side.synchronize()
    BS.check_images(out.cpu().numpy(), pitch, plain, [BR.box_ref(img, f.out_w, 2, bool(f.ops & 1), bool(f.ops & 2)) for f in plain],
                    "after refused updates")
    box.close()


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
    plan.close()
    return res


def _oracle_over(avg, f, cl, rm):
    """the reference's renderer over the averaged image at its own size (its resize is the identity there), then the
    descriptor's padding as ascii_convert_with_capabilities applies it"""
    rows = f.out_h // 2 if rm == 2 else f.out_h
    body = orc.display_convert(avg, f.out_w, rows, cl, rm, False, False, False, False, 0)
    return orc.pad_height(orc.pad_width(body, f.pad_left), f.pad_top)


_big = {}


def _terminal_scenes():
    """the 60x20 scene, and one 160x48 terminal over nine sources that cycle through three 1080p images"""
    if not _big:
        imgs = [orc.frame_hash_noise(1920, 1080, 3), orc.frame_smooth(1920, 1080), orc.frame_hash_noise(1920, 1080, 4)]
        nine = CS.Scene([(imgs[i % 3], 0, 0) for i in range(9)], [], term=(160, 48))
        _big["60x20"] = (SCENES["four slots, one empty, on 60x20"], (60, 20))
        _big["160x48"] = (nine, (160, 48))
    return _big


@pytest.mark.parametrize("mode", list(CAPS))
@pytest.mark.parametrize("size", ["60x20", "160x48"])
def test_end_to_end_against_the_oracle_over_the_averaged_image(pkg, mode, size):
    import torch
    mode_id, (cl, rm) = CAPS[mode]
    sc, (tw, th) = _terminal_scenes()[size]
    comp, keep = sc.build(_upload)
    if size == "160x48":
        assert CS.geometry(comp)[:4] == ((160, 96), (3, 3), (53, 32), 9)
        assert CS.geometry(comp)[4] == [(53, 30, 53 * (k % 3), 32 * (k // 3) + 1) for k in range(9)]
    f = pkg.frame_setup(None, comp.canvas_w, comp.canvas_h, tw, th, rm, False, False, False)
    assert f is not None and (f.out_w, f.out_h) == (tw, 2 * th if rm == 2 else th)
    box = pkg.Box([f, f], comps=[comp, comp], stream=_stream())
    images = torch.full((2 * box.pitch,), BS.FILL, dtype=torch.uint8, device="cuda")
    dense = box.render_frames(images.data_ptr())
    assert all(not d.comp and d.src == images.data_ptr() + i * box.pitch for i, d in enumerate(dense))
    box.run(images.data_ptr(), stream=_stream())
    got = _render(pkg, mode_id, dense, _stream())
    exp = _oracle_over(sc.expected(comp, f.out_w, f.out_h), f, cl, rm)
    assert got[0] == exp and got[1] == exp, f"{mode} {size}: {len(got[0])} vs {len(exp)} bytes"
    box.close()
