"""The digital rain pass on the GPU: the drop-in digital_rain_* functions and asciichat_hip_rain_apply_batch against the
sequential restatement (tests/cabi/rain_restatement.c) and the reference-generated fixture, byte for byte and state for
state."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orc  # noqa: E402
import rain_support as RS  # noqa: E402

# (color_level, render_mode): mono, 16 / 256 / truecolor foreground, truecolor background, half blocks
CAPS = [(0, 0), (1, 0), (2, 0), (3, 0), (3, 1), (3, 2), (0, 2)]


@pytest.fixture(scope="module")
def pkg():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from __graft_entry__ import load_package

    p = load_package()
    assert torch.cuda.is_available() and p.lib().asciichat_hip_device_count() > 0
    return p


def _images():
    a = orc.frame_smooth(640, 360)
    b = a.copy()
    b[100:220, 200:420] = orc.frame_hash_noise(220, 120, 5)
    return [a, b]


def _first_diff(a, b):
    i = next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), min(len(a), len(b)))
    return f"first difference at byte {i}: gpu {a[i - 20:i + 20]!r} vs restatement {b[i - 20:i + 20]!r}"


def _same(gpu, rs, what):
    assert gpu == rs, f"{what}: {len(gpu)} vs {len(rs)} bytes; {_first_diff(gpu, rs)}"


def test_dropin_matches_fixture(pkg):
    fx = json.load(open(RS.GOLDEN))
    import hashlib
    for case in fx["cases"]:
        r = pkg.Rain(case["cols"], case["rows"])
        r.set_field = lambda name, v, s=r.s: setattr(s, name, v)
        try:
            for step in case["steps"]:
                RS.apply_ops(r, step.get("ops", []))
                out = r.apply(bytes.fromhex(step["input"]), step["dt"])
                assert len(out) == step["out_len"], f"{case['name']}: length"
                assert hashlib.sha256(out).hexdigest() == step["sha256"], f"{case['name']}: bytes"
                if "output" in step:
                    _same(out, bytes.fromhex(step["output"]), case["name"])
        finally:
            r.close()


@pytest.mark.parametrize("cols,rows", [(80, 24), (200, 60), (400, 120)])
def test_dropin_sequences_every_mode(pkg, cols, rows):
    imgs = _images()
    for cl, rm in CAPS:
        frames = [orc.convert_with_caps(im, cols, rows, cl, rm) for im in imgs]
        g, ref = pkg.Rain(cols, rows), RS.Restated(cols, rows)
        try:
            for step in range(20):
                if step == 6:
                    g.reset(), ref.reset()
                if step == 9:
                    g.set_fall_speed(4.5), g.set_raindrop_length(7.0)
                    ref.r.fall_speed, ref.r.raindrop_length = 4.5, 7.0
                if step == 11:  # direct writes to the struct's fields
                    for o in (g.s, ref.r):
                        o.brightness_decay, o.animation_speed, o.color_r, o.color_g, o.color_b = 0.35, 1.5, 200, 90, 10
                if step == 14:
                    g.set_color_from_filter(12)
                    ref.r.rainbow_mode, ref.r.color_r, ref.r.color_g, ref.r.color_b = True, 255, 0, 0
                if step == 17:
                    g.set_color_from_filter(6)
                    ref.r.rainbow_mode = False
                    ref.r.color_r, ref.r.color_g, ref.r.color_b = g.s.color_r, g.s.color_g, g.s.color_b
                dt = 0.016 + 0.003 * (step % 5)
                f = frames[step % 2]
                _same(g.apply(f, dt), ref.apply(f, dt), f"{cols}x{rows} caps {cl},{rm} step {step}")
                assert g.grid() == ref.state(), f"{cols}x{rows} caps {cl},{rm} step {step}: brightness grid"
                assert (g.s.time, g.s.first_frame, g.s.color_r, g.s.color_g, g.s.color_b) == \
                    (ref.r.time, ref.r.first_frame, ref.r.color_r, ref.r.color_g, ref.r.color_b)
        finally:
            g.close()
            ref.close()


def test_batch_after_plan_render_then_pack_and_packets(pkg):
    import torch
    img = _images()[1]
    dev = torch.from_numpy(img).cuda()
    sizes = [(80, 24), (200, 60)]
    n = 256
    frames = [pkg.frame_setup(dev.data_ptr(), img.shape[1], img.shape[0], *sizes[i % 2], 0, False, False, False) for i in range(n)]
    plan = pkg.Plan(pkg.MODE_TRUE_FG, orc.PALETTE_STANDARD, frames)
    slab = torch.zeros(n * plan.stride, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    plan.render(slab.data_ptr(), plan.stride, ln.data_ptr(), stream)
    # mixed grids: matching, narrower and shorter than the frame, wider than the frame; 32 contexts, 8 frames each
    grids = [(80, 24), (200, 60), (60, 20), (150, 70)]
    ctxs = [(pkg.Rain(*grids[k % 4]), RS.Restated(*grids[k % 4])) for k in range(32)]
    out_stride = pkg.Rain.out_stride(plan.stride, 200 * 60)
    dst = torch.zeros(n * out_stride, dtype=torch.uint8, device="cuda")
    dln = torch.zeros(n, dtype=torch.int32, device="cuda")
    try:
        for rnd in range(8):  # every context once per call: 8 calls of 32 frames each over the 256-frame slab
            sel = list(range(rnd * 32, rnd * 32 + 32))
            dts = [0.02 + 0.001 * i for i in sel]
            rc = pkg.Rain.apply_batch([ctxs[i % 32][0] for i in sel], dts, slab.data_ptr() + sel[0] * plan.stride, plan.stride,
                                      ln.data_ptr() + 4 * sel[0], dst.data_ptr() + sel[0] * out_stride, out_stride,
                                      dln.data_ptr() + 4 * sel[0], stream)
            assert rc == 0, pkg.last_error()
        torch.cuda.synchronize()
        lens = [int(v) & 0xFFFFFFFF for v in ln.cpu().numpy()]
        dlens = [int(v) & 0xFFFFFFFF for v in dln.cpu().numpy()]
        src_host, dst_host = slab.cpu().numpy(), dst.cpu().numpy()
        expected = []
        for i in range(n):
            f = bytes(src_host[i * plan.stride:i * plan.stride + lens[i]])
            exp = ctxs[i % 32][1].apply(f, 0.02 + 0.001 * i)
            got = bytes(dst_host[i * out_stride:i * out_stride + dlens[i]])
            _same(got, exp, f"slab frame {i}")
            expected.append(exp)
        # the output slab feeds pack_frames and frame_packets as it is
        cap = sum((len(e) + 15) // 16 * 16 for e in expected)
        packed = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        pkg.pack_frames(dst.data_ptr(), out_stride, dln.data_ptr(), n, packed.data_ptr(), cap, off.data_ptr(), None, stream)
        dims = torch.tensor([sizes[i % 2] for i in range(n)], dtype=torch.int32, device="cuda")
        crc = torch.zeros(n, dtype=torch.int32, device="cuda")
        hdr = torch.zeros(n * 24, dtype=torch.uint8, device="cuda")
        pkt = torch.zeros(n, dtype=torch.int32, device="cuda")
        rc = pkg.lib().asciichat_hip_frame_packets(dst.data_ptr(), out_stride, dln.data_ptr(), out_stride, n, dims.data_ptr(),
                                                   crc.data_ptr(), hdr.data_ptr(), pkt.data_ptr(), stream)
        assert rc == 0, pkg.last_error()
        torch.cuda.synchronize()
        offs, ph, crcs, hdrs, pkts = off.cpu().numpy(), packed.cpu().numpy(), crc.cpu().numpy(), hdr.cpu().numpy(), pkt.cpu().numpy()
        for i in range(n):
            assert bytes(ph[offs[i]:offs[i] + len(expected[i])]) == expected[i], f"packed frame {i}"
            assert int(crcs[i]) & 0xFFFFFFFF == orc.crc32c(expected[i]), f"crc {i}"
            h, pc = orc.ascii_frame_packet(expected[i], *sizes[i % 2])
            assert bytes(hdrs[24 * i:24 * i + 24]) == h and int(pkts[i]) & 0xFFFFFFFF == pc, f"packet {i}"
        for g, ref in ctxs:  # the grids the batches left, read through one more drop-in step
            f = orc.convert_with_caps(img, g.s.num_columns, g.s.num_rows, 3, 0)
            _same(g.apply(f, 0.01), ref.apply(f, 0.01), "after the batches")
            assert g.grid() == ref.state()
    finally:
        for g, ref in ctxs:
            g.close()
            ref.close()
        plan.close()


def test_batch_refuses_duplicate_context_and_overflows_cleanly(pkg):
    import torch
    f = orc.convert_with_caps(_images()[0], 80, 24, 3, 0)
    stride = (len(f) + 15) // 16 * 16
    src = torch.zeros(2 * stride, dtype=torch.uint8, device="cuda")
    src[:len(f)] = torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda()
    src[stride:stride + len(f)] = src[:len(f)]
    ln = torch.tensor([len(f), len(f)], dtype=torch.int32, device="cuda")
    g, ref = pkg.Rain(80, 24), RS.Restated(80, 24)
    try:
        _same(g.apply(f, 0.03), ref.apply(f, 0.03), "warm-up")
        t0 = g.s.time
        out_stride = pkg.Rain.out_stride(stride, 80 * 24)
        dst = torch.zeros(2 * out_stride, dtype=torch.uint8, device="cuda")
        dln = torch.zeros(2, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        rc = pkg.Rain.apply_batch([g, g], [0.01, 0.01], src.data_ptr(), stride, ln.data_ptr(), dst.data_ptr(), out_stride,
                                  dln.data_ptr(), stream)
        assert rc != 0 and g.s.time == t0, "a context twice in one call is refused before anything advances"
        small = (len(f) + 127) // 128 * 128  # room for the input, not for the injected colours
        rc = pkg.Rain.apply_batch([g], [0.01], src.data_ptr(), stride, ln.data_ptr(), dst.data_ptr(), small, dln.data_ptr(),
                                  stream)
        assert rc == 0, pkg.last_error()
        torch.cuda.synchronize()
        assert int(dln[0].item()) & 0xFFFFFFFF == RS.LEN_OVERFLOW
        # the host side advanced at issue time; the grid did not move: the next step matches a restatement that skipped it
        ref.r.time = float(np.float32(np.float32(ref.r.time) + np.float32(np.float32(0.01) * np.float32(ref.r.animation_speed))))
        ref.r.first_frame = False
        assert g.s.time == ref.r.time
        _same(g.apply(f, 0.02), ref.apply(f, 0.02), "after the overflow")
        assert g.grid() == ref.state()
    finally:
        g.close()
        ref.close()
