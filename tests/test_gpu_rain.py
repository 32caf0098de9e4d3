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


# ---- boundaries, parameter extremes and the host paths of rain.c (rain_cases.py; compared under its rule) ----
import rain_cases as RC  # noqa: E402


def _round16(n):
    return (n + 15) // 16 * 16


def _product(pkg, cols, rows):
    g = pkg.Rain(cols, rows)
    g.set_field = lambda name, v, s=g.s: setattr(s, name, v)
    g.cells = cols * rows  # as allocated
    return g


def _slab(frames, stride=None):
    """frames side by side on the device: (tensor, stride, lengths tensor)"""
    import torch
    stride = stride or max(16, _round16(max(len(f) for f in frames)))
    host = np.zeros(len(frames) * stride, dtype=np.uint8)
    for i, f in enumerate(frames):
        host[i * stride:i * stride + len(f)] = np.frombuffer(f, dtype=np.uint8)
    return torch.from_numpy(host).cuda(), stride, torch.tensor([len(f) for f in frames], dtype=torch.int32, device="cuda")


def _outputs(dst, dln, stride, n):
    """the n frames of an output slab, on the host (LEN_OVERFLOW and error codes as numbers)"""
    lens = [int(v) & 0xFFFFFFFF for v in dln.cpu().numpy()[:n]]
    host = dst.cpu().numpy()
    return [ln if ln >= 0xFFFFFFF0 else bytes(host[i * stride:i * stride + ln]) for i, ln in enumerate(lens)]


def _device_grids(pkg, ctxs, stream):
    """the grids, as allocated, that the batches left on the device (asciichat_hip_rain_state_dev), copied out by the pack
    kernel on the stream the batches went to"""
    import torch
    sizes = [4 * g.cells for g in ctxs]
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + _round16(s))
    dst = torch.zeros(offs[-1], dtype=torch.uint8, device="cuda")
    lens = torch.tensor(sizes, dtype=torch.int32, device="cuda")
    off = torch.zeros(2, dtype=torch.int64, device="cuda")
    for i, g in enumerate(ctxs):
        ptr = g.state_dev()
        assert ptr, pkg.last_error()
        pkg.pack_frames(ptr, _round16(sizes[i]), lens.data_ptr() + 4 * i, 1, dst.data_ptr() + offs[i], _round16(sizes[i]),
                        off.data_ptr(), None, stream)
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    return [host[offs[i]:offs[i] + sizes[i]].view(np.float32) for i in range(len(ctxs))]


def _check_grid(got, ref, what, cols):
    want = np.ctypeslib.as_array(ref.r.previous_brightness, shape=(ref.cols * ref.rows,))
    a, b = np.asarray(got, dtype=np.float32).view(np.uint32), want.view(np.uint32)
    if a.shape != b.shape or not ((a == b) | (np.isnan(got) & np.isnan(want))).all():
        RC.check_grid(got, want, what, cols)  # names the cell


def _run_cases_on_device(pkg, cs, per_call=256):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    for lo in range(0, len(cs), per_call):
        group = cs[lo:lo + per_call]
        pairs = [(_product(pkg, c.cols, c.rows), RS.Restated(c.cols, c.rows)) for c in group]
        try:
            for (g, r), c in zip(pairs, group):
                RC.apply_case_ops(g, c.ops)
                RC.apply_case_ops(r, c.ops)
            for k in range(max(len(c.frames) for c in group)):
                live = [(p, c) for p, c in zip(pairs, group) if k < len(c.frames)]
                src, stride, ln = _slab([c.frames[k] for _, c in live])
                out_stride = pkg.Rain.out_stride(stride, stride)  # (no more events than bytes)
                dst = torch.zeros(len(live) * out_stride, dtype=torch.uint8, device="cuda")
                dln = torch.zeros(len(live), dtype=torch.int32, device="cuda")
                rc = pkg.Rain.apply_batch([g for (g, _), _ in live], [c.dts[k] for _, c in live], src.data_ptr(), stride,
                                          ln.data_ptr(), dst.data_ptr(), out_stride, dln.data_ptr(), stream)
                assert rc == 0, pkg.last_error()
                grids = _device_grids(pkg, [g for (g, _), _ in live], stream)
                got = _outputs(dst, dln, out_stride, len(live))
                for ((g, r), c), o, grid in zip(live, got, grids):
                    what = f"{c.name} step {k}"
                    assert not isinstance(o, int), f"{what}: length code 0x{o:08x}"
                    RC.check_output(o, r.apply(c.frames[k], c.dts[k]), what)
                    _check_grid(grid, r, what + ": grid", c.cols)
        finally:
            for g, r in pairs:
                g.close()
                r.close()


def test_parameter_extremes_on_the_device(pkg):
    """OCML's sin, the device's division, floorf, denormals and NaNs against glibc and SSE: bytes and bits, no tolerance"""
    _run_cases_on_device(pkg, RC.parameter_cases())


def test_boundary_cases_on_the_device(pkg):
    _run_cases_on_device(pkg, RC.boundary_cases())


def test_dropin_matches_edges_fixture(pkg):
    import hashlib
    fx = json.load(open(RS.GOLDEN_EDGES))
    for case in fx["cases"]:
        g = _product(pkg, case["cols"], case["rows"])
        try:
            for k, step in enumerate(case["steps"]):
                RC.apply_case_ops(g, step.get("ops", []))
                out = g.apply(RC.unpack_frame(step["input_parts"]), step["dt"])
                assert (len(out), hashlib.sha256(out).hexdigest()) == (step["out_len"], step["sha256"]), f"{case['name']} step {k}"
            assert hashlib.sha256(RC.canonical_grid_bytes(g.grid())).hexdigest() == case["final_grid_sha256"], case["name"]
        finally:
            g.close()


def _small_frame(i, step):
    E = RC.E
    parts = [b"abcdefgh\nij", E + b"[38;2;%d;%d;9mxy" % (i % 256, (7 * i + step) % 256), "█é".encode() + b"\n\nq",
             E + b"[48;2;1;2;3m" + E + b"[38;2;200;100;50mQ", b"z" * (i % 9) + b"\n", E + b"[5bk" + E]
    return parts[i % 6] + parts[(i // 6 + step) % 6] + parts[(i + 2 * step) % 6]


def test_batch_longer_than_a_ring_segment(pkg):
    """2 200 frames in one call: three launches from three ring segments"""
    import torch
    n = 2200
    stream = torch.cuda.current_stream().cuda_stream
    pairs = [(_product(pkg, 8, 3), RS.Restated(8, 3)) for _ in range(n)]
    try:
        for step in range(2):
            frames = [_small_frame(i, step) for i in range(n)]
            dts = [0.01 + 0.0001 * (i % 97) for i in range(n)]
            src, stride, ln = _slab(frames)
            out_stride = pkg.Rain.out_stride(stride, stride)
            dst = torch.zeros(n * out_stride, dtype=torch.uint8, device="cuda")
            dln = torch.zeros(n, dtype=torch.int32, device="cuda")
            rc = pkg.Rain.apply_batch([g for g, _ in pairs], dts, src.data_ptr(), stride, ln.data_ptr(), dst.data_ptr(), out_stride,
                                      dln.data_ptr(), stream)
            assert rc == 0, pkg.last_error()
            grids = _device_grids(pkg, [g for g, _ in pairs], stream)
            for i, ((g, r), o) in enumerate(zip(pairs, _outputs(dst, dln, out_stride, n))):
                RC.check_output(o, r.apply(frames[i], dts[i]), f"step {step} frame {i}")
                _check_grid(grids[i], r, f"step {step} frame {i}: grid", 8)
    finally:
        for g, r in pairs:
            g.close()
            r.close()


def _issue_rounds(pkg, pairs, rounds, streams, grid):
    """`rounds` batch calls over the same contexts with no host wait between them, call j on streams[j % len(streams)];
    each call has its own input and output slab, all inputs on the device before the first call.  Returns what to check
    after the caller's synchronise: [(dst, dln, out_stride, frames, dts)]."""
    import torch
    n = len(pairs)
    calls = []
    for j in range(rounds):
        frames = [_small_frame(i + 5 * j, j) * (1 + (i + j) % 3) for i in range(n)]
        src, stride, ln = _slab(frames)
        out_stride = pkg.Rain.out_stride(stride, stride)
        calls.append((src, stride, ln, torch.zeros(n * out_stride, dtype=torch.uint8, device="cuda"),
                      torch.zeros(n, dtype=torch.int32, device="cuda"), out_stride, frames, [0.01 + 0.002 * ((i + j) % 5) for i in range(n)]))
    torch.cuda.synchronize()  # every slab is written before any stream starts: the calls order the contexts, not these
    for j, (src, stride, ln, dst, dln, out_stride, frames, dts) in enumerate(calls):
        rc = pkg.Rain.apply_batch([g for g, _ in pairs], dts, src.data_ptr(), stride, ln.data_ptr(), dst.data_ptr(), out_stride,
                                  dln.data_ptr(), streams[j % len(streams)])
        assert rc == 0, pkg.last_error()
    return calls


def _check_rounds(pairs, calls, what):
    for j, (src, stride, ln, dst, dln, out_stride, frames, dts) in enumerate(calls):
        for i, ((g, r), o) in enumerate(zip(pairs, _outputs(dst, dln, out_stride, len(pairs)))):
            RC.check_output(o, r.apply(frames[i], dts[i]), f"{what}: call {j} frame {i}")


def test_forty_calls_without_a_host_wait_wrap_the_ring(pkg):
    """16 ring segments, 40 calls over the same 32 contexts: the ring wraps twice and every call blends with the one before"""
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    pairs = [(_product(pkg, 12, 5), RS.Restated(12, 5)) for _ in range(32)]
    try:
        calls = _issue_rounds(pkg, pairs, 40, [stream], (12, 5))
        torch.cuda.synchronize()
        _check_rounds(pairs, calls, "one stream")
        for i, grid in enumerate(_device_grids(pkg, [g for g, _ in pairs], stream)):
            _check_grid(grid, pairs[i][1], f"context {i}: grid after 40 calls", 12)
    finally:
        for g, r in pairs:
            g.close()
            r.close()


def test_two_streams_in_turn_then_the_dropin_without_a_host_wait(pkg):
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    pairs = [(_product(pkg, 12, 5), RS.Restated(12, 5)) for _ in range(32)]
    try:
        calls = _issue_rounds(pkg, pairs, 12, [s1.cuda_stream, s2.cuda_stream], (12, 5))
        # the drop-in directly behind batch calls that are still in flight: its own stream waits for the context's last launch
        f = RC.PARAM_FRAME
        outs = [g.apply(f, 0.02) for g, _ in pairs]
        torch.cuda.synchronize()
        _check_rounds(pairs, calls, "two streams")
        for i, (g, r) in enumerate(pairs):
            RC.check_output(outs[i], r.apply(f, 0.02), f"context {i}: drop-in behind the batches")
            _check_grid(np.array(g.grid(), dtype=np.float32), r, f"context {i}: grid after the drop-in", 12)
    finally:
        for g, r in pairs:
            g.close()
            r.close()


def test_dropin_staging_grows_and_is_reused(pkg):
    g, r = _product(pkg, 40, 12), RS.Restated(40, 12)
    small = RC.E + b"[38;2;1;2;3mab\ncd" + RC.E + b"[48;2;9;9;m"
    line = RC.E + b"[38;2;200;100;50m" + b"abcdefghijklmnopqrstuvwxyz0123456789#@%&" + RC.E + b"[48;2;5;6;7m+\n"
    big = line * (200 * 1024 // len(line) + 1)
    assert len(small) == 30 and len(big) >= 200 * 1024
    try:
        for k, (f, dt) in enumerate(((small, 0.02), (big, 0.03), (small, 0.04), (big, 0.01))):
            RC.check_output(g.apply(f, dt), r.apply(f, dt), f"step {k} ({len(f)} bytes)")
            _check_grid(np.array(g.grid(), dtype=np.float32), r, f"step {k}: grid", 40)
    finally:
        g.close()
        r.close()


def test_grid_written_smaller_than_allocated_and_back_on_the_device(pkg):
    """the sequence of test_rain_boundaries.py through the product's context: batch calls, the overflow step in a slot too
    small, the grid as allocated read from the device after every step, and the drop-in at the end"""
    import torch
    SHRUNK_FRAME, SHRUNK_STEPS = RC.SHRUNK_FRAME, RC.SHRUNK_STEPS
    stream = torch.cuda.current_stream().cuda_stream
    g, r = _product(pkg, 12, 6), RS.Restated(12, 6)
    src, stride, ln = _slab([SHRUNK_FRAME])
    out_stride = pkg.Rain.out_stride(stride, stride)
    dst = torch.zeros(out_stride, dtype=torch.uint8, device="cuda")
    dln = torch.zeros(1, dtype=torch.int32, device="cuda")
    try:
        for k, (cols, rows, dt, overflow) in enumerate(SHRUNK_STEPS):
            if cols:
                for o in (g.s, r.r):
                    o.num_columns, o.num_rows = cols, rows
            rc = pkg.Rain.apply_batch([g], [dt], src.data_ptr(), stride, ln.data_ptr(), dst.data_ptr(), 256 if overflow else out_stride,
                                      dln.data_ptr(), stream)
            assert rc == 0, pkg.last_error()
            grid = _device_grids(pkg, [g], stream)[0]
            got = _outputs(dst, dln, out_stride, 1)[0]
            if overflow:
                assert got == RS.LEN_OVERFLOW
                r.r.time = g.s.time
            else:
                RC.check_output(got, r.apply(SHRUNK_FRAME, dt), f"step {k}")
            _check_grid(grid, r, f"step {k}: the grid as allocated", None)
        RC.check_output(g.apply(SHRUNK_FRAME, 0.02), r.apply(SHRUNK_FRAME, 0.02), "drop-in at the end")
        _check_grid(np.array(g.grid(), dtype=np.float32), r, "drop-in at the end: grid", 12)
    finally:
        g.close()
        r.close()
