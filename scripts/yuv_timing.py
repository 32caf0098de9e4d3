#!/usr/bin/env python3
"""Times libasciichat_yuv.so on one GPU, all in one run: (1) the sampled pass (Yuv.run) for 256 1080p sources -> 80x24 and
16 -> 200x60, NV12 and I420, beside Plan.render of the same descriptors over RGB24 sources -- the capability without the
library --, and the tick set + run + Plan.render end to end; (2) Yuv.run_whole for 256 x 1080p per format as bytes moved (planes
read + RGB written) over time, beside a device-to-device hipMemcpyAsync of the same output bytes.  HIP events around every
launch, the stages alternating; medians over --launches after --warmup; the tick also on the host clock around a synchronise.
The RGB sources are run_whole's own output, and the text rendered from the sampled images is asserted equal to the text
rendered from them at the timed sizes.  Writes the figures to --out.  No time is a pass criterion."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from raster_timing import hip_runtime  # noqa: E402

W, H = 1920, 1080
SHAPES = ((256, 80, 24), (16, 200, 60))
DISTINCT = 8  # different contents; every source has device memory of its own


def events():
    import torch
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fns, launches, warmup):
    """{name: [us]} of the stages, alternating, one pair of events around each call"""
    import torch
    times = {k: [] for k in fns}
    for it in range(warmup + launches):
        evs = []
        for name, fn in fns.items():
            a, b = events()
            a.record()
            fn()
            b.record()
            evs.append((name, a, b))
        torch.cuda.synchronize()
        if it >= warmup:
            for name, a, b in evs:
                times[name].append(a.elapsed_time(b) * 1000.0)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_timing.txt"))
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=256, help="sources of the large batch (a rehearsal may take fewer)")
    args = ap.parse_args()
    import torch

    import orc
    import yuv_ref as YR
    from __graft_entry__ import load_package

    pkg = load_package()
    if not torch.cuda.is_available() or pkg.yuv_lib().asciichat_yuv_device_count() <= 0:
        raise SystemExit("yuv_timing: needs a GPU")
    hip = hip_runtime()
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream
    N = args.frames
    lines = ["# YUV sources: scripts/yuv_timing.py (HIP events around every launch, the stages alternating; medians of "
             f"{args.launches} launches after {args.warmup} warm-ups; {torch.cuda.get_device_name(0)})"]

    # the sources: DISTINCT contents per format, N device copies each
    rng = np.random.default_rng(7)
    base = orc.frame_smooth(W, H).astype(np.int32)
    slabs, sources = {}, {}
    for fmt in (YR.NV12, YR.I420, YR.YUYV, YR.UYVY):
        cshape = (H, W // 2) if fmt in YR.PACKED else YR.chroma_size(W, H)[::-1]
        host = []
        for k in range(DISTINCT):
            Y = np.clip(base[:, :, k % 3] + rng.integers(-20, 21, (H, W)), 0, 255).astype(np.uint8)
            planes, strides = YR.pack(fmt, Y, rng.integers(0, 256, cshape, dtype=np.uint8), rng.integers(0, 256, cshape, dtype=np.uint8))
            host.append(np.concatenate(planes))
        per = host[0].size
        assert per % 16 == 0
        slab = torch.from_numpy(np.stack(host)).cuda()[torch.arange(N, device="cuda") % DISTINCT].contiguous()
        at = np.cumsum([0] + [p.size for p in planes])
        slabs[fmt] = slab
        sources[fmt] = [pkg.yuv_source(fmt, W, H, [slab.data_ptr() + i * per + int(a) for a in at[:-1]]) for i in range(N)]
    plane_bytes = {fmt: slabs[fmt].shape[1] for fmt in slabs}

    # (2) first: run_whole also makes the RGB sources of (1)
    rgb = torch.empty(N * 3 * W * H, dtype=torch.uint8, device="cuda")
    copy = torch.empty_like(rgb)
    y = pkg.Yuv(N)
    lines.append(f"run_whole: {N} sources of {W}x{H} -> RGB24 ({rgb.numel() / 1e6:.0f} MB written per launch)")
    for fmt in (YR.NV12, YR.I420, YR.YUYV, YR.UYVY):
        y.set(sources[fmt], None, stream=stream)

        def whole():
            y.run_whole(rgb.data_ptr(), 3 * W * H, stream=stream)

        def memcpy():
            rc = hip.hipMemcpyAsync(copy.data_ptr(), rgb.data_ptr(), rgb.numel(), 3, stream)
            if rc != 0:
                raise RuntimeError(f"hipMemcpyAsync failed ({rc})")

        whole()
        torch.cuda.synchronize()
        probe = rgb[:3 * W * H].cpu().numpy().reshape(H, W, 3)
        per = plane_bytes[fmt]
        first = slabs[fmt][0].cpu().numpy()
        st = [YR.row_bytes(fmt, k, W) for k in range(YR.planes_of(fmt))]
        offs = np.cumsum([0] + [YR.plane_rows(fmt, k, H) * st[k] for k in range(len(st))])
        ref = YR.Source(fmt, W, H, [first[int(o):] for o in offs[:-1]], st)
        assert np.array_equal(probe, YR.convert_whole(ref)), "run_whole differs from the restatement at the timed size"
        t = timed(dict(run_whole=whole, memcpy=memcpy), max(10, args.launches // 5), args.warmup)
        med = {k: statistics.median(v) for k, v in t.items()}
        moved = N * per + rgb.numel()
        lines.append(f"  {YR.NAMES[fmt]:<5} run_whole median {med['run_whole']:9.1f} us  least {min(t['run_whole']):9.1f} us  "
                     f"{moved / 1e6:.0f} MB moved -> {moved / med['run_whole'] / 1e6:.2f} TB/s     memcpy D2D of the output bytes median "
                     f"{med['memcpy']:9.1f} us  ({2 * rgb.numel() / med['memcpy'] / 1e6:.2f} TB/s read + written)")
    y.set(sources[YR.NV12], None, stream=stream)
    y.run_whole(rgb.data_ptr(), 3 * W * H, stream=stream)  # the RGB twins of the NV12 sources
    rgb_i420 = None
    torch.cuda.synchronize()
    y.close()
    del copy

    # (1) the sampled pass beside the render from RGB
    for n, cols, rows in SHAPES:
        n = min(n, N)
        for fmt in (YR.NV12, YR.I420):
            if fmt == YR.I420:  # RGB twins of the first n I420 sources
                yw = pkg.Yuv(n)
                yw.set(sources[fmt][:n], None, stream=stream)
                rgb_i420 = torch.empty(n * 3 * W * H, dtype=torch.uint8, device="cuda")
                yw.run_whole(rgb_i420.data_ptr(), 3 * W * H, stream=stream)
                torch.cuda.synchronize()
                yw.close()
            twins = rgb if fmt == YR.NV12 else rgb_i420
            frames = [pkg.frame_setup(twins.data_ptr() + i * 3 * W * H, W, H, cols, rows, 0, False, False, False) for i in range(n)]
            plan_rgb = pkg.Plan(pkg.MODE_TRUE_FG, orc.PALETTE_STANDARD, frames)
            ys = pkg.Yuv(n)
            src_arr, frame_arr = (pkg.YuvSource * n)(*sources[fmt][:n]), (pkg.Frame * n)(*frames)  # as a C caller holds them
            ys.set(src_arr, frame_arr, stream=stream)
            images = torch.empty(n * ys.pitch, dtype=torch.uint8, device="cuda")
            plan_img = pkg.Plan(pkg.MODE_TRUE_FG, orc.PALETTE_STANDARD, ys.render_frames(images.data_ptr()))
            stride = max(plan_rgb.stride, plan_img.stride)
            text = [torch.zeros(n * stride, dtype=torch.uint8, device="cuda") for _ in range(2)]
            lens = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]

            def render_rgb():
                plan_rgb.render(text[0].data_ptr(), stride, lens[0].data_ptr(), stream)

            def run():
                ys.run(images.data_ptr(), stream=stream)

            def render_images():
                plan_img.render(text[1].data_ptr(), stride, lens[1].data_ptr(), stream)

            def tick():
                ys.set(src_arr, frame_arr, stream=stream)
                ys.run(images.data_ptr(), stream=stream)
                plan_img.render(text[1].data_ptr(), stride, lens[1].data_ptr(), stream)

            render_rgb()
            tick()
            torch.cuda.synchronize()
            la, lb = lens[0].cpu().numpy(), lens[1].cpu().numpy()
            ta, tb = text[0].cpu().numpy().reshape(n, stride), text[1].cpu().numpy().reshape(n, stride)
            assert np.array_equal(la, lb) and all(np.array_equal(ta[i, :la[i]], tb[i, :la[i]]) for i in range(n)), "the two paths' text differs"
            t = timed(dict(render_from_rgb=render_rgb, yuv_run=run, render_from_images=render_images, tick_set_run_render=tick),
                      args.launches, args.warmup)
            wall = []
            for it in range(args.warmup + args.launches):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tick()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    wall.append((time.perf_counter() - t0) * 1e6)
            lines.append(f"{n} {YR.NAMES[fmt]} sources of {W}x{H} -> {cols}x{rows} (truecolor foreground; {int(la.astype(np.int64).sum()) / 1e6:.2f} MB of text, "
                         f"{n * 3 * cols * rows / 1e3:.0f} KB of sampled images; both paths' text equal)")
            for k, v in t.items():
                lines.append(f"  {k:<22} median {statistics.median(v):9.1f} us   least {min(v):9.1f} us")
            lines.append(f"  {'tick, host clock':<22} median {statistics.median(wall):9.1f} us   least {min(wall):9.1f} us   (enqueue to synchronise)")
            ys.close()
            plan_rgb.close()
            plan_img.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
