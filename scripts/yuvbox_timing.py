#!/usr/bin/env python3
"""Times libasciichat_yuvbox.so on one GPU, all in one run: YuvBox.run (YUV sources box-averaged straight from their planes)
beside the route it replaces -- Yuv.run_whole into a slab of whole RGB24 frames, then Box.run over that slab -- for 256 NV12 and
256 YUYV 1080p sources -> 80x24 and 16 of each -> 200x60, and beside a device-to-device hipMemcpyAsync of the sources' bytes as
the traffic's own floor.  HIP events around every stage, the two ways alternating; medians over --launches after --warmup.  The
images of the two ways are asserted equal before anything is printed.  Writes the figures to --out, the bytes of the
intermediate slab the route needs among them, and says for each 256-source workload whether the pass's median stayed at or below
the route's."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from raster_timing import hip_runtime  # noqa: E402
from yuv_timing import timed  # noqa: E402

W, H = 1920, 1080
SHAPES = ((256, 80, 24), (16, 200, 60))
DISTINCT = 8  # different contents; every source has device memory of its own


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuvbox_timing.txt"))
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=256, help="sources of the large batch (a rehearsal may take fewer)")
    args = ap.parse_args()
    import torch

    import orc
    import yuv_ref as YR
    from __graft_entry__ import load_package

    pkg = load_package()
    if not torch.cuda.is_available() or pkg.yuvbox_lib().asciichat_yuvbox_device_count() <= 0:
        raise SystemExit("yuvbox_timing: needs a GPU")
    hip = hip_runtime()
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream
    N = args.frames
    lines = ["# YUV sources box-averaged from their planes: scripts/yuvbox_timing.py (HIP events around every stage, the two ways "
             f"alternating; medians of {args.launches} launches after {args.warmup} warm-ups; {torch.cuda.get_device_name(0)})"]

    rng = np.random.default_rng(11)
    base = orc.frame_smooth(W, H).astype(np.int32)
    verdicts = []
    for fmt in (YR.NV12, YR.YUYV):
        # the sources: DISTINCT contents, N device copies
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
        sources = [pkg.yuv_source(fmt, W, H, [slab.data_ptr() + i * per + int(a) for a in at[:-1]]) for i in range(N)]
        floor_dst = torch.empty_like(slab)
        for count, cols, rows in SHAPES:
            n = min(count, N)
            whole = torch.empty(n * 3 * W * H, dtype=torch.uint8, device="cuda")  # the slab only the route needs
            frames = [pkg.frame_setup(whole.data_ptr() + i * 3 * W * H, W, H, cols, rows, 0, False, False, False) for i in range(n)]
            assert all(f is not None and (f.out_w, f.out_h) == (cols, rows) for f in frames)
            y = pkg.Yuv(n)
            y.set(sources[:n], None, stream=stream)
            box = pkg.Box(frames)
            fused = pkg.YuvBox(n)
            fused.set(sources[:n], frames, stream=stream)
            assert fused.pitch == box.pitch
            images = [torch.full((n * box.pitch,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
            moved = n * per

            def run_whole():
                y.run_whole(whole.data_ptr(), 3 * W * H, stream=stream)

            def box_run():
                box.run(images[0].data_ptr(), stream=stream)

            def route():
                run_whole()
                box_run()

            def yuvbox_run():
                fused.run(images[1].data_ptr(), stream=stream)

            def memcpy():
                rc = hip.hipMemcpyAsync(floor_dst.data_ptr(), slab.data_ptr(), moved, 3, stream)
                if rc != 0:
                    raise RuntimeError(f"hipMemcpyAsync failed ({rc})")

            route()
            yuvbox_run()
            torch.cuda.synchronize()
            assert torch.equal(images[0], images[1]), "the two ways' images differ"
            assert int((images[1] != 0xA5).sum().item()) > n * 3 * cols * rows // 2, "nothing was stored"
            t = timed({"yuv_run_whole": run_whole, "box_run": box_run, "route: run_whole + box_run": route, "yuvbox_run": yuvbox_run,
                       "memcpy D2D of the sources": memcpy}, args.launches, args.warmup)
            med = {k: statistics.median(v) for k, v in t.items()}
            lines.append(f"{n} {YR.NAMES[fmt]} sources of {W}x{H} -> {cols}x{rows} ({moved / 1e6:.0f} MB of samples, {n * 3 * cols * rows / 1e3:.0f} KB of images; "
                         f"the two ways' images equal; the route's slab of whole frames: {whole.numel() / 1e6:.0f} MB, the pass needs none)")
            for k, v in t.items():
                note = ""
                if k == "yuvbox_run":
                    note = f"   {moved / med[k] / 1e6:.2f} TB/s of samples read, {med['route: run_whole + box_run'] / med[k]:.2f} x the route's rate"
                if k.startswith("memcpy"):
                    note = f"   {moved / med[k] / 1e6:.2f} TB/s read (and as much written)"
                lines.append(f"  {k:<28} median {med[k]:9.1f} us   least {min(v):9.1f} us{note}")
            if count == SHAPES[0][0]:
                ok = med["yuvbox_run"] <= med["route: run_whole + box_run"]
                verdicts.append(f"{n} {YR.NAMES[fmt]} -> {cols}x{rows}: yuvbox_run {med['yuvbox_run']:.1f} us "
                                f"{'<=' if ok else '> (CONDITION MISSED)'} route {med['route: run_whole + box_run']:.1f} us")
            y.close()
            box.close()
            fused.close()
            del whole, images
        del slab, floor_dst
    lines.append("condition (the pass's median does not exceed the route's, no margin): " + "; ".join(verdicts))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
