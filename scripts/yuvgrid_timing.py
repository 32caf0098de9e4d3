#!/usr/bin/env python3
"""Times libasciichat_yuvgrid.so on one GPU, all in one run: nine NV12 1080p sources as the tiles of the grid composites at 80x24,
160x48 and 200x60 in ONE set (27 tiles), 256 truecolor-foreground targets per size.  The two ways to the same text, alternating:
the tile way -- YuvGrid.run, then the three Plan.render over the rewritten descriptors --, and the only way there was before --
asciichat_yuv_run_whole of the nine sources, then the three Plan.render over the original descriptors, whose sources are the whole
RGB24 frames.  HIP events around every stage; medians over --launches after --warmup; the tick (set + run + renders) also on the
host clock around a synchronise.  The text of the two ways is asserted equal at the timed sizes.  Writes the figures to --out.
No time is a pass criterion."""
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

from yuv_timing import timed  # noqa: E402

W, H = 1920, 1080
SIZES = ((80, 24), (160, 48), (200, 60))
SOURCES = 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuvgrid_timing.txt"))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--targets", type=int, default=256, help="targets per size (a rehearsal may take fewer)")
    args = ap.parse_args()
    import torch

    import orc
    import yuv_ref as YR
    from __graft_entry__ import load_package

    pkg = load_package()
    if not torch.cuda.is_available() or pkg.yuvgrid_lib().asciichat_yuvgrid_device_count() <= 0:
        raise SystemExit("yuvgrid_timing: needs a GPU")
    L = pkg.lib()
    stream = torch.cuda.current_stream().cuda_stream
    N = args.targets
    lines = ["# YUV sources as grid tiles: scripts/yuvgrid_timing.py (HIP events around every stage, the two ways alternating; medians of "
             f"{args.launches} launches after {args.warmup} warm-ups; {torch.cuda.get_device_name(0)})"]

    # nine NV12 sources of their own contents and device memory
    rng = np.random.default_rng(11)
    base = orc.frame_smooth(W, H).astype(np.int32)
    cshape = YR.chroma_size(W, H)[::-1]
    planes_dev, sources = [], []
    for k in range(SOURCES):
        Y = np.clip(base[:, :, k % 3] + rng.integers(-20, 21, (H, W)), 0, 255).astype(np.uint8)
        planes, _ = YR.pack(YR.NV12, Y, rng.integers(0, 256, cshape, dtype=np.uint8), rng.integers(0, 256, cshape, dtype=np.uint8))
        t = torch.from_numpy(np.concatenate(planes)).cuda()
        planes_dev.append(t)
        sources.append(pkg.yuv_source(YR.NV12, W, H, [t.data_ptr(), t.data_ptr() + planes[0].size]))

    # the old way's whole frames
    whole = pkg.Yuv(SOURCES)
    whole.set(sources, None, stream=stream)
    pitch = whole.whole_pitch
    rgb = torch.empty(SOURCES * pitch, dtype=torch.uint8, device="cuda")

    # the three composites over the whole frames, as achip_composite_setup makes them
    comps = []
    for tw, th in SIZES:
        c = pkg.Composite()
        ptrs = (C.c_void_p * SOURCES)(*[rgb.data_ptr() + i * pitch for i in range(SOURCES)])
        L.achip_composite_setup(C.byref(c), ptrs, (C.c_int * SOURCES)(*[W] * SOURCES), (C.c_int * SOURCES)(*[H] * SOURCES), SOURCES, tw, th)
        assert c.n_src == SOURCES and all(c.s[k].src for k in range(SOURCES))
        comps.append(c)
    grid = pkg.YuvGrid(len(SIZES) * SOURCES)
    per_comp = [sources] * len(SIZES)
    grid.set(comps, per_comp, stream=stream)
    tiles = torch.empty(grid.tiles_bytes(), dtype=torch.uint8, device="cuda")
    rewritten = grid.composites(tiles.data_ptr())

    def upload(c):
        d = C.c_void_p()
        if L.asciichat_hip_composite_upload(C.byref(c), C.byref(d)) != 0:
            raise RuntimeError("composite_upload failed: " + pkg.last_error())
        return d

    ways = {}
    for name, descs in (("tiles", rewritten), ("whole", comps)):
        devs = [upload(c) for c in descs]
        plans = []
        for (tw, th), d in zip(SIZES, devs):
            f = pkg.frame_setup(None, tw, 2 * th, tw, th, 0, True, True, False)
            f.comp = d.value
            plans.append(pkg.Plan(pkg.MODE_TRUE_FG, orc.PALETTE_STANDARD, [f] * N))
        text = [torch.zeros(N * p.stride, dtype=torch.uint8, device="cuda") for p in plans]
        lens = [torch.zeros(N, dtype=torch.int32, device="cuda") for _ in plans]
        ways[name] = (devs, plans, text, lens)

    def renders(name):
        _, plans, text, lens = ways[name]
        for p, t, n in zip(plans, text, lens):
            p.render(t.data_ptr(), p.stride, n.data_ptr(), stream)

    def run_tiles():
        grid.run(tiles.data_ptr(), stream=stream)

    def run_whole():
        whole.run_whole(rgb.data_ptr(), pitch, stream=stream)

    def tick_tiles():
        grid.set(comps, per_comp, stream=stream)
        run_tiles()
        renders("tiles")

    def tick_whole():
        whole.set(sources, None, stream=stream)
        run_whole()
        renders("whole")

    tick_tiles()
    tick_whole()
    torch.cuda.synchronize()
    text_bytes = 0
    for i, size in enumerate(SIZES):
        la, lb = ways["tiles"][3][i].cpu().numpy(), ways["whole"][3][i].cpu().numpy()
        stride = ways["tiles"][1][i].stride
        assert stride == ways["whole"][1][i].stride
        ta, tb = ways["tiles"][2][i].cpu().numpy().reshape(N, stride), ways["whole"][2][i].cpu().numpy().reshape(N, stride)
        assert np.array_equal(la, lb) and la.min() > size[0] * size[1], f"{size}: the two ways' lengths differ"
        assert all(np.array_equal(ta[k, :la[k]], tb[k, :la[k]]) for k in range(N)), f"{size}: the two ways' text differs"
        text_bytes += int(la.astype(np.int64).sum())

    t = timed({"tile launch (27 tiles)": run_tiles, "renders over the tiles": lambda: renders("tiles"),
               "run_whole (9 x 1080p)": run_whole, "renders over whole frames": lambda: renders("whole")}, args.launches, args.warmup)
    t.update(timed({"tick: set + tiles + renders": tick_tiles, "tick: set + run_whole + renders": tick_whole}, args.launches, args.warmup))
    wall = {"tiles": [], "whole": []}
    for it in range(args.warmup + args.launches):
        for name, fn in (("tiles", tick_tiles), ("whole", tick_whole)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= args.warmup:
                wall[name].append((time.perf_counter() - t0) * 1e6)
    tile_px = sum(c.s[k].tile_w * c.s[k].tile_h for c in comps for k in range(SOURCES))
    lines.append(f"{SOURCES} NV12 sources of {W}x{H}; composites at {', '.join('%dx%d' % s for s in SIZES)} in one set: {len(SIZES) * SOURCES} tiles, "
                 f"{3 * tile_px / 1e3:.0f} KB of tiles in a slab of {tiles.numel() / 1e3:.0f} KB against {SOURCES * 3 * W * H / 1e6:.0f} MB of whole frames; "
                 f"{N} truecolor-foreground targets per size, {text_bytes / 1e6:.2f} MB of text; both ways' text equal")
    for k, v in t.items():
        lines.append(f"  {k:<34} median {statistics.median(v):9.1f} us   least {min(v):9.1f} us")
    for name, label in (("tiles", "tick over tiles, host clock"), ("whole", "tick over whole frames, host clock")):
        lines.append(f"  {label:<34} median {statistics.median(wall[name]):9.1f} us   least {min(wall[name]):9.1f} us   (enqueue to synchronise)")
    for devs, plans, _, _ in ways.values():
        for p in plans:
            p.close()
        for d in devs:
            L.asciichat_hip_free(d)
    grid.close()
    whole.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
