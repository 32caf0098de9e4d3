#!/usr/bin/env python3
"""Times the rasteriser's two stages (asciichat_raster_parse, asciichat_raster_draw) on one GPU against a hipMemsetAsync of
the same pixel bytes, the write floor, in the same run: frames from Plan.render (truecolor foreground), a procedural 95-glyph
atlas at cell 10x20.  HIP events around every launch, the three alternating; medians over --launches after --warmup.
Writes the figures and the two ratios (raster / memset, parse / raster) to --out.  No time is a pass criterion."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(256, 80, 24), (16, 200, 60)]  # frames, cols, rows
CELL_W, CELL_H, BASELINE = 10, 20, 15


def atlas(pkg):
    """printable ASCII, every glyph 8 x 14 inside its cell, seeded noise coverage: 95 * 112 bytes"""
    rng = np.random.default_rng(1)
    glyphs, off = [], 0
    for cp in range(32, 127):
        glyphs.append((cp, 1, 13, 8, 14, 8, off))
        off += 8 * 14
    cov = rng.integers(0, 256, size=off, dtype=np.uint8)
    return pkg.raster_font(CELL_W, CELL_H, BASELINE, glyphs, cov.tobytes())


def hip_runtime():
    """the HIP runtime this process already uses (torch's)"""
    with open("/proc/self/maps") as f:
        paths = sorted({l.split()[-1] for l in f if "libamdhip64" in l})
    if not paths:
        raise RuntimeError("no HIP runtime is loaded")
    L = C.CDLL(paths[0])
    L.hipMemsetAsync.restype = C.c_int
    L.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_timing.txt"))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch

    import orc
    from __graft_entry__ import load_package

    pkg = load_package()
    if not torch.cuda.is_available() or pkg.raster_lib().asciichat_raster_device_count() <= 0:
        raise SystemExit("raster_timing: needs a GPU")
    hip = hip_runtime()
    stream = torch.cuda.current_stream().cuda_stream
    font = atlas(pkg)
    lines = ["# rasteriser stages against the write floor: scripts/raster_timing.py (HIP events around every launch, the three",
             f"# alternating; medians of {args.launches} launches after {args.warmup} warm-ups; {torch.cuda.get_device_name(0)})"]
    for n, cols, rows in SHAPES:
        src_w, src_h = 4 * cols, 4 * rows
        imgs = torch.from_numpy(np.stack([orc.frame_hash_noise(src_w, src_h, 10 + k) for k in range(4)])).cuda()
        frames = [pkg.frame_setup(imgs.data_ptr() + (i % 4) * 3 * src_w * src_h, src_w, src_h, cols, rows, 0, False, False, False)
                  for i in range(n)]
        plan = pkg.Plan(pkg.MODE_TRUE_FG, orc.PALETTE_STANDARD, frames)
        text = torch.zeros(n * plan.stride, dtype=torch.uint8, device="cuda")
        lens = torch.zeros(n, dtype=torch.int32, device="cuda")
        plan.render(text.data_ptr(), plan.stride, lens.data_ptr(), stream)
        torch.cuda.synchronize()
        text_bytes = int((lens.cpu().numpy().view(np.uint32)).astype(np.int64).sum())
        r = pkg.Raster(font, cols, rows, n)
        pixels = torch.empty(n * r.pitch, dtype=torch.uint8, device="cuda")
        status = torch.zeros(n, dtype=torch.int32, device="cuda")

        def parse():
            r.parse(text.data_ptr(), plan.stride, lens.data_ptr(), n, status.data_ptr(), stream)

        def draw():
            r.draw(n, pixels.data_ptr(), stream=stream)

        def memset():
            rc = hip.hipMemsetAsync(pixels.data_ptr(), 0, n * r.pitch, stream)
            if rc != 0:
                raise RuntimeError(f"hipMemsetAsync failed ({rc})")

        stages = (("parse", parse), ("raster", draw), ("memset", memset))
        times = {k: [] for k, _ in stages}
        for it in range(args.warmup + args.launches):
            evs = []
            for name, fn in stages:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                evs.append((name, a, b))
            torch.cuda.synchronize()
            if it >= args.warmup:
                for name, a, b in evs:
                    times[name].append(a.elapsed_time(b) * 1000.0)
        draw()  # (the memset came last: leave the images drawn)
        torch.cuda.synchronize()
        assert int(status.cpu().numpy().view(np.uint32).max()) == 0, "a frame outside the grammar"
        med = {k: statistics.median(v) for k, v in times.items()}
        lo = {k: min(v) for k, v in times.items()}
        px_bytes = n * r.pitch
        lines.append(f"{n} frames of {cols}x{rows} at cell {CELL_W}x{CELL_H}: {text_bytes / 1e6:.2f} MB of text -> {px_bytes / 1e6:.1f} MB of pixels per launch")
        for k in ("parse", "raster", "memset"):
            rate = f"   ({px_bytes / med[k] / 1e6:.2f} TB/s of pixels)" if k != "parse" else ""
            lines.append(f"  {k:<7} median {med[k]:9.1f} us   least {lo[k]:9.1f} us{rate}")
        lines.append(f"  raster / memset  {med['raster'] / med['memset']:.2f}      parse / raster  {med['parse'] / med['raster']:.2f}")
        r.close()
        plan.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
