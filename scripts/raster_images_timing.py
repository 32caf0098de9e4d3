#!/usr/bin/env python3
"""Times the two ways to the rasteriser's cells on one GPU, in the same run: the text path (Plan.render, then
asciichat_raster_parse) and asciichat_raster_cells_from_images over the same descriptors, beside asciichat_raster_draw and a
hipMemsetAsync of the same pixel bytes, the write floor.  The shapes, the sources and the atlas are scripts/raster_timing.py's:
truecolor foreground, a procedural 95-glyph atlas at cell 10x20.  HIP events around every launch, the five alternating; medians
over --launches after --warmup.  Asserts that both paths give the same pixels and status at the timed sizes, then writes the
figures and the two ratios (cells_from_images / (render + parse), cells_from_images / draw) to --out.  No time is a pass
criterion."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from raster_timing import CELL_H, CELL_W, SHAPES, atlas, hip_runtime  # noqa: E402

STAGES = ("render", "parse", "cells_from_images", "draw", "memset")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_images_timing.txt"))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch

    import orc
    from __graft_entry__ import load_package

    pkg = load_package()
    if not torch.cuda.is_available() or pkg.raster_lib().asciichat_raster_device_count() <= 0:
        raise SystemExit("raster_images_timing: needs a GPU")
    hip = hip_runtime()
    stream = torch.cuda.current_stream().cuda_stream
    font = atlas(pkg)
    lines = ["# the rasteriser's cells from the text and from the images: scripts/raster_images_timing.py (HIP events around every",
             f"# launch, the five alternating; medians of {args.launches} launches after {args.warmup} warm-ups; {torch.cuda.get_device_name(0)})"]
    for n, cols, rows in SHAPES:
        src_w, src_h = 4 * cols, 4 * rows
        imgs = torch.from_numpy(np.stack([orc.frame_hash_noise(src_w, src_h, 10 + k) for k in range(4)])).cuda()
        frames = [pkg.frame_setup(imgs.data_ptr() + (i % 4) * 3 * src_w * src_h, src_w, src_h, cols, rows, 0, False, False, False)
                  for i in range(n)]
        plan = pkg.Plan(pkg.MODE_TRUE_FG, orc.PALETTE_STANDARD, frames)
        text = torch.zeros(n * plan.stride, dtype=torch.uint8, device="cuda")
        lens = torch.zeros(n, dtype=torch.int32, device="cuda")
        r = pkg.Raster(font, cols, rows, n)
        r.set_images(pkg.MODE_TRUE_FG, orc.PALETTE_STANDARD, frames, stream=stream)
        pixels = torch.empty(n * r.pitch, dtype=torch.uint8, device="cuda")
        status = torch.zeros(n, dtype=torch.int32, device="cuda")

        def render():
            plan.render(text.data_ptr(), plan.stride, lens.data_ptr(), stream)

        def parse():
            r.parse(text.data_ptr(), plan.stride, lens.data_ptr(), n, status.data_ptr(), stream)

        def cells_from_images():
            r.cells_from_images(n, status.data_ptr(), stream)

        def draw():
            r.draw(n, pixels.data_ptr(), stream=stream)

        def memset():
            rc = hip.hipMemsetAsync(pixels.data_ptr(), 0, n * r.pitch, stream)
            if rc != 0:
                raise RuntimeError(f"hipMemsetAsync failed ({rc})")

        fns = dict(render=render, parse=parse, cells_from_images=cells_from_images, draw=draw, memset=memset)
        # both paths, once, before anything is timed: the same pixels and the same status
        results = []
        for path in (("render", "parse", "draw"), ("cells_from_images", "draw")):
            pixels.fill_(0xEE)
            status.fill_(-1)
            for name in path:
                fns[name]()
            torch.cuda.synchronize()
            results.append((pixels.cpu().numpy().copy(), status.cpu().numpy().copy()))
        assert np.array_equal(results[0][0], results[1][0]), "the two paths' pixels differ"
        assert np.array_equal(results[0][1], results[1][1]) and int(results[0][1].view(np.uint32).max()) == 0, "the two paths' status differ"
        text_bytes = int((lens.cpu().numpy().view(np.uint32)).astype(np.int64).sum())

        times = {k: [] for k in STAGES}
        for it in range(args.warmup + args.launches):
            evs = []
            for name in STAGES:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fns[name]()
                b.record()
                evs.append((name, a, b))
            torch.cuda.synchronize()
            if it >= args.warmup:
                for name, a, b in evs:
                    times[name].append(a.elapsed_time(b) * 1000.0)
        med = {k: statistics.median(v) for k, v in times.items()}
        lo = {k: min(v) for k, v in times.items()}
        px_bytes = n * r.pitch
        lines.append(f"{n} frames of {cols}x{rows} from {src_w}x{src_h} sources at cell {CELL_W}x{CELL_H}: {text_bytes / 1e6:.2f} MB of text, "
                     f"{n * cols * rows * 12 / 1e6:.2f} MB of cells, {px_bytes / 1e6:.1f} MB of pixels per launch; both paths' pixels equal")
        for k in STAGES:
            lines.append(f"  {k:<18} median {med[k]:9.1f} us   least {lo[k]:9.1f} us")
        both = med["render"] + med["parse"]
        lines.append(f"  cells_from_images / (render + parse)  {med['cells_from_images'] / both:.4f}  (1 / {both / med['cells_from_images']:.0f})"
                     f"      cells_from_images / draw  {med['cells_from_images'] / med['draw']:.3f}")
        r.close()
        plan.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
