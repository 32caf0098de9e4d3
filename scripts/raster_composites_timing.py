#!/usr/bin/env python3
"""Times the ways to the rasteriser's cells of a grid composite on one GPU, in the same run: (a) asciichat_raster_cells_from_images
over a set made by asciichat_raster_images_set_composites -- every target frame samples ONE uploaded composite of nine 1080p
sources, as a server's grid view does --, (b) the text path of the same frames (Plan.render, then asciichat_raster_parse), and
(c) asciichat_raster_cells_from_images over a plain set of the same grid sizes (each frame one of the nine 1080p sources), which
is the stage without the composite sampler.  The shapes and the atlas are scripts/raster_timing.py's: truecolor foreground, a
procedural 95-glyph atlas at cell 10x20.  HIP events around every launch, the four alternating; medians, least and the 10th and
90th percentiles over --launches after --warmup.  Asserts that (a) and (b) give the same pixels and status at the timed sizes
before anything is timed, then writes the figures and the two ratios, a / b and a / c, to --out.  No time is a pass criterion."""
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

from raster_timing import CELL_H, CELL_W, SHAPES, atlas  # noqa: E402

STAGES = ("render", "parse", "cells_from_composites", "cells_from_plain")
SRC_W, SRC_H, SOURCES = 1920, 1080, 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_composites_timing.txt"))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch

    import orc
    from __graft_entry__ import load_package

    pkg = load_package()
    if not torch.cuda.is_available() or pkg.raster_lib().asciichat_raster_device_count() <= 0:
        raise SystemExit("raster_composites_timing: needs a GPU")
    L = pkg.lib()
    stream = torch.cuda.current_stream().cuda_stream
    font = atlas(pkg)
    base = orc.frame_hash_noise(SRC_W, SRC_H, 10)
    imgs = torch.from_numpy(np.stack([np.roll(base, 37 * k, axis=1) for k in range(SOURCES)])).cuda()
    ptrs = [imgs.data_ptr() + k * 3 * SRC_W * SRC_H for k in range(SOURCES)]
    lines = ["# the rasteriser's cells of grid composites: scripts/raster_composites_timing.py (HIP events around every launch, the",
             f"# four alternating; medians of {args.launches} launches after {args.warmup} warm-ups; {torch.cuda.get_device_name(0)})"]
    for n, cols, rows in SHAPES:
        comp = pkg.Composite()
        L.achip_composite_setup(C.byref(comp), (C.c_void_p * SOURCES)(*ptrs), (C.c_int * SOURCES)(*[SRC_W] * SOURCES),
                                (C.c_int * SOURCES)(*[SRC_H] * SOURCES), SOURCES, cols, rows)
        comp_dev = C.c_void_p()
        if L.asciichat_hip_composite_upload(C.byref(comp), C.byref(comp_dev)) != 0:
            raise RuntimeError("composite_upload failed: " + pkg.last_error())
        target = pkg.frame_setup(None, cols, 2 * rows, cols, rows, 0, True, True, False)
        target.comp = comp_dev.value
        assert (target.pad_left + target.out_w, target.pad_top + target.out_h) == (cols, rows)
        targets = [target] * n
        plain = [pkg.frame_setup(ptrs[i % SOURCES], SRC_W, SRC_H, cols, rows, 0, False, False, False) for i in range(n)]
        plan = pkg.Plan(pkg.MODE_TRUE_FG, orc.PALETTE_STANDARD, targets)
        text = torch.zeros(n * plan.stride, dtype=torch.uint8, device="cuda")
        lens = torch.zeros(n, dtype=torch.int32, device="cuda")
        r = pkg.Raster(font, cols, rows, n)
        r.set_images_composites(pkg.MODE_TRUE_FG, orc.PALETTE_STANDARD, targets, stream=stream)
        rp = pkg.Raster(font, cols, rows, n)
        rp.set_images(pkg.MODE_TRUE_FG, orc.PALETTE_STANDARD, plain, stream=stream)
        pixels = torch.empty(n * r.pitch, dtype=torch.uint8, device="cuda")
        status = torch.zeros(n, dtype=torch.int32, device="cuda")

        def render():
            plan.render(text.data_ptr(), plan.stride, lens.data_ptr(), stream)

        def parse():
            r.parse(text.data_ptr(), plan.stride, lens.data_ptr(), n, status.data_ptr(), stream)

        def cells_from_composites():
            r.cells_from_images(n, status.data_ptr(), stream)

        def cells_from_plain():
            rp.cells_from_images(n, status.data_ptr(), stream)

        fns = dict(render=render, parse=parse, cells_from_composites=cells_from_composites, cells_from_plain=cells_from_plain)
        # both ways to the composite's cells, once, before anything is timed: the same pixels and the same status
        results = []
        for path in (("render", "parse"), ("cells_from_composites",)):
            pixels.fill_(0xEE)
            status.fill_(-1)
            for name in path:
                fns[name]()
            r.draw(n, pixels.data_ptr(), stream=stream)
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
        lines.append(f"{n} targets of {cols}x{rows} over one composite of {SOURCES} sources of {SRC_W}x{SRC_H} ({comp.cols}x{comp.rows} cells of "
                     f"{comp.cell_w}x{comp.cell_h} on a {comp.canvas_w}x{comp.canvas_h} canvas) at cell {CELL_W}x{CELL_H}: {text_bytes / 1e6:.2f} MB of "
                     f"text, {n * cols * rows * 12 / 1e6:.2f} MB of cells; both paths' pixels equal")
        for k in STAGES:
            v = sorted(times[k])
            lines.append(f"  {k:<22} median {med[k]:9.1f} us   least {v[0]:9.1f} us   p10 {v[len(v) // 10]:9.1f} us   p90 {v[len(v) * 9 // 10]:9.1f} us")
        both = med["render"] + med["parse"]
        a = med["cells_from_composites"]
        lines.append(f"  a / b  cells_from_composites / (render + parse)  {a / both:.4f}  (1 / {both / a:.0f})"
                     f"      a / c  cells_from_composites / cells_from_plain  {a / med['cells_from_plain']:.3f}")
        r.close()
        rp.close()
        plan.close()
        L.asciichat_hip_free(comp_dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
