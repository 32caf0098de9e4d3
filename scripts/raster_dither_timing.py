#!/usr/bin/env python3
"""Times the two ways to the rasteriser's cells of Floyd-Steinberg frames (ACHIP_MODE_16_DITHER_BG, the background form) on one
GPU, in the same run: (a) asciichat_raster_cells_from_images over a set made by asciichat_raster_images_set_dithered, and (b) the
text path of the same frames -- the plan's mode-9 render, then asciichat_raster_parse --, and the draw both end in.  Plain frames
(every frame one of nine 1080p sources) at the shapes and with the atlas of scripts/raster_timing.py, then 256 targets over ONE
uploaded composite of nine 1080p sources.  HIP events around every launch, the stages alternating; medians, least and the 10th and
90th percentiles over --launches after --warmup.  Asserts that (a) and (b) give the same pixels and status before anything is
timed, then writes the figures and the ratios a / render and a / (render + parse) to --out.  The yardstick of the cells stage is
the plan's own render measured here: it runs the same serial chain.  No time is a pass criterion."""
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

STAGES = ("render", "parse", "cells_dithered", "draw")
SRC_W, SRC_H, SOURCES = 1920, 1080, 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_dither_timing.txt"))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch

    import orc
    from __graft_entry__ import load_package

    pkg = load_package()
    if not torch.cuda.is_available() or pkg.raster_lib().asciichat_raster_device_count() <= 0:
        raise SystemExit("raster_dither_timing: needs a GPU")
    L = pkg.lib()
    stream = torch.cuda.current_stream().cuda_stream
    font = atlas(pkg)
    base = orc.frame_hash_noise(SRC_W, SRC_H, 10)
    imgs = torch.from_numpy(np.stack([np.roll(base, 37 * k, axis=1) for k in range(SOURCES)])).cuda()
    ptrs = [imgs.data_ptr() + k * 3 * SRC_W * SRC_H for k in range(SOURCES)]
    lines = ["# the rasteriser's cells of Floyd-Steinberg frames: scripts/raster_dither_timing.py (HIP events around every launch, the",
             f"# four alternating; medians of {args.launches} launches after {args.warmup} warm-ups; {torch.cuda.get_device_name(0)})"]
    n0, cols0, rows0 = SHAPES[0]
    for kind, n, cols, rows in [("plain", *s) for s in SHAPES] + [("composite", n0, cols0, rows0)]:
        comp_dev = C.c_void_p()
        if kind == "plain":
            frames = [pkg.frame_setup(ptrs[i % SOURCES], SRC_W, SRC_H, cols, rows, 1, False, False, False) for i in range(n)]
            what = f"{n} frames of {SRC_W}x{SRC_H} -> {cols}x{rows}"
        else:
            comp = pkg.Composite()
            L.achip_composite_setup(C.byref(comp), (C.c_void_p * SOURCES)(*ptrs), (C.c_int * SOURCES)(*[SRC_W] * SOURCES),
                                    (C.c_int * SOURCES)(*[SRC_H] * SOURCES), SOURCES, cols, rows)
            if L.asciichat_hip_composite_upload(C.byref(comp), C.byref(comp_dev)) != 0:
                raise RuntimeError("composite_upload failed: " + pkg.last_error())
            target = pkg.frame_setup(None, cols, 2 * rows, cols, rows, 1, True, True, False)
            target.comp = comp_dev.value
            assert (target.pad_left + target.out_w, target.pad_top + target.out_h) == (cols, rows)
            frames = [target] * n
            what = f"{n} targets of {cols}x{rows} over one composite of {SOURCES} sources of {SRC_W}x{SRC_H}"
        assert all(f.ops & 48 == 0 for f in frames)  # the background form
        plan = pkg.Plan(pkg.MODE_16_DITHER_BG, orc.PALETTE_STANDARD, frames)
        text = torch.zeros(n * plan.stride, dtype=torch.uint8, device="cuda")
        lens = torch.zeros(n, dtype=torch.int32, device="cuda")
        r = pkg.Raster(font, cols, rows, n)
        r.set_images_dithered(orc.PALETTE_STANDARD, frames, stream=stream)
        pixels = torch.empty(n * r.pitch, dtype=torch.uint8, device="cuda")
        status = torch.zeros(n, dtype=torch.int32, device="cuda")

        def render():
            plan.render(text.data_ptr(), plan.stride, lens.data_ptr(), stream)

        def parse():
            r.parse(text.data_ptr(), plan.stride, lens.data_ptr(), n, status.data_ptr(), stream)

        def cells_dithered():
            r.cells_from_images(n, status.data_ptr(), stream)

        def draw():
            r.draw(n, pixels.data_ptr(), stream=stream)

        fns = dict(render=render, parse=parse, cells_dithered=cells_dithered, draw=draw)
        # both ways to the cells, once, before anything is timed: the same pixels and the same status
        results = []
        for path in (("render", "parse"), ("cells_dithered",)):
            pixels.fill_(0xEE)
            status.fill_(-1)
            for name in path:
                fns[name]()
            draw()
            torch.cuda.synchronize()
            results.append((pixels.cpu().numpy().copy(), status.cpu().numpy().copy()))
        assert np.array_equal(results[0][0], results[1][0]), "the two paths' pixels differ"
        assert np.array_equal(results[0][1], results[1][1]) and int(results[0][1].view(np.uint32).max()) == 0, "the two paths' status differ"
        text_bytes = int((lens.cpu().numpy().view(np.uint32)).astype(np.int64).sum())

        times = {k: [] for k in STAGES}
        for it in range(args.warmup + args.launches):
            evs = []
            for name in STAGES:  # (draw follows cells_dithered: it paints the cells of the stage that ran last)
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
        lines.append(f"{what} at cell {CELL_W}x{CELL_H}, background form: {text_bytes / 1e6:.2f} MB of text, {n * cols * rows * 12 / 1e6:.2f} MB "
                     f"of cells; both paths' pixels equal")
        for k in STAGES:
            v = sorted(times[k])
            lines.append(f"  {k:<16} median {med[k]:9.1f} us   least {v[0]:9.1f} us   p10 {v[len(v) // 10]:9.1f} us   p90 {v[len(v) * 9 // 10]:9.1f} us")
        a, both = med["cells_dithered"], med["render"] + med["parse"]
        lines.append(f"  cells_dithered / render  {a / med['render']:.3f}      cells_dithered / (render + parse)  {a / both:.4f}  (1 / {both / a:.0f})")
        r.close()
        plan.close()
        if comp_dev.value:
            L.asciichat_hip_free(comp_dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
