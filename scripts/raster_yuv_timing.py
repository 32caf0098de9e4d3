#!/usr/bin/env python3
"""Times the rasteriser's YUV 4:2:0 draw (asciichat_raster_draw_yuv420, both layouts) on one GPU against the RGBA draw of the
same parsed cells and a hipMemsetAsync of the 1.5 bytes per pixel it writes, in the same run: the shapes, frames and atlas of
scripts/raster_timing.py, one handle per shape.  HIP events around every launch, the four alternating; medians over
--launches after --warmup.  Writes the figures to --out.  No time is a pass criterion."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import raster_timing as RT  # noqa: E402  (the shapes, the atlas and the runtime's memset)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_yuv_timing.txt"))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch

    import orc
    from __graft_entry__ import load_package

    pkg = load_package()
    if not torch.cuda.is_available() or pkg.raster_lib().asciichat_raster_device_count() <= 0:
        raise SystemExit("raster_yuv_timing: needs a GPU")
    hip = RT.hip_runtime()
    stream = torch.cuda.current_stream().cuda_stream
    font = RT.atlas(pkg)
    lines = ["# the YUV 4:2:0 draw against the RGBA draw and the write floor: scripts/raster_yuv_timing.py (HIP events around every",
             f"# launch, the four alternating; medians of {args.launches} launches after {args.warmup} warm-ups; {torch.cuda.get_device_name(0)})"]
    for n, cols, rows in RT.SHAPES:
        src_w, src_h = 4 * cols, 4 * rows
        imgs = torch.from_numpy(np.stack([orc.frame_hash_noise(src_w, src_h, 10 + k) for k in range(4)])).cuda()
        frames = [pkg.frame_setup(imgs.data_ptr() + (i % 4) * 3 * src_w * src_h, src_w, src_h, cols, rows, 0, False, False, False)
                  for i in range(n)]
        plan = pkg.Plan(pkg.MODE_TRUE_FG, orc.PALETTE_STANDARD, frames)
        text = torch.zeros(n * plan.stride, dtype=torch.uint8, device="cuda")
        lens = torch.zeros(n, dtype=torch.int32, device="cuda")
        plan.render(text.data_ptr(), plan.stride, lens.data_ptr(), stream)
        r = pkg.Raster(font, cols, rows, n)
        assert r.yuv_pitch % 4 == 0
        pixels = torch.empty(n * r.pitch, dtype=torch.uint8, device="cuda")
        planes = torch.empty(n * r.yuv_pitch, dtype=torch.uint8, device="cuda")
        status = torch.zeros(n, dtype=torch.int32, device="cuda")
        r.parse(text.data_ptr(), plan.stride, lens.data_ptr(), n, status.data_ptr(), stream)  # once: every draw below reads these cells
        torch.cuda.synchronize()
        assert int(status.cpu().numpy().view(np.uint32).max()) == 0, "a frame outside the grammar"

        def memset():
            rc = hip.hipMemsetAsync(planes.data_ptr(), 0, n * r.yuv_pitch, stream)
            if rc != 0:
                raise RuntimeError(f"hipMemsetAsync failed ({rc})")

        stages = (("i420", lambda: r.draw_yuv420(n, planes.data_ptr(), pkg.RASTER_YUV_I420, stream=stream)),
                  ("nv12", lambda: r.draw_yuv420(n, planes.data_ptr(), pkg.RASTER_YUV_NV12, stream=stream)),
                  ("rgba", lambda: r.draw(n, pixels.data_ptr(), stream=stream)),
                  ("memset", memset))
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
        med = {k: statistics.median(v) for k, v in times.items()}
        lo = {k: min(v) for k, v in times.items()}
        yuv_bytes, px_bytes = n * r.yuv_pitch, n * r.pitch
        lines.append(f"{n} frames of {cols}x{rows} at cell {RT.CELL_W}x{RT.CELL_H}: {yuv_bytes / 1e6:.1f} MB of planes per launch "
                     f"({px_bytes / 1e6:.1f} MB as RGBA)")
        for k, nbytes in (("i420", yuv_bytes), ("nv12", yuv_bytes), ("rgba", px_bytes), ("memset", yuv_bytes)):
            lines.append(f"  {k:<7} median {med[k]:9.1f} us   least {lo[k]:9.1f} us   ({nbytes / med[k] / 1e6:.2f} TB/s written, "
                         f"{n * r.width * r.height / med[k] / 1e3:.2f} Gpx/s)")
        lines.append(f"  i420 / rgba  {med['i420'] / med['rgba']:.2f}   nv12 / rgba  {med['nv12'] / med['rgba']:.2f}   "
                     f"i420 / memset  {med['i420'] / med['memset']:.2f}   rgba median - least  {med['rgba'] - lo['rgba']:.1f} us")
        r.close()
        plan.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
