#!/usr/bin/env python3
"""Times libasciichat_pix.so on one GPU, all in one run, for 256 BGRA and 256 BGR24 1080p sources -> 80x24:
  - Pix.run (only the pixels a target samples), to read beside asciichat_yuv_run's figure in profiles/yuv_timing.txt;
  - Pix.run_whole at the shipped run of pixels per lane and, with --other-lib (the library built at the other
    PIX_WHOLE_PIXELS: make EXTRA=-DPIX_WHOLE_PIXELS=N BUILD=build_pixN PIXOUT=libasciichat_pixN.so libasciichat_pixN.so), at
    the other one, beside a device-to-device hipMemcpyAsync that moves as many bytes as run_whole reads plus writes;
  - Pix.run_box beside the route it replaces -- Pix.run_whole into a slab of whole RGB24 frames, then Box.run over that slab --
    and beside a device-to-device copy of the sources' own bytes.
HIP events around every stage, the stages alternating within one run; medians over --launches after --warmup.  The images of
the routes are asserted equal before anything is timed.  Writes the figures to --out."""
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
COLS, ROWS = 80, 24
DISTINCT = 8  # different contents; every source has device memory of its own


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pix_timing.txt"))
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=256, help="sources of the batch (a rehearsal may take fewer)")
    ap.add_argument("--other-lib", default=None, help="libasciichat_pix.so built at the other PIX_WHOLE_PIXELS")
    ap.add_argument("--shipped-run", type=int, default=4, help="PIX_WHOLE_PIXELS of the package's library (a label)")
    ap.add_argument("--other-run", type=int, default=16, help="PIX_WHOLE_PIXELS of --other-lib (a label)")
    args = ap.parse_args()
    import torch

    import orc
    import pix_ref as PR
    import pix_support as PS
    from __graft_entry__ import load_package

    pkg = load_package()
    if not torch.cuda.is_available() or pkg.pix_lib().asciichat_pix_device_count() <= 0:
        raise SystemExit("pix_timing: needs a GPU")
    hip = hip_runtime()
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream
    other = PS.bind(C.CDLL(os.path.abspath(args.other_lib))) if args.other_lib else None
    n = args.frames
    lines = ["# packed RGB sources: scripts/pix_timing.py (HIP events around every stage, the stages alternating; medians of "
             f"{args.launches} launches after {args.warmup} warm-ups; {torch.cuda.get_device_name(0)})"]

    rng = np.random.default_rng(12)
    base = orc.frame_smooth(W, H).astype(np.int32)
    for fmt in (PR.BGRA, PR.BGR):
        bpp = PR.BPP[fmt]
        per = bpp * W * H
        host = []
        for k in range(DISTINCT):
            px = np.empty((H, W, bpp), dtype=np.uint8)
            px[:, :, :3] = np.clip(base[:, :, ::-1] + rng.integers(-20, 21, (H, W, 3)), 0, 255)
            if bpp == 4:
                px[:, :, 3] = rng.integers(0, 256, (H, W))
            host.append(px.reshape(-1))
        slab = torch.from_numpy(np.stack(host)).cuda()[torch.arange(n, device="cuda") % DISTINCT].contiguous()
        assert slab.data_ptr() % 16 == 0 and per % 16 == 0
        sources = [pkg.pix_source(fmt, W, H, slab.data_ptr() + i * per) for i in range(n)]
        whole_bytes = 3 * W * H
        whole = torch.full((n * whole_bytes,), 0xA5, dtype=torch.uint8, device="cuda")  # the slab run_whole writes and the route needs
        frames = [pkg.frame_setup(whole.data_ptr() + i * whole_bytes, W, H, COLS, ROWS, 0, False, False, False) for i in range(n)]
        assert all(f is not None and (f.out_w, f.out_h) == (COLS, ROWS) for f in frames)
        p = pkg.Pix(n)
        p.set(sources, frames, stream=stream)
        box = pkg.Box(frames)
        assert p.pitch == box.pitch and p.whole_pitch == whole_bytes
        images = [torch.full((n * box.pitch,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(3)]
        moved_whole = n * (per + whole_bytes)  # what run_whole reads plus writes
        floor = torch.empty(max(moved_whole // 2, n * per) + 16, dtype=torch.uint8, device="cuda")

        def run():
            p.run(images[2].data_ptr(), stream=stream)

        def run_whole():
            p.run_whole(whole.data_ptr(), whole_bytes, stream=stream)

        def box_run():
            box.run(images[0].data_ptr(), stream=stream)

        def route():
            run_whole()
            box_run()

        def run_box():
            p.run_box(images[1].data_ptr(), stream=stream)

        def copy_of(nbytes, src):
            def fn():
                rc = hip.hipMemcpyAsync(floor.data_ptr(), src.data_ptr(), nbytes, 3, stream)
                if rc != 0:
                    raise RuntimeError(f"hipMemcpyAsync failed ({rc})")
            return fn

        # a copy that moves what run_whole moves: half of (read + written) bytes read, as many written; out of the slab it wrote
        # and the sources (both are as large or larger)
        copy_whole = copy_of(moved_whole // 2, slab if slab.numel() >= moved_whole // 2 else whole)
        copy_sources = copy_of(n * per, slab)
        stages = {"pix_run": run, f"pix_run_whole ({args.shipped_run} pixels a lane)": run_whole}
        route()
        run_box()
        run()
        torch.cuda.synchronize()
        assert torch.equal(images[0], images[1]), "run_box differs from run_whole + Box.run"
        assert int((images[1] != 0xA5).sum().item()) > n * 3 * COLS * ROWS // 2 and int((images[2] != 0xA5).sum().item()) > n * 3 * COLS * ROWS // 2
        if other is not None:
            oh = PS.Handle(other, n, stream)
            keep = (pkg.PixSource * n)(*sources)
            assert other.asciichat_pix_set(oh.h, C.cast(keep, C.c_void_p), None, n, stream) == 0, oh.error()
            whole2 = torch.full((n * whole_bytes,), 0x5A, dtype=torch.uint8, device="cuda")

            def run_whole_other():
                rc = oh.run_whole(whole2.data_ptr(), whole_bytes)
                if rc != 0:
                    raise RuntimeError(oh.error())

            run_whole_other()
            torch.cuda.synchronize()
            assert torch.equal(whole, whole2), "the two runs' whole frames differ"
            stages[f"pix_run_whole ({args.other_run} pixels a lane)"] = run_whole_other
        stages.update({"memcpy D2D, run_whole's bytes": copy_whole, "box_run": box_run, "route: run_whole + box_run": route, "pix_run_box": run_box,
                       "memcpy D2D of the sources": copy_sources})
        t = timed(stages, args.launches, args.warmup)
        med = {k: statistics.median(v) for k, v in t.items()}
        lines.append(f"{n} {PR.NAMES[fmt]} sources of {W}x{H} -> {COLS}x{ROWS} ({n * per / 1e6:.0f} MB of sources, {n * whole_bytes / 1e6:.0f} MB of whole frames, "
                     f"{n * 3 * COLS * ROWS / 1e3:.0f} KB of images; run_box's images equal the route's" + ("; both runs' whole frames equal" if other else "") + ")")
        for k, v in t.items():
            note = ""
            if k.startswith("pix_run_whole"):
                note = f"   {moved_whole / med[k] / 1e6:.2f} TB/s read + written"
            if k.startswith("memcpy D2D, run_whole"):
                note = f"   {moved_whole // 2 * 2 / med[k] / 1e6:.2f} TB/s read + written ({moved_whole // 2 / 1e6:.0f} MB copied)"
            if k == "pix_run_box":
                note = f"   {n * per / med[k] / 1e6:.2f} TB/s of sources read, {med['route: run_whole + box_run'] / med[k]:.2f} x the route's rate"
            if k == "memcpy D2D of the sources":
                note = f"   {n * per / med[k] / 1e6:.2f} TB/s read (and as much written)"
            lines.append(f"  {k:<36} median {med[k]:9.1f} us   least {min(v):9.1f} us{note}")
        p.close()
        box.close()
        if other is not None:
            oh.close()
            del whole2
        del slab, whole, images, floor
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
