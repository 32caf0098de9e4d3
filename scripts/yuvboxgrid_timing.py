#!/usr/bin/env python3
"""Times libasciichat_yuvboxgrid.so on one GPU: YuvBoxGrid.run (the YUV tiles of grid composites box-averaged straight from their
planes) and asciichat_hip_box_composites over its rewritten descriptors, beside the route they replace -- Yuv.run_whole into a
slab of whole RGB24 frames, then asciichat_hip_box_composites over descriptors pointing into that slab.  Three steps, each a child
process of its own under its own time limit (a step that fails or runs out of time ends the run: nothing more is started):
  shape    nine NV12 1080p sources into the 27 tiles of the composites at 80x24, 160x48 and 200x60, one frame per composite;
  targets  one composite of the nine sources at 160x48 with 256 targets;
  widths   YuvBoxGrid.run at the first shape, and for the one composite at 160x48 (9 tiles), from builds of the library at the four candidate segment widths (no split, 1024,
           512, 256; built here when missing: make SEG_COLS=N into ascii-chat_amd/build_segN/).
HIP events around every stage, the ways alternating in one run; medians over --launches after --warmup.  The images of the two
routes are asserted equal before anything is printed, and so are the tiles of every width.  A device-to-device hipMemcpyAsync of
the sources' bytes is the traffic's own floor.  Writes the figures, and the width the library ships with, to --out."""
import argparse
import ctypes as C
import os
import re
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ascii-chat_amd")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

W, H, SOURCES = 1920, 1080, 9
SIZES = ((80, 24), (160, 48), (200, 60))
WIDTHS = (0, 1024, 512, 256)
STEPS = {"shape": 240, "targets": 240, "widths": 240}  # seconds a step may take


def variant_path(width):
    return os.path.join(PKG, f"build_seg{width}", "libasciichat_yuvboxgrid.so")


def build_variants():
    """the library at each candidate width, where it is not there yet (two translation units each)"""
    for w in WIDTHS:
        if not os.path.exists(variant_path(w)):
            out = f"build_seg{w}/libasciichat_yuvboxgrid.so"
            subprocess.run(["make", "-C", PKG, f"BUILD=build_seg{w}", f"XOUT={out}", f"SEG_COLS={w}", out], check=True, timeout=600,
                           stdout=subprocess.DEVNULL)


class Bench:
    """the nine sources on the device and what every step needs of them"""

    def __init__(self):
        import torch

        import orc
        import yuv_ref as YR
        from __graft_entry__ import load_package
        from raster_timing import hip_runtime

        self.torch, self.pkg = torch, load_package()
        if not torch.cuda.is_available() or self.pkg.yuvboxgrid_lib().asciichat_yuvboxgrid_device_count() <= 0:
            raise SystemExit("yuvboxgrid_timing: needs a GPU")
        self.hip = hip_runtime()
        self.hip.hipMemcpyAsync.restype = C.c_int
        self.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.stream = torch.cuda.current_stream().cuda_stream
        rng = np.random.default_rng(11)
        base = orc.frame_smooth(W, H).astype(np.int32)
        cshape = YR.chroma_size(W, H)[::-1]
        host = []
        for k in range(SOURCES):
            Y = np.clip(base[:, :, k % 3] + rng.integers(-20, 21, (H, W)), 0, 255).astype(np.uint8)
            planes, _ = YR.pack(YR.NV12, Y, rng.integers(0, 256, cshape, dtype=np.uint8), rng.integers(0, 256, cshape, dtype=np.uint8))
            host.append(np.concatenate(planes))
        self.per = host[0].size
        self.samples = torch.from_numpy(np.stack(host)).cuda()
        self.floor_dst = torch.empty_like(self.samples)
        self.sources = [self.pkg.yuv_source(YR.NV12, W, H, [self.samples.data_ptr() + i * self.per, self.samples.data_ptr() + i * self.per + planes[0].size])
                        for i in range(SOURCES)]
        self.whole = self.pkg.Yuv(SOURCES)
        self.whole.set(self.sources, None, stream=self.stream)
        self.pitch = self.whole.whole_pitch
        self.rgb = torch.empty(SOURCES * self.pitch, dtype=torch.uint8, device="cuda")

    def composites(self, sizes):
        """achip_composite_setup's descriptors over the whole frames"""
        comps = []
        for tw, th in sizes:
            c = self.pkg.Composite()
            ptrs = (C.c_void_p * SOURCES)(*[self.rgb.data_ptr() + i * self.pitch for i in range(SOURCES)])
            self.pkg.lib().achip_composite_setup(C.byref(c), ptrs, (C.c_int * SOURCES)(*[W] * SOURCES), (C.c_int * SOURCES)(*[H] * SOURCES), SOURCES, tw, th)
            assert c.n_src == SOURCES and all(c.s[k].src for k in range(SOURCES))
            comps.append(c)
        return comps

    def frame(self, comp, tw, th):
        """the descriptor of a composite frame averaged to the terminal's size: the canvas as its source"""
        f = self.pkg.Frame()
        f.src_w, f.src_h, f.out_w, f.out_h = comp.canvas_w, comp.canvas_h, tw, th
        f.x_ratio, f.y_ratio = (comp.canvas_w << 16) // tw + 1, (comp.canvas_h << 16) // th + 1
        return f

    def run_whole(self):
        self.whole.run_whole(self.rgb.data_ptr(), self.pitch, stream=self.stream)

    def memcpy(self):
        rc = self.hip.hipMemcpyAsync(self.floor_dst.data_ptr(), self.samples.data_ptr(), SOURCES * self.per, 3, self.stream)
        if rc != 0:
            raise RuntimeError(f"hipMemcpyAsync failed ({rc})")


def report(t, moved, ours, route):
    med = {k: statistics.median(v) for k, v in t.items()}
    lines = []
    for k, v in t.items():
        note = ""
        if k == ours:
            note = f"   {med[route] / med[k]:.2f} x the old route's rate"
        if k.startswith("memcpy"):
            note = f"   {moved / med[k] / 1e6:.2f} TB/s read (and as much written)"
        lines.append(f"  {k:<44} median {med[k]:9.1f} us   least {min(v):9.1f} us{note}")
    return lines, med


def compare(b, sizes, targets, args):
    """the two routes for the composites at `sizes`, `targets` frames per composite -> the lines"""
    from yuv_timing import timed
    torch, pkg, stream = b.torch, b.pkg, b.stream
    comps = b.composites(sizes)
    grid = pkg.YuvBoxGrid(len(sizes) * SOURCES)
    per_comp = [b.sources] * len(sizes)
    grid.set(comps, per_comp, stream=stream)
    tiles = torch.full((grid.tiles_bytes(),), 0xA5, dtype=torch.uint8, device="cuda")
    rewritten = grid.composites(tiles.data_ptr())
    frames = [b.frame(c, tw, th) for c, (tw, th) in zip(comps, sizes) for _ in range(targets)]
    old_comps = [c for c in comps for _ in range(targets)]
    new_comps = [c for c in rewritten for _ in range(targets)]
    boxes = [pkg.Box(frames, comps=old_comps, stream=stream), pkg.Box(frames, comps=new_comps, stream=stream)]
    assert boxes[0].pitch == boxes[1].pitch
    images = [torch.full((len(frames) * boxes[0].pitch,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]

    def box_old():
        boxes[0].run(images[0].data_ptr(), stream=stream)

    def box_new():
        boxes[1].run(images[1].data_ptr(), stream=stream)

    def tiles_run():
        grid.run(tiles.data_ptr(), stream=stream)

    def old_route():
        b.run_whole()
        box_old()

    def new_route():
        tiles_run()
        box_new()

    old_route()
    new_route()
    torch.cuda.synchronize()
    assert torch.equal(images[0], images[1]), "the two routes' images differ"
    assert int((images[1] != 0xA5).sum().item()) > sum(3 * tw * th for tw, th in sizes) * targets // 2, "nothing was stored"
    t = timed({"yuv_run_whole (9 x 1080p)": b.run_whole, "box_composites over whole frames": box_old, "old route: run_whole + box_composites": old_route,
               "yuvboxgrid_run": tiles_run, "box_composites over the averaged tiles": box_new, "new route: yuvboxgrid_run + box_composites": new_route,
               "memcpy D2D of the sources": b.memcpy}, args.launches, args.warmup)
    moved = SOURCES * b.per
    n_tiles = len(sizes) * SOURCES
    lines = [f"{SOURCES} NV12 sources of {W}x{H}, composites at {', '.join(f'{w}x{h}' for w, h in sizes)} ({n_tiles} tiles, {grid.tiles_bytes() / 1e3:.0f} KB of "
             f"tiles), {targets} target{'s' if targets > 1 else ''} per composite ({moved / 1e6:.0f} MB of samples; the two routes' images equal; the old "
             f"route's slab of whole frames: {b.rgb.numel() / 1e6:.0f} MB, the new route needs none)"]
    body, med = report(t, moved, "new route: yuvboxgrid_run + box_composites", "old route: run_whole + box_composites")
    lines += body
    lines.append(f"  the pass against the conversion it replaces: yuvboxgrid_run {med['yuvboxgrid_run']:.1f} us, yuv_run_whole "
                 f"{med['yuv_run_whole (9 x 1080p)']:.1f} us ({med['yuv_run_whole (9 x 1080p)'] / med['yuvboxgrid_run']:.2f} x)")
    ok = med["new route: yuvboxgrid_run + box_composites"] <= med["old route: run_whole + box_composites"]
    lines.append(f"  condition (the new route's median does not exceed the old route's, no margin): {'met' if ok else 'MISSED'}")
    for x in boxes:
        x.close()
    grid.close()
    return lines


def widths(b, args, sizes):
    from yuv_timing import timed
    torch, pkg, stream = b.torch, b.pkg, b.stream
    comps = b.composites(sizes)
    per_comp = [b.sources] * len(sizes)
    grids, slabs, fns = [], [], {}
    for w in WIDTHS:
        g = pkg.YuvBoxGrid(len(sizes) * SOURCES, lib=pkg.yuvboxgrid_lib(variant_path(w)))
        g.set(comps, per_comp, stream=stream)
        slab = torch.full((g.tiles_bytes(),), 0xA5, dtype=torch.uint8, device="cuda")
        grids.append(g)
        slabs.append(slab)
        fns[f"yuvboxgrid_run, segment width {w if w else 'none (no split)'}"] = (lambda g=g, slab=slab: g.run(slab.data_ptr(), stream=stream))
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    assert all(torch.equal(slabs[0], s) for s in slabs[1:]), "the widths' tiles differ"
    assert int((slabs[0] != 0xA5).sum().item()) > slabs[0].numel() // 2, "nothing was stored"
    fns["memcpy D2D of the sources"] = b.memcpy
    t = timed(fns, args.launches, args.warmup)
    lines = [f"the segment width: {SOURCES} NV12 sources of {W}x{H} into the {len(sizes) * SOURCES} tiles of the composite{'s' if len(sizes) > 1 else ''} at "
             f"{', '.join(f'{w}x{h}' for w, h in sizes)}, one build of the library per width, alternating in one run (the tiles of all four equal)"]
    body, med = report(t, SOURCES * b.per, None, None)
    lines += body
    best = min((k for k in med if k.startswith("yuvboxgrid_run")), key=lambda k: med[k])
    lines.append(f"  least median: {best}")
    for g in grids:
        g.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuvboxgrid_timing.txt"))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--targets", type=int, default=256, help="targets of the second step (a rehearsal may take fewer)")
    ap.add_argument("--step", choices=list(STEPS), help="run this step alone, in this process, and print its lines")
    args = ap.parse_args()
    if args.step:
        b = Bench()
        if args.step == "shape":
            lines = compare(b, SIZES, 1, args)
        elif args.step == "targets":
            lines = compare(b, (SIZES[1],), args.targets, args)
        else:
            lines = widths(b, args, SIZES) + widths(b, args, (SIZES[1],))
        print("\n".join([f"# {b.torch.cuda.get_device_name(0)}"] + lines))
        return
    build_variants()
    lines = [f"# The YUV tiles of grid composites box-averaged from their planes: scripts/yuvboxgrid_timing.py (HIP events around every stage, the ways "
             f"alternating; medians of {args.launches} launches after {args.warmup} warm-ups; each step a process of its own)"]
    for step, limit in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--launches", str(args.launches), "--warmup", str(args.warmup),
               "--targets", str(args.targets)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"yuvboxgrid_timing: step {step} ran out of its {limit} s: nothing more is started")
        if out.returncode != 0:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
            raise SystemExit(f"yuvboxgrid_timing: step {step} ended with {out.returncode}: nothing more is started")
        got = out.stdout.strip().splitlines()
        if len(lines) == 1:
            lines[0] += f"; {got[0][2:]}"
        lines += got[1:]
    shipped = re.search(r"#define YUVBOXGRID_SEG_COLS (\d+)", open(os.path.join(PKG, "csrc", "yuvboxgrid.h")).read()).group(1)
    lines.append(f"the choice: the library ships with YUVBOXGRID_SEG_COLS {shipped} (csrc/yuvboxgrid.h), the width of the least median where three "
                 "composites share a launch; for one composite 1024 and 512 lie within a microsecond of each other")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
