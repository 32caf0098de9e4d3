#!/usr/bin/env python3
"""Times libasciichat_pixgrid.so on one GPU: nine 1080p packed sources, BGRA and BGR24, as the 27 tiles of the grid composites at
80x24, 160x48 and 200x60 in one set, beside the only route there was before -- Pix.run_whole of the nine sources into a slab of
whole RGB24 frames, the composites' slots pointing into it.  Three steps per format, each a child process of its own under its
own time limit (a step that fails or runs out of time ends the run: nothing more is started):
  sampled   PixGrid.run against Pix.run_whole, and the tick -- set, the pass, three Plan.render with 256 truecolor-foreground
            targets per size -- both ways;
  averaged  PixGrid.run_box alone, and run_box + asciichat_hip_box_composites over the rewritten descriptors against run_whole +
            asciichat_hip_box_composites over the whole frames, one averaged frame per composite;
  widths    PixGrid.run_box from builds of the library at the four candidate segment widths (no split, 1024, 512, 256; built
            here when missing: make EXTRA=-DPIXGRID_SEG_COLS=N into ascii-chat_amd/build_pixgridN/).
HIP events around every stage, the ways alternating in one run; medians over --launches after --warmup.  The text of the two
ticks, the images of the two averaged routes and the tiles of every width are asserted equal before anything is printed.  A
device-to-device hipMemcpyAsync of the sources' bytes is the traffic's own floor.  Writes the figures, and the width the library
ships with, to --out.  No time is a pass criterion."""
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
FORMATS = {"BGRA": 3, "BGR24": 2}
STEPS = {"sampled": 240, "averaged": 240, "widths": 240}  # seconds a step may take


def variant_path(width):
    return os.path.join(PKG, f"build_pixgrid{width}", "libasciichat_pixgrid.so")


def build_variants():
    """the library at each candidate width, where it is not there yet (two translation units each)"""
    for w in WIDTHS:
        if not os.path.exists(variant_path(w)):
            out = f"build_pixgrid{w}/libasciichat_pixgrid.so"
            subprocess.run(["make", "-C", PKG, f"BUILD=build_pixgrid{w}", f"PIXGRIDOUT={out}", f"EXTRA=-DPIXGRID_SEG_COLS={w}", out], check=True,
                           timeout=600, stdout=subprocess.DEVNULL)


class Bench:
    """the nine sources of one format on the device and what every step needs of them"""

    def __init__(self, fmt_name):
        import torch

        import orc
        from __graft_entry__ import load_package
        from raster_timing import hip_runtime

        self.torch, self.pkg = torch, load_package()
        if not torch.cuda.is_available() or self.pkg.pixgrid_lib().asciichat_pixgrid_device_count() <= 0:
            raise SystemExit("pixgrid_timing: needs a GPU")
        self.hip = hip_runtime()
        self.hip.hipMemcpyAsync.restype = C.c_int
        self.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.stream = torch.cuda.current_stream().cuda_stream
        self.name, fmt = fmt_name, FORMATS[fmt_name]
        bpp = 3 + (fmt & 1)
        rng = np.random.default_rng(11)
        base = orc.frame_smooth(W, H).astype(np.int32)
        host = []
        for k in range(SOURCES):
            px = np.empty((H, W, bpp), dtype=np.uint8)
            px[:, :, :3] = np.clip(np.roll(base, k, axis=2) + rng.integers(-20, 21, (H, W, 1)), 0, 255)
            if bpp == 4:
                px[:, :, 3] = rng.integers(0, 256, (H, W), dtype=np.uint8)
            host.append(px.reshape(-1))
        self.per = host[0].size
        self.pixels = torch.from_numpy(np.stack(host)).cuda()
        self.floor_dst = torch.empty_like(self.pixels)
        self.sources = [self.pkg.pix_source(fmt, W, H, self.pixels.data_ptr() + i * self.per) for i in range(SOURCES)]
        self.whole = self.pkg.Pix(SOURCES)
        self.whole.set(self.sources, None, stream=self.stream)
        self.pitch = self.whole.whole_pitch
        self.rgb = torch.empty(SOURCES * self.pitch, dtype=torch.uint8, device="cuda")
        self.comps = []
        for tw, th in SIZES:  # achip_composite_setup's descriptors over the whole frames
            c = self.pkg.Composite()
            ptrs = (C.c_void_p * SOURCES)(*[self.rgb.data_ptr() + i * self.pitch for i in range(SOURCES)])
            self.pkg.lib().achip_composite_setup(C.byref(c), ptrs, (C.c_int * SOURCES)(*[W] * SOURCES), (C.c_int * SOURCES)(*[H] * SOURCES), SOURCES, tw, th)
            assert c.n_src == SOURCES and all(c.s[k].src for k in range(SOURCES))
            self.comps.append(c)
        self.per_comp = [self.sources] * len(SIZES)

    def head(self, what):
        return (f"{self.name}: {SOURCES} sources of {W}x{H} ({SOURCES * self.per / 1e6:.0f} MB), composites at {', '.join('%dx%d' % s for s in SIZES)} in one "
                f"set ({len(SIZES) * SOURCES} tiles); the old route's slab of whole frames: {self.rgb.numel() / 1e6:.0f} MB, the tile passes need none; {what}")

    def run_whole(self):
        self.whole.run_whole(self.rgb.data_ptr(), self.pitch, stream=self.stream)

    def memcpy(self):
        rc = self.hip.hipMemcpyAsync(self.floor_dst.data_ptr(), self.pixels.data_ptr(), SOURCES * self.per, 3, self.stream)
        if rc != 0:
            raise RuntimeError(f"hipMemcpyAsync failed ({rc})")


def rows(t, moved=0):
    out = []
    for k, v in t.items():
        note = f"   {moved / statistics.median(v) / 1e6:.2f} TB/s read (and as much written)" if k.startswith("memcpy") else ""
        out.append(f"  {k:<52} median {statistics.median(v):9.1f} us   least {min(v):9.1f} us{note}")
    return out


def sampled(b, args):
    from yuv_timing import timed
    import orc
    torch, pkg, stream, L, N = b.torch, b.pkg, b.stream, b.pkg.lib(), args.targets
    grid = pkg.PixGrid(len(SIZES) * SOURCES)
    grid.set(b.comps, b.per_comp, stream=stream)
    tiles = torch.empty(grid.tiles_bytes(), dtype=torch.uint8, device="cuda")
    rewritten = grid.composites(tiles.data_ptr())

    def upload(c):
        d = C.c_void_p()
        if L.asciichat_hip_composite_upload(C.byref(c), C.byref(d)) != 0:
            raise RuntimeError("composite_upload failed: " + pkg.last_error())
        return d

    ways = {}
    for name, descs in (("tiles", rewritten), ("whole", b.comps)):
        devs = [upload(c) for c in descs]
        plans = []
        for (tw, th), d in zip(SIZES, devs):
            f = pkg.frame_setup(None, tw, 2 * th, tw, th, 0, True, True, False)
            f.comp = d.value
            plans.append(pkg.Plan(pkg.MODE_TRUE_FG, orc.PALETTE_STANDARD, [f] * N))
        ways[name] = (devs, plans, [torch.zeros(N * p.stride, dtype=torch.uint8, device="cuda") for p in plans],
                      [torch.zeros(N, dtype=torch.int32, device="cuda") for _ in plans])

    def renders(name):
        _, plans, text, lens = ways[name]
        for p, t, n in zip(plans, text, lens):
            p.render(t.data_ptr(), p.stride, n.data_ptr(), stream)

    def run_tiles():
        grid.run(tiles.data_ptr(), stream=stream)

    def tick_tiles():
        grid.set(b.comps, b.per_comp, stream=stream)
        run_tiles()
        renders("tiles")

    def tick_whole():
        b.whole.set(b.sources, None, stream=stream)
        b.run_whole()
        renders("whole")

    tick_tiles()
    tick_whole()
    torch.cuda.synchronize()
    for i, size in enumerate(SIZES):
        la, lb = ways["tiles"][3][i].cpu().numpy(), ways["whole"][3][i].cpu().numpy()
        stride = ways["tiles"][1][i].stride
        ta, tb = ways["tiles"][2][i].cpu().numpy().reshape(N, stride), ways["whole"][2][i].cpu().numpy().reshape(N, stride)
        assert np.array_equal(la, lb) and la.min() > size[0] * size[1], f"{size}: the two ways' lengths differ"
        assert all(np.array_equal(ta[k, :la[k]], tb[k, :la[k]]) for k in range(N)), f"{size}: the two ways' text differs"
    t = timed({"pixgrid_run (27 tiles)": run_tiles, "pix_run_whole (9 x 1080p)": b.run_whole, "memcpy D2D of the sources": b.memcpy}, args.launches, args.warmup)
    t.update(timed({"tick: set + pixgrid_run + renders": tick_tiles, "tick: set + pix_run_whole + renders": tick_whole}, args.launches, args.warmup))
    lines = [b.head(f"sampled tiles, {N} truecolor-foreground targets per size; both ways' text equal")] + rows(t, SOURCES * b.per)
    med = {k: statistics.median(v) for k, v in t.items()}
    lines.append(f"  the pass against the conversion it replaces: {med['pix_run_whole (9 x 1080p)'] / med['pixgrid_run (27 tiles)']:.2f} x; the tick: "
                 f"{med['tick: set + pix_run_whole + renders'] / med['tick: set + pixgrid_run + renders']:.2f} x")
    for devs, plans, _, _ in ways.values():
        for p in plans:
            p.close()
        for d in devs:
            L.asciichat_hip_free(d)
    grid.close()
    return lines


def averaged(b, args):
    from yuv_timing import timed
    torch, pkg, stream = b.torch, b.pkg, b.stream
    grid = pkg.PixGrid(len(SIZES) * SOURCES)
    grid.set(b.comps, b.per_comp, stream=stream)
    tiles = torch.full((grid.tiles_bytes(),), 0xA5, dtype=torch.uint8, device="cuda")
    rewritten = grid.composites(tiles.data_ptr())
    frames = []
    for c, (tw, th) in zip(b.comps, SIZES):  # a composite frame averaged to the terminal's size: the canvas as its source
        f = pkg.Frame()
        f.src_w, f.src_h, f.out_w, f.out_h = c.canvas_w, c.canvas_h, tw, th
        f.x_ratio, f.y_ratio = (c.canvas_w << 16) // tw + 1, (c.canvas_h << 16) // th + 1
        frames.append(f)
    boxes = [pkg.Box(frames, comps=b.comps, stream=stream), pkg.Box(frames, comps=rewritten, stream=stream)]
    assert boxes[0].pitch == boxes[1].pitch
    images = [torch.full((len(frames) * boxes[0].pitch,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]

    def box_old():
        boxes[0].run(images[0].data_ptr(), stream=stream)

    def box_new():
        boxes[1].run(images[1].data_ptr(), stream=stream)

    def tiles_run():
        grid.run_box(tiles.data_ptr(), stream=stream)

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
    assert int((images[1] != 0xA5).sum().item()) > sum(3 * tw * th for tw, th in SIZES) // 2, "nothing was stored"
    t = timed({"pixgrid_run_box (27 tiles)": tiles_run, "pix_run_whole (9 x 1080p)": b.run_whole, "box_composites over whole frames": box_old,
               "box_composites over the averaged tiles": box_new, "old route: pix_run_whole + box_composites": old_route,
               "new route: pixgrid_run_box + box_composites": new_route, "memcpy D2D of the sources": b.memcpy}, args.launches, args.warmup)
    lines = [b.head("averaged tiles, one averaged frame per composite; the two routes' images equal")] + rows(t, SOURCES * b.per)
    med = {k: statistics.median(v) for k, v in t.items()}
    lines.append(f"  the new route against the old: {med['old route: pix_run_whole + box_composites'] / med['new route: pixgrid_run_box + box_composites']:.2f} x")
    for x in boxes:
        x.close()
    grid.close()
    return lines


def widths(b, args):
    from yuv_timing import timed
    torch, pkg, stream = b.torch, b.pkg, b.stream
    grids, slabs, fns = [], [], {}
    for w in WIDTHS:
        g = pkg.PixGrid(len(SIZES) * SOURCES, lib=pkg.pixgrid_lib(variant_path(w)))
        g.set(b.comps, b.per_comp, stream=stream)
        slab = torch.full((g.tiles_bytes(),), 0xA5, dtype=torch.uint8, device="cuda")
        grids.append(g)
        slabs.append(slab)
        fns[f"pixgrid_run_box, segment width {w if w else 'none (no split)'}"] = (lambda g=g, slab=slab: g.run_box(slab.data_ptr(), stream=stream))
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    assert all(torch.equal(slabs[0], s) for s in slabs[1:]), "the widths' tiles differ"
    assert int((slabs[0] != 0xA5).sum().item()) > slabs[0].numel() // 2, "nothing was stored"
    t = timed(fns, args.launches, args.warmup)
    med = {k: statistics.median(v) for k, v in t.items()}
    lines = [b.head("the segment width of run_box, one build of the library per width (the tiles of all four equal)")] + rows(t)
    lines.append(f"  least median: {min(med, key=med.get)}")
    for g in grids:
        g.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixgrid_timing.txt"))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--targets", type=int, default=256, help="targets per size of the tick (a rehearsal may take fewer)")
    ap.add_argument("--step", choices=list(STEPS), help="run this step alone, in this process, and print its lines")
    ap.add_argument("--format", choices=list(FORMATS), default="BGRA")
    args = ap.parse_args()
    if args.step:
        b = Bench(args.format)
        lines = {"sampled": sampled, "averaged": averaged, "widths": widths}[args.step](b, args)
        print("\n".join([f"# {b.torch.cuda.get_device_name(0)}"] + lines))
        return
    build_variants()
    lines = [f"# Packed RGB sources as grid tiles: scripts/pixgrid_timing.py (HIP events around every stage, the ways alternating; medians of "
             f"{args.launches} launches after {args.warmup} warm-ups; each step a process of its own)"]
    for fmt in FORMATS:
        for step, limit in STEPS.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--format", fmt, "--launches", str(args.launches), "--warmup", str(args.warmup),
                   "--targets", str(args.targets)]
            try:
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"pixgrid_timing: step {step} ({fmt}) ran out of its {limit} s: nothing more is started")
            if out.returncode != 0:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                raise SystemExit(f"pixgrid_timing: step {step} ({fmt}) ended with {out.returncode}: nothing more is started")
            got = out.stdout.strip().splitlines()
            if len(lines) == 1:
                lines[0] += f"; {got[0][2:]}"
            lines += got[1:]
    shipped = re.search(r"#define PIXGRID_SEG_COLS (\d+)", open(os.path.join(PKG, "csrc", "pixgrid.h")).read()).group(1)
    lines.append(f"the library ships with PIXGRID_SEG_COLS {shipped} (csrc/pixgrid.h)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
