#!/usr/bin/env python3
"""Timing of grid composites through the area-average pass (profiles/box_composite_timing.txt).

The shape: nine 1080p sources laid out for a 160x48 terminal (canvas 160x96, tiles 53x30 in cells 53x32), averaged to the
160x48 image of a truecolor-foreground target, for 9 targets and for 256 targets of equal geometry (every target shares the
nine unique tiles).  HIP events around launches, one at a time (synchronised after each) and four in flight on four streams,
each with buffers of its own (time of a round / launches in it); medians after warm-up.  Recorded per target count:
  * the whole Box.run of the composite batch: the tile launch and the assemble launch;
  * pass 1 alone: the nine 53x30 tiles through the plain-frame API (box_kernel only): the traffic floor;
  * the point-sampled composite plan's truecolor render of the same tick: what opting in is compared with;
  * the truecolor render of the averaged images (Plan over Box.render_frames);
  * for scale, a device-to-device copy of the averaged images.
Inputs are resident before anything is timed.  Every target count runs in a child process of its own under a time limit; the
first that fails ends the run.

    python3 scripts/box_composite_bench.py [--out FILE]        (--targets N: one count, in this process)
"""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from box_downscale_bench import median_us  # noqa: E402

TARGETS = (9, 256)
SRC_W, SRC_H, TERM_W, TERM_H, N_SRC = 1920, 1080, 160, 48, 9


def run_targets(n):
    import torch

    import orc
    from __graft_entry__ import load_package
    pkg = load_package()
    L = pkg.lib()
    assert torch.cuda.is_available() and L.asciichat_hip_device_count() > 0, "no GPU: nothing is measured"
    n_streams = 4
    streams = [torch.cuda.Stream() for _ in range(n_streams)]
    frame_bytes = 3 * SRC_W * SRC_H
    gen = torch.Generator(device="cuda").manual_seed(1)
    srcs = [torch.randint(0, 256, (N_SRC * frame_bytes,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(n_streams)]
    boxes, tiles, images, copies, plans, points, outs, lens, tile_imgs, comp_devs, comps = [], [], [], [], [], [], [], [], [], [], []
    for k in range(n_streams):
        ptrs = [srcs[k].data_ptr() + i * frame_bytes for i in range(N_SRC)]
        comp = pkg.Composite()
        L.achip_composite_setup(C.byref(comp), (C.c_void_p * N_SRC)(*ptrs), (C.c_int * N_SRC)(*[SRC_W] * N_SRC),
                                (C.c_int * N_SRC)(*[SRC_H] * N_SRC), N_SRC, TERM_W, TERM_H)
        assert (comp.canvas_w, comp.canvas_h, comp.n_src) == (TERM_W, 2 * TERM_H, N_SRC)
        tw, th = comp.s[0].tile_w, comp.s[0].tile_h
        comps.append(comp)
        f = pkg.frame_setup(None, comp.canvas_w, comp.canvas_h, TERM_W, TERM_H, 0, False, False, False)
        assert f is not None and (f.out_w, f.out_h) == (TERM_W, TERM_H)
        box = pkg.Box([f] * n, comps=[comp] * n)
        img = torch.zeros(n * box.pitch, dtype=torch.uint8, device="cuda")
        plan = pkg.Plan(pkg.MODE_TRUE_FG, orc.PALETTE_STANDARD, box.render_frames(img.data_ptr()))
        # pass 1 alone: the nine tiles as plain frames
        tile_box = pkg.Box([pkg.frame_setup(p, SRC_W, SRC_H, tw, th, 0, False, False, False) for p in ptrs])
        # the point-sampled composite plan of the same tick
        d = C.c_void_p()
        assert L.asciichat_hip_composite_upload(C.byref(comp), C.byref(d)) == 0 and d.value
        g = pkg.Frame.from_buffer_copy(bytes(f))
        g.comp = d.value
        point = pkg.Plan(pkg.MODE_TRUE_FG, orc.PALETTE_STANDARD, [g] * n)
        stride = max(plan.stride, point.stride)
        boxes.append(box)
        tiles.append(tile_box)
        images.append(img)
        copies.append(torch.zeros_like(img))
        plans.append(plan)
        points.append(point)
        comp_devs.append(d)
        tile_imgs.append(torch.zeros(N_SRC * tile_box.pitch, dtype=torch.uint8, device="cuda"))
        outs.append(torch.zeros(n * stride, dtype=torch.uint8, device="cuda"))
        lens.append(torch.zeros(n, dtype=torch.int32, device="cuda"))
    reps, warm = (50, 10)

    def whole(k):
        boxes[k].run(images[k].data_ptr(), stream=streams[k].cuda_stream)

    def pass1(k):
        tiles[k].run(tile_imgs[k].data_ptr(), stream=streams[k].cuda_stream)

    def point(k):
        points[k].render(outs[k].data_ptr(), points[k].stride, lens[k].data_ptr(), streams[k].cuda_stream)

    def render(k):
        plans[k].render(outs[k].data_ptr(), plans[k].stride, lens[k].data_ptr(), streams[k].cuda_stream)

    def copy(k):
        with torch.cuda.stream(streams[k]):
            copies[k].copy_(images[k], non_blocking=True)

    w1, w4 = median_us(torch, whole, streams, reps, warm)
    t1, t4 = median_us(torch, pass1, streams, reps, warm)
    p1, p4 = median_us(torch, point, streams, reps, warm)
    r1, r4 = median_us(torch, render, streams, reps, warm)
    c1, c4 = median_us(torch, copy, streams, reps, warm)
    img_bytes = n * 3 * TERM_W * TERM_H
    print(f"nine 1080p sources -> {TERM_W}x{TERM_H} x{n}: {N_SRC * frame_bytes / 1e6:.1f} MB of source, tiles {tw}x{th}, "
          f"{img_bytes / 1e6:.2f} MB of averaged images, render geometry {plans[0].variant} (point-sampled composite: {points[0].variant})")
    print(f"  whole Box.run (tiles + assemble)       one at a time {w1:9.1f} us   four in flight {w4:9.1f} us per launch")
    print(f"  pass 1 alone (nine tiles, plain API)   one at a time {t1:9.1f} us   four in flight {t4:9.1f} us per launch")
    print(f"  assemble = whole - pass 1              one at a time {w1 - t1:9.1f} us   four in flight {w4 - t4:9.1f} us per launch")
    print(f"  copy of the averaged images (d2d)      one at a time {c1:9.1f} us   four in flight {c4:9.1f} us per launch")
    print(f"  point-sampled composite render         one at a time {p1:9.1f} us   four in flight {p4:9.1f} us per launch")
    print(f"  render of the averaged images          one at a time {r1:9.1f} us   four in flight {r4:9.1f} us per launch")
    print(f"  opt-in tick (Box.run + render) / point-sampled render: one at a time {(w1 + r1) / p1:.2f}, four in flight {(w4 + r4) / p4:.2f}")
    for k in range(n_streams):
        plans[k].close()
        points[k].close()
        boxes[k].close()
        tiles[k].close()
        L.asciichat_hip_free(comp_devs[k])


def main():
    if "--targets" in sys.argv:
        run_targets(int(sys.argv[sys.argv.index("--targets") + 1]))
        return 0
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    text = ["# grid composites through the area-average pass: scripts/box_composite_bench.py (HIP events, medians; MI355X)"]
    for n in TARGETS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--targets", str(n)], capture_output=True, text=True,
                               timeout=240)
        except subprocess.TimeoutExpired:
            text.append(f"{n} targets: time limit of 240 s reached; nothing further was run")
            break
        text.append(r.stdout.rstrip())
        if r.returncode != 0:
            text.append(f"{n} targets: exit status {r.returncode}; nothing further was run\n{r.stderr[-2000:]}")
            break
    body = "\n".join(text) + "\n"
    sys.stdout.write(body)
    if out:
        with open(out, "w") as f:
            f.write(body)
    return 0 if "nothing further was run" not in body else 1


if __name__ == "__main__":
    sys.exit(main())
