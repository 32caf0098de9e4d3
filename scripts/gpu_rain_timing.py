#!/usr/bin/env python3
"""Timing of the digital rain pass (profiles/rain_timing.txt).

Batch form (asciichat_hip_rain_apply_batch) on 256 frames per launch, HIP events around the launches: one launch at a time
(synchronised after each) and four launches in flight (time of four / 4); median of 30 after 5 warm-up launches.  Each
against its traffic floor: bytes read + written (input, output, the contexts' brightness grids read and written) at
6.3 TB/s.  Drop-in form (digital_rain_apply) per call, median of 50, against the sequential C restatement on one CPU of the
same machine.

    python3 scripts/gpu_rain_timing.py [--out FILE]
"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orc  # noqa: E402
import rain_support as RS  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

HBM = 6.3e12


def slab(pkg, torch, img, cols, rows, mode, n):
    dev = torch.from_numpy(img).cuda()
    frames = [pkg.frame_setup(dev.data_ptr(), img.shape[1], img.shape[0], cols, rows, 0, False, False, False)] * n
    plan = pkg.Plan(mode, orc.PALETTE_STANDARD, frames)
    out = torch.zeros(n * plan.stride, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    plan.render(out.data_ptr(), plan.stride, ln.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    plan.close()
    return out, ln, plan.stride, dev


def batch_case(pkg, torch, label, img, cols, rows, mode, n=256):
    src, ln, stride, _keep = slab(pkg, torch, img, cols, rows, mode, n)
    rains = [pkg.Rain(cols, rows) for _ in range(n)]
    ostride = pkg.Rain.out_stride(stride, cols * rows)
    dst = torch.zeros(n * ostride, dtype=torch.uint8, device="cuda")
    dln = torch.zeros(n, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    dts = [0.016] * n

    def launch():
        rc = pkg.Rain.apply_batch(rains, dts, src.data_ptr(), stride, ln.data_ptr(), dst.data_ptr(), ostride, dln.data_ptr(), s)
        assert rc == 0, pkg.last_error()

    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    one, four = [], []
    for _ in range(30):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        one.append(a.elapsed_time(b) * 1e3)
    for _ in range(30):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(4):
            launch()
        b.record()
        b.synchronize()
        four.append(a.elapsed_time(b) * 1e3 / 4)
    lin = [int(v) & 0xFFFFFFFF for v in ln.cpu().numpy()]
    lout = [int(v) & 0xFFFFFFFF for v in dln.cpu().numpy()]
    assert all(v != RS.LEN_OVERFLOW for v in lout)
    traffic = sum(lin) + sum(lout) + n * cols * rows * 4 * 2
    floor = traffic / HBM * 1e6
    for r in rains:
        r.close()
    m1, m4 = statistics.median(one), statistics.median(four)
    return (f"{label:28s} in {sum(lin) / n / 1e3:7.1f} KB out {sum(lout) / n / 1e3:7.1f} KB per frame; traffic "
            f"{traffic / 1e6:6.1f} MB, floor {floor:6.1f} us | one launch {m1:8.1f} us ({m1 / floor:5.1f}x) | "
            f"four in flight {m4:8.1f} us per launch ({m4 / floor:5.1f}x)")


def dropin_case(pkg, label, img, cols, rows):
    f = orc.convert_with_caps(img, cols, rows, 3, 0)
    g, r = pkg.Rain(cols, rows), RS.Restated(cols, rows)
    gt, ct = [], []
    for k in range(55):
        t0 = time.perf_counter()
        a = g.apply(f, 0.016)
        t1 = time.perf_counter()
        b = r.apply(f, 0.016)
        t2 = time.perf_counter()
        assert a == b
        if k >= 5:
            gt.append((t1 - t0) * 1e6)
            ct.append((t2 - t1) * 1e6)
    g.close()
    r.close()
    return (f"{label:28s} {len(f) / 1e3:7.1f} KB in | digital_rain_apply (GPU) {statistics.median(gt):8.1f} us | "
            f"C restatement, one CPU {statistics.median(ct):8.1f} us")


def main():
    import torch
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})  # the CPU side on one CPU
    pkg = load_package()
    img = orc.frame_smooth(1280, 720)
    img[200:500, 300:900] = orc.frame_hash_noise(600, 300, 3)
    lines = ["# digital rain pass (scripts/gpu_rain_timing.py): medians; floors are estimates at 6.3 TB/s",
             "## batch form, 256 frames per launch, one context per frame"]
    lines.append(batch_case(pkg, torch, "80x24 truecolor fg", img, 80, 24, pkg.MODE_TRUE_FG))
    lines.append(batch_case(pkg, torch, "80x24 mono", img, 80, 24, pkg.MODE_MONO))
    lines.append(batch_case(pkg, torch, "200x60 truecolor fg", img, 200, 60, pkg.MODE_TRUE_FG))
    lines.append("## drop-in form, per call (truecolor fg frames)")
    lines.append(dropin_case(pkg, "80x24", img, 80, 24))
    lines.append(dropin_case(pkg, "200x60", img, 200, 60))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
