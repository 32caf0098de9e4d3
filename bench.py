#!/usr/bin/env python3
"""bench.py -- frames/s of the MI355X render path on BASELINE.json's metric.

A "step" is one pass of the hot path (one kernel launch through the C-ABI) over one batch of 256 device-resident
synthetic frames.  Default workload = the configuration the metric is quoted on: 1080p -> 80x24 truecolor foreground
(BASELINE.json `metric`; `configs[1]` is the same shape in ANSI-256 and is reported under "other_workloads" with the
other configs).  One process per GPU; frames are independent, so N > 1 shards the batch across ranks with no
data-path collective (weak scaling: 256 frames per rank and step).

Protocol (VERDICT r1 "next round" 1-2):
  * the K steps of a timed region are issued from C (asciichat_hip_render_many) round-robin over S independent
    batches on separate HIP streams -- the reference's model is one render thread per client
    (src/server/render.c:1233) -- and drained with a spin wait; barrier + torch.cuda.synchronize() on both sides;
    S (`--streams`, default 0 = automatic) is picked for the burst length K in an untimed calibration: a queue that
    went idle at the synchronize takes ~20 us to wake up, so short regions want fewer launches in flight than the
    steady state does (profiles/r02_region_overhead.txt); the calibration's numbers are in the line;
  * the timed steps are exactly `--steps` K: one region of K steps, whose wall time over K is `ms_per_step`
    (`--regions R` repeats the region R times and takes the MEDIAN region, for profiling runs);
  * a fresh input batch every step (12 batches rotate: no step re-reads the previous step's frames out of the 256 MB
    Infinity Cache);
  * everything in the line was measured by this run, except what sits under "committed_profile" (rocprofv3 summaries
    from profiles/, labelled with their source).

A plain run does only what the headline needs: it sets up, calibrates S, warms up, times the steps, writes
`--dump-outputs` if asked and prints the line.  `--full` adds everything else this file measures or checks:
  * `roofline.kernel_ms` = GPU time per step from HIP events recorded on the launch streams around a long
    back-to-back run of the same schedule; `roofline.achieved` = algorithmic bytes per launch / kernel_ms;
  * after timing, 8 frames per workload are compared byte-for-byte with the CPU oracle on the very same input frames;
  * one launch at a time, the PCIe-inclusive, wire-stage and server-tick legs, the CPU baseline, the other workloads
    (`--others`), the batch-size axis (`--batch-sweep`) and, for N > 1, the all-gather of the rendered frames.

Prints ONE compact JSON line on rank 0 (< 4 KB: the contract's keys, with --full also roofline + cpu_baseline + verify + a
digest of the other workloads); the full record of the run -- every leg, table and note -- goes to the side file `--extra`
(default bench_extra.json next to this script).
"""
import argparse
import ctypes as C
import json
import math
import os
import platform
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PALETTE_STANDARD = "   ...',;:clodxkO0KXNWM"  # PALETTE_CHARS_STANDARD (palette.h:161)
MULTI_LEG_TIMEOUT_S = 180  # the optional all-gather leg of an N > 1 run (after the timing line is complete)
HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: 8.0 TB/s spec

WORKLOADS = {
    # name: (src_w, src_h, W, H, color_level, render_mode)
    "1080p_80x24_truecolor": (1920, 1080, 80, 24, 3, 0),  # the metric's shape
    "1080p_80x24_ansi256": (1920, 1080, 80, 24, 2, 0),    # configs[1] (K2)
    "4k_200x60_truecolor": (3840, 2160, 200, 60, 3, 0),   # configs[2] (K3)
    "4k_400x120_halfblock": (3840, 2160, 400, 120, 3, 2),  # configs[4] (K5)
    "1080p_80x24_halfblock": (1920, 1080, 80, 24, 3, 2),   # the metric's shape in half blocks (fg + bg per cell)
    "640x480_80x24_mono": (640, 480, 80, 24, 0, 0),       # configs[0] (K1)
    # what a server tick renders after the sampled-image ingest (frame_dense.c): the source IS the 80x24 image the target
    # samples of the client's 1080p frame, ratios 1.0 -- 5.6 KB of dense reads per frame instead of 1 920 lone dwords
    "sampled_80x24_truecolor": (80, 24, 80, 24, 3, 0),
    # configs[2] / configs[4] from sampled images: the kernels where HBM line fills are NOT the limit
    "sampled_200x60_truecolor": (200, 60, 200, 60, 3, 0),
    "sampled_400x240_halfblock": (400, 240, 400, 120, 3, 2),
    # truecolor foreground with the reference's multi-byte palettes (palette.h:161-197; three of its five built-ins take
    # foreground.c:281-296's branch): round 6's instantiation of the stream kernel
    "1080p_80x24_truecolor_blocks": (1920, 1080, 80, 24, 3, 0),
    "4k_200x60_truecolor_cool": (3840, 2160, 200, 60, 3, 0),
    "sampled_200x60_truecolor_blocks": (200, 60, 200, 60, 3, 0),
    # rows wider than one block of the rows kernel (448 cells): ascii.c:204 admits terminals up to 10 000 columns, and 4K ->
    # 640x180 half blocks is a plain use: the rows kernel's segment geometries (render_rows.hpp WIDE)
    "4k_640x180_halfblock": (3840, 2160, 640, 180, 3, 2),
    "sampled_640x360_halfblock": (640, 360, 640, 180, 3, 2),
    # the two renderers of SURVEY 8(a) no other leg reaches at the metric's shape: monochrome frames in a batch (PM, rows kernel)
    # and the serial Floyd-Steinberg 16-colour background renderer (PD: TRUECOLOR + BACKGROUND, sgr.c:429) -- one wave per frame
    # on the phase kernel; plain legs only (no aspect + padding variant)
    "1080p_80x24_mono": (1920, 1080, 80, 24, 0, 0),
    "1080p_80x24_dither16_bg": (1920, 1080, 80, 24, 3, 1),
}
PLAIN_ONLY_WORKLOADS = ("1080p_80x24_mono", "1080p_80x24_dither16_bg")
# the 16-colour renderers (P16, H16) beside them: named workloads for A/B runs (scripts/gpu_abn.sh), not part of the default run
WORKLOADS.update({"1080p_80x24_ansi16": (1920, 1080, 80, 24, 1, 0), "sampled_200x60_ansi16": (200, 60, 200, 60, 1, 0),
                  "1080p_80x24_halfblock16": (1920, 1080, 80, 24, 1, 2), "sampled_400x240_halfblock16": (400, 240, 400, 120, 1, 2)})
ON_REQUEST_WORKLOADS = ("1080p_80x24_ansi16", "sampled_200x60_ansi16", "1080p_80x24_halfblock16", "sampled_400x240_halfblock16")
# the wide-row workloads: part of the default run since round 6 (the rows kernel's segment geometries: 350-400 us per launch;
# on the phase kernel they were 600 us of 1 GB each), but not with aspect + padding on top (4K sources twice more)
HEAVY_WORKLOADS = ("4k_640x180_halfblock", "sampled_640x360_halfblock")
PALETTE_BLOCKS = "   \u2591\u2591\u2592\u2592\u2593\u2593\u2588\u2588"  # PALETTE_CHARS_BLOCKS (palette.h)
PALETTE_COOL = "   \u2581\u2582\u2583\u2584\u2585\u2586\u2587\u2588"    # PALETTE_CHARS_COOL
WORKLOAD_PALETTE = {"1080p_80x24_truecolor_blocks": PALETTE_BLOCKS, "4k_200x60_truecolor_cool": PALETTE_COOL,
                    "sampled_200x60_truecolor_blocks": PALETTE_BLOCKS}


def palette_of(name):
    return WORKLOAD_PALETTE.get(name, PALETTE_STANDARD)
# batch-size axis: the 1-GPU stand-in for a scaling curve -- where each kernel saturates
SWEEP_WORKLOADS = ("1080p_80x24_truecolor", "4k_200x60_truecolor", "sampled_80x24_truecolor", "sampled_200x60_truecolor",
                   "sampled_400x240_halfblock")
SWEEP_MAX_SET_BYTES = 110e9  # one input set of the largest point (4096 x 4K RGB24 = 102 GB of the 288 GB HBM)
INPUT_KINDS = ("noise", "smooth", "bars", "gray")


def make_frames(torch, batch, w, h, seed, kind="noise"):
    """Device-resident synthetic inputs of SURVEY 8(d).  noise: uniform random RGB24 (every cell changes colour, no
    runs -- the worst case for output size); smooth / bars / gray: the formulas of tests/orc.py frame_smooth /
    frame_bars (phase = frame index / 2) / frame_gray, evaluated on the device."""
    if kind == "noise":
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        return torch.randint(0, 256, (batch, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)
    x = torch.arange(w, device="cuda", dtype=torch.int64)[None, None, :]
    y = torch.arange(h, device="cuda", dtype=torch.int64)[None, :, None]
    out = torch.empty((batch, h, w, 3), dtype=torch.uint8, device="cuda")
    if kind == "smooth":
        out[..., 0] = (x * 255 // max(1, w - 1)).to(torch.uint8)
        out[..., 1] = (y * 255 // max(1, h - 1)).to(torch.uint8)
        out[..., 2] = ((((x // 64) + (y // 64)) * 32) & 0xFF).to(torch.uint8)
    elif kind == "bars":
        bar, rowgap = max(1, w // 8), max(1, h // 8)
        phase = (torch.arange(batch, device="cuda", dtype=torch.int64) + seed % 1000)[:, None, None] // 2
        ax = (x + phase) % w
        sel = (ax // bar) % 3
        grid = (ax % bar == 0) | (y % rowgap == 0)
        for c in range(3):
            out[..., c] = torch.where((sel == c) & ~grid, 255, 0).to(torch.uint8)
    elif kind == "gray":
        i = (y * w + x)
        gch = (i * 255 // (w * h)).to(torch.uint8)
        for c in range(3):
            out[..., c] = gch
    else:
        raise ValueError(kind)
    return out


def build_plan(pkg, frames_t, W, H, cl, rm, aspect=False, palette=PALETTE_STANDARD):
    """aspect=False: full W x H (SURVEY 8(d) first variant); aspect=True: use_aspect_ratio + wants_padding, the
    server's call (stream.c:841)."""
    b, h, w, _ = frames_t.shape
    mode = pkg.lib().achip_mode_from_caps(cl, rm)
    base = frames_t.data_ptr()
    descs = [pkg.frame_setup(base + i * h * w * 3, w, h, W, H, rm, aspect, aspect, False) for i in range(b)]
    return pkg.Plan(mode, palette, descs), mode


_LANE_POOL = []


class Runner:
    """P plans (independent input batches) rendered round-robin on S streams through asciichat_hip_render_many."""

    def __init__(self, torch, pkg, plans, batch, streams):
        self.torch, self.pkg, self.plans, self.batch = torch, pkg, plans, batch
        self.S = streams
        self.cur = torch.cuda.current_stream()
        # ONE pool of streams for the whole process: HIP maps streams onto a handful of hardware queues round-robin, so
        # every extra stream object ever created shifts the mapping and two "independent" lanes can end up sharing a
        # queue (measured: 8.7 -> 10.8 us per step after a calibration pass had created its own streams)
        while len(_LANE_POOL) < streams - 1:
            _LANE_POOL.append(torch.cuda.Stream())
        self.lanes = [self.cur] + _LANE_POOL[:streams - 1]
        self.stride = plans[0].stride
        self.outs = [torch.empty(batch * self.stride, dtype=torch.uint8, device="cuda") for _ in range(streams)]
        self.lns = [torch.zeros(batch, dtype=torch.int32, device="cuda") for _ in range(streams)]
        self.sched = pkg.Schedule(plans, [o.data_ptr() for o in self.outs], [l.data_ptr() for l in self.lns],
                                  self.stride, [s.cuda_stream for s in self.lanes])
        self.step = 0

    def issue(self, n):
        self.sched.issue(self.step, n)
        self.step += n

    def region(self, K, dist=None):
        """EXACTLY K steps, barrier + synchronize on both sides; returns THIS rank's wall seconds from the opening
        bracket to the completion of its own K steps (the caller takes the MAX over ranks of every region: the time the
        slowest rank needed; the closing barrier's own latency is not a step and is not counted)."""
        torch = self.torch
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.issue(K)
        self.sched.wait()  # spin on hipStreamQuery: no driver sleep in a ~170 us region
        torch.cuda.synchronize()
        t1 = time.perf_counter()  # this rank's K steps are done; the MAX over ranks is taken by the caller
        if dist is not None:  # closing bracket: nobody starts the next region before everybody has finished this one
            dist.barrier()
            torch.cuda.synchronize()
        return t1 - t0

    def gpu_ms_per_step(self, n):
        """GPU time per step over n back-to-back steps: HIP events on every launch stream, first begin -> last end."""
        torch = self.torch
        torch.cuda.synchronize()
        b = [torch.cuda.Event(enable_timing=True) for _ in range(self.S)]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(self.S)]
        self.issue(self.S)  # streams busy: the begin events complete when these kernels end, not at record time
        for s in range(self.S):
            b[s].record(self.lanes[s])
        self.issue(n)
        for s in range(self.S):
            e[s].record(self.lanes[s])
        torch.cuda.synchronize()
        return max(b[s].elapsed_time(e[t]) for s in range(self.S) for t in range(self.S)) / n


def verify_against_oracle(torch, pkg, plan, frames_t, W, H, cl, rm, aspect, n_check=8, palette=PALETTE_STANDARD):
    """Renders the batch once more (untimed) and compares n_check frames byte-for-byte with the CPU oracle run on the
    very same input frames (downloaded from the device).  Raises on any difference."""
    import numpy as np

    import orc

    b = frames_t.shape[0]
    out = torch.zeros(b * plan.stride, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(b, dtype=torch.int32, device="cuda")
    plan.render(out.data_ptr(), plan.stride, ln.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    lens = ln.cpu().numpy().astype("uint32")
    assert (lens < 0xFFFFFFF0).all(), "kernel reported overflow / bad descriptor"
    idx = sorted(set(int(round(i * (b - 1) / max(1, n_check - 1))) for i in range(min(n_check, b))))
    for i in idx:
        img = np.ascontiguousarray(frames_t[i].cpu().numpy())
        exp = orc.convert_with_caps(img, W, H, cl, rm, aspect, aspect, False, palette)
        got = bytes(out[i * plan.stride:i * plan.stride + int(lens[i])].cpu().numpy())
        if got != exp:
            raise SystemExit(f"bench.py: output of frame {i} differs from the oracle ({len(got)} vs {len(exp)} bytes)")
    return {"frames_checked": len(idx), "byte_identical_to_oracle": True}, lens


def run_workload(torch, pkg, name, batch, steps, warmup, regions, dist=None, seed=1234, variant=-1, nsets=12,
                 streams=4, kind="noise", aspect=False, serial_leg=True, verify=True, streams_auto=None, keep_last=False,
                 roofline=True):
    """Sets up, calibrates the launches in flight (streams_auto), warms up and times `regions` regions of `steps` steps.
    verify, roofline and serial_leg add the legs of a --full run: the oracle comparison, the passes the roofline needs
    (exact output bytes of every input set, HIP-event kernel time) and the one-launch-at-a-time leg."""
    sw, sh, W, H, cl, rm = WORKLOADS[name]
    assert nsets % streams == 0 and all(nsets % c == 0 for c in (streams_auto or ()))
    sets = [make_frames(torch, batch, sw, sh, seed + 7919 * s, kind) for s in range(nsets)]
    plans = []
    for t in sets:
        plan, mode = build_plan(pkg, t, W, H, cl, rm, aspect, palette_of(name))
        plan.set_concurrency(streams)
        if variant >= 0:
            plan.set_variant(variant)
        plans.append(plan)
    tune = None
    if streams_auto and batch > 1:
        # launches in flight for THIS burst length: a queue that has gone idle takes ~20 us to wake up, so a short
        # region is better served by fewer streams than the steady state is (profiles/r02_region_overhead.txt)
        tune = {}
        for cand in streams_auto:
            for plan in plans:
                plan.set_concurrency(cand)
                if variant >= 0:
                    plan.set_variant(variant)
            r = Runner(torch, pkg, plans, batch, cand)
            r.issue(24)
            torch.cuda.synchronize()
            tune[cand] = statistics.median(r.region(steps, None) for _ in range(9)) / steps * 1e3
            r.sched.close()
        streams = min(tune, key=tune.get)
        for plan in plans:
            plan.set_concurrency(streams)
            if variant >= 0:
                plan.set_variant(variant)
    run = Runner(torch, pkg, plans, batch, streams)
    ver, lens = (verify_against_oracle(torch, pkg, plans[0], sets[0], W, H, cl, rm, aspect, palette=palette_of(name)) if verify
                 else (None, None))
    # exact output bytes of every input set (B_alg = sampled RGB consumed + exact output length)
    out_bytes = []
    for g in range(0, nsets, streams) if roofline else ():
        run.step = g
        run.issue(streams)
        torch.cuda.synchronize()
        for s in range(streams):
            l = run.lns[s].cpu().numpy().astype("uint32")
            assert (l < 0xFFFFFFF0).all(), "kernel reported overflow / bad descriptor"
            out_bytes.append(int(l.sum()))
    run.step = 0
    run.issue(warmup)
    torch.cuda.synchronize()
    walls = [run.region(steps, dist) for _ in range(regions)]
    last = None
    if keep_last:  # the timed regions' last step k rendered plans[k % nsets] into lane k % streams (region() synchronised)
        k = run.step - 1
        last = {"slab": run.outs[k % streams].cpu().numpy(), "lens": run.lns[k % streams].cpu().numpy().astype("uint32"),
                "stride": run.stride}
    gpu_ms = out_mean = alg_bytes = None
    f0 = pkg.frame_setup(sets[0].data_ptr(), sw, sh, W, H, rm, aspect, aspect, False)
    if roofline:
        gpu_ms = run.gpu_ms_per_step(max(200, steps))
        cells_px = f0.out_w * f0.out_h  # sampled pixels per frame (2 rows per text row in half-block)
        out_mean = sum(out_bytes) / len(out_bytes)
        alg_bytes = int(out_mean) + batch * 3 * cells_px
    res = dict(name=name, mode=pkg.MODE_NAMES[mode], batch=batch, walls=walls, steps=steps, gpu_ms=gpu_ms,
               out_bytes_per_frame=out_mean / batch if roofline else None, alg_bytes_per_launch=alg_bytes, variant=plans[0].variant,
               input_sets=nsets, streams=streams, kind=kind, aspect=aspect, verify=ver, streams_autotune=tune,
               cells_per_frame=(f0.pad_left + f0.out_w) * ((f0.out_h + 1) // 2 if rm == 2 else f0.out_h),
               serial=None, plans=plans, sets=sets, forced_variant=variant, last=last)
    if serial_leg:
        # the same steps one launch at a time (each plan re-chooses its geometry for the whole GPU), and the same
        # batch rendered every step (its sampled lines then come out of the Infinity Cache)
        for plan in plans:
            plan.set_concurrency(1)
            if variant >= 0:
                plan.set_variant(variant)
        one = Runner(torch, pkg, plans, batch, 1)
        one.issue(8)
        g1 = one.gpu_ms_per_step(max(100, steps))
        w1 = statistics.median(one.region(steps, None) for _ in range(max(3, regions // 3)))
        same = Runner(torch, pkg, plans[:1], batch, 1)
        same.issue(8)
        gs = same.gpu_ms_per_step(max(100, steps))
        res["serial"] = {"kernel_ms": g1, "ms_per_step_wall": w1 / steps * 1e3, "frames_per_s": batch / (g1 * 1e-3),
                         "kernel_variant": plans[0].variant, "kernel_ms_same_batch_every_step": gs,
                         "roofline_frac": alg_bytes / (g1 * 1e-3) / 1e9 / HBM_PEAK_GBS}
    return res


def summarize(res, world=1, wall=None):
    """Per-workload entry of the JSON line (everything measured by this run)."""
    wall = statistics.median(res["walls"]) if wall is None else wall
    fps = res["batch"] * res["steps"] * world / wall
    d = {"frames_per_s": fps, "ms_per_step": wall / res["steps"] * 1e3, "launches_in_flight": res["streams"],
         "region_ms": {"min": min(res["walls"]) * 1e3, "median": statistics.median(res["walls"]) * 1e3,
                       "max": max(res["walls"]) * 1e3, "regions": len(res["walls"]), "steps_per_region": res["steps"]},
         "input": res["kind"], "aspect_and_padding": res["aspect"], "mode": res["mode"],
         "cells_per_s": res["cells_per_frame"] * fps, "kernel_variant": res["variant"], "input_sets": res["input_sets"]}
    k = res["gpu_ms"]
    if k is not None:  # the roofline passes ran
        a = res["alg_bytes_per_launch"] / (k * 1e-3) / 1e9
        d.update({"kernel_ms": k, "out_bytes_per_frame": res["out_bytes_per_frame"],
                  "alg_bytes_per_launch": res["alg_bytes_per_launch"], "output_GBps": res["out_bytes_per_frame"] * fps / 1e9,
                  "roofline_GBps": a, "roofline_frac": a / HBM_PEAK_GBS})
    if res["verify"] is not None:
        d["verify"] = res["verify"]
    if res.get("streams_autotune"):
        d["launches_in_flight_autotune_ms_per_step"] = {str(k): v for k, v in res["streams_autotune"].items()}
    if res["serial"] is not None:
        d["one_launch_at_a_time"] = res["serial"]
    return d


def free_workload(torch, res):
    for p in res.pop("plans", []):
        p.close()
    res.pop("sets", None)
    torch.cuda.empty_cache()


def batch_sweep(torch, pkg, batches, names=SWEEP_WORKLOADS, streams=4):
    """frames/s and roofline fraction over the batch size (frames per launch): every BASELINE number is quoted at 256
    frames = one workgroup per CU = ONE wave of workgroups; larger launches show the kernels' asymptotic rate.  Input
    sets shrink with the batch so that a point's sources stay below SWEEP_MAX_SET_BYTES in total."""
    out = {}
    for name in names:
        sw, sh = WORKLOADS[name][:2]
        row = {}
        for b in batches:
            set_bytes = b * sw * sh * 3
            if set_bytes > SWEEP_MAX_SET_BYTES:
                row[str(b)] = {"skipped": f"one input set would be {set_bytes / 1e9:.0f} GB"}
                continue
            nsets = streams * max(1, min(3, int(SWEEP_MAX_SET_BYTES // (streams * set_bytes))))
            if nsets * set_bytes > SWEEP_MAX_SET_BYTES:
                nsets, st = 1, 1
            else:
                st = streams
            steps = max(4, min(40, 40 * 256 // b))
            t_w = time.perf_counter()
            try:
                r = run_workload(torch, pkg, name, b, steps, 4, 5, None, nsets=nsets, streams=st, serial_leg=False,
                                 verify=(b == batches[0]))
            except (RuntimeError, AssertionError) as e:
                row[str(b)] = {"error": str(e)[:160]}
                torch.cuda.empty_cache()
                continue
            d = summarize(r)
            row[str(b)] = {"frames_per_s": d["frames_per_s"], "kernel_ms": d["kernel_ms"], "roofline_frac": d["roofline_frac"],
                           "roofline_GBps": d["roofline_GBps"], "launches_in_flight": st, "input_sets": nsets,
                           "steps_per_region": steps, "kernel_variant": d["kernel_variant"],
                           "alg_bytes_per_launch": d["alg_bytes_per_launch"]}
            free_workload(torch, r)
            print(f"[bench] sweep {name} batch {b}: {time.perf_counter() - t_w:.1f} s", file=sys.stderr)
        out[name] = row
    return out


def time_with_d2h(torch, plan, n, steps):
    """the same steps with the output copied to pinned host memory after every launch -- slab and
    lengths share one allocation so that they cross PCIe in ONE transfer.  The PCIe-inclusive rate, never `value`."""
    stream = torch.cuda.current_stream().cuda_stream
    slab = n * plan.stride
    buf = torch.empty(slab + 4 * n, dtype=torch.uint8, device="cuda")
    host = torch.empty(buf.shape, dtype=buf.dtype, pin_memory=True)
    out_ptr, len_ptr = buf.data_ptr(), buf.data_ptr() + slab

    def step():
        plan.render(out_ptr, plan.stride, len_ptr, stream)
        host.copy_(buf, non_blocking=True)

    for _ in range(30):  # the first transfers into a fresh pinned block are slow
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, int(buf.numel())


def run_grid9(torch, pkg, steps, regions, targets=256, dist=None, world=1, rank=0, backend="nccl", last=None, full=True):
    """BASELINE configs[3]: nine 1080p sources -> the 3x3 grid at 160x48 (stream.c:523-854), sharded over the ranks
    with an RCCL all-gather for the composite -- through the C-ABI (asciichat_hip_comm_* / asciichat_hip_grid_*):
    a step = every rank resizes the sources it owns into their tiles, ONE ncclAllGather moves the tiles to every rank,
    and every rank renders the grid for its `targets` target clients (the server renders the mixed frame once per
    connected client, render.c:340-600) straight from the gathered tiles -- the W x 2H canvas stays virtual.  The
    exchange is inside the timed step.  World size 1 still runs the real ncclAllGather.  `last` (a dict): filled with
    the output of the last timed step of the `targets` leg (the one the line reports)."""
    import numpy as np

    import orc

    n, sw, sh, tw, th = 9, 1920, 1080, 160, 48
    comm = None
    if backend == "nccl":
        if world > 1:
            uid = torch.zeros(pkg.COMM_ID_BYTES, dtype=torch.uint8, device="cuda")
            if rank == 0:
                uid.copy_(torch.frombuffer(bytearray(pkg.comm_unique_id()), dtype=torch.uint8))
            dist.broadcast(uid, 0)
            comm = pkg.Comm(world, rank, bytes(uid.cpu().numpy()))
        else:
            comm = pkg.Comm(1, 0, pkg.comm_unique_id())
    grid = pkg.Grid(comm, [(sw, sh)] * n, tw, th)
    # every rank generates the sources it owns (same seeds on every rank: source k is the same frame everywhere)
    own = [k for k in range(n) if grid.owner(k) == (rank if comm else 0)]
    src = {k: make_frames(torch, 1, sw, sh, 4321 + k)[0] for k in own}
    ptrs = {k: t.data_ptr() for k, t in src.items()}
    out = {}
    cur = torch.cuda.current_stream()
    legs = [("nine_targets", 9, False), (f"{targets}_targets", targets, False)]
    if world == 1:  # one GPU: the tick without tiles, resize launch or collective (asciichat_hip_grid_set_direct)
        legs += [("nine_targets_direct", 9, True), (f"{targets}_targets_direct", targets, True)]
    for label, nt, direct in legs:
        grid.set_direct(direct)
        descs = []
        for _ in range(nt):  # every client looks at the same grid (stream.c:790-854: aspect + padding on)
            f = pkg.frame_setup(None, tw, 2 * th, tw, th, 0, True, True, False)
            f.comp = grid.composite_dev
            descs.append(f)
        plan = pkg.Plan(pkg.lib().achip_mode_from_caps(3, 0), PALETTE_STANDARD, descs)
        slab = torch.empty(nt * plan.stride, dtype=torch.uint8, device="cuda")
        ln = torch.zeros(nt, dtype=torch.int32, device="cuda")

        def step():
            grid.exchange(ptrs, cur.cuda_stream)
            plan.render(slab.data_ptr(), plan.stride, ln.data_ptr(), cur.cuda_stream)

        def region(K):
            torch.cuda.synchronize()
            if dist is not None:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                step()
            torch.cuda.synchronize()
            t1 = time.perf_counter()  # this rank's K steps (each with its all-gather) are done; MAX over ranks below
            if dist is not None:
                dist.barrier()
                torch.cuda.synchronize()
            return t1 - t0

        for _ in range(5):
            step()
        walls = [region(steps) for _ in range(regions)]
        if last is not None and label == f"{targets}_targets":
            last.update(slab=slab.cpu().numpy(), lens=ln.cpu().numpy().astype("uint32"), stride=plan.stride)
        if dist is not None:
            t = torch.tensor(walls, dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            walls = [float(v) for v in t.tolist()]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        step()
        e0.record(cur)
        for _ in range(max(50, steps)):
            step()
        e1.record(cur)
        torch.cuda.synchronize()
        g = e0.elapsed_time(e1) / max(50, steps)
        lens = ln.cpu().numpy().astype("uint32")
        assert (lens < 0xFFFFFFF0).all()
        cells = int(sum(d.out_w * d.out_h for d in descs))
        alg = int(lens.sum()) + 3 * cells
        wall = statistics.median(walls)
        entry = {"frames_per_s": nt * world * steps / wall, "ms_per_step": wall / steps * 1e3, "kernel_ms": g,
                 "out_bytes_per_frame": float(lens.mean()), "alg_bytes_per_launch": alg,
                 "roofline_GBps": alg / (g * 1e-3) / 1e9, "roofline_frac": alg / (g * 1e-3) / 1e9 / HBM_PEAK_GBS,
                 "kernel_variant": plan.variant, "bands_per_frame": plan.parts, "targets_per_rank": nt,
                 "collective": ("none: plans sample the sources directly, a tick refreshes nine pointers" if direct else
                                "ncclAllGather of the composite tiles inside every step (C-ABI, comm.c)") if comm else "none (gloo run)",
                 "sources_owned_by_rank0": len(own), "rccl_ranks": comm.count if comm else None}
        if comm and not direct and label != "nine_targets":
            # configs[3]'s consumer side: every rank's rendered target frames all-gathered, both forms
            try:
                entry["all_gather_of_rendered_frames"] = gather_leg(torch, pkg, comm, plan, nt, world, rank, reps=6)
            except Exception as e:  # never lose the leg's timing to the optional exchange
                entry["all_gather_of_rendered_frames"] = {"error": str(e)[:200]}
        if rank == 0 and world == 1:  # the composite every rank renders from is the oracle's, byte for byte
            allsrc = [np.ascontiguousarray(make_frames(torch, 1, sw, sh, 4321 + k)[0].cpu().numpy()) for k in range(n)]
            exp = orc.convert_with_caps(orc.composite(allsrc, tw, th), tw, th, 3, 0, True, True, False)
            got = bytes(slab[:int(lens[0])].cpu().numpy())
            if got != exp:
                raise SystemExit("bench.py: grid frame differs from the oracle")
            entry["verify"] = {"frames_checked": 1, "byte_identical_to_oracle": True}
        out[label] = entry
        plan.close()
    grid.close()
    if comm:
        comm.close()
    return out


def wire_stage(torch, pkg, res, steps=None):
    """SURVEY 8(f).3 behind the metric's render, measured in this run: GPU time per step (HIP events, same schedule as
    the main leg: res['streams'] launches in flight, a fresh input batch every step) of (a) render alone, (b) render +
    the stand-alone checksum / packet-header kernel (a second pass over the slab), (c) the render launch that also
    leaves frame CRC-32Cs, packet headers and packet CRCs (asciichat_hip_plan_render_packets).  The fused checksums are compared with the stand-alone kernel's on a whole
    batch and with the oracle's CRC-32C on 8 frames."""
    import numpy as np

    import orc

    L = pkg.lib()
    plans, batch, S = res["plans"], res["batch"], res["streams"]
    if steps is None:  # ~10 ms of GPU time per timing whatever the workload
        steps = max(12, min(160, int(10.0 / max(res["gpu_ms"], 1e-3))))
    for p in plans:  # the serial leg left them at one launch in flight
        p.set_concurrency(S)
        if res.get("forced_variant", -1) >= 0:
            p.set_variant(res["forced_variant"])
    stride = plans[0].stride
    lanes = [torch.cuda.current_stream()] + _LANE_POOL[:S - 1]
    outs = [torch.empty(batch * stride, dtype=torch.uint8, device="cuda") for _ in range(S)]
    lns = [torch.zeros(batch, dtype=torch.int32, device="cuda") for _ in range(S)]
    crcs = [torch.zeros(batch, dtype=torch.int32, device="cuda") for _ in range(S)]
    hdrs = [torch.zeros(batch * 24, dtype=torch.uint8, device="cuda") for _ in range(S)]
    pkts = [torch.zeros(batch, dtype=torch.int32, device="cuda") for _ in range(S)]
    sw, sh, W, H, cl, rm = WORKLOADS[res["name"]]
    dims = torch.tensor([[W, H]] * batch, dtype=torch.int32, device="cuda")
    # compacted copies (device memory here: the passes over HBM are what is compared; with_d2h_packed has the PCIe side)
    pks = [torch.empty(batch * stride, dtype=torch.uint8, device="cuda") for _ in range(S)]
    offs = [torch.zeros(batch + 1, dtype=torch.int64, device="cuda") for _ in range(S)]
    plens = [torch.zeros(batch, dtype=torch.int32, device="cuda") for _ in range(S)]

    def step(kind, k):
        s, p = k % S, plans[k % len(plans)]
        st = lanes[s].cuda_stream
        if kind == "packets_then_pack":  # the wire stage, then the compaction as a pass of its own
            p.render_packets(outs[s].data_ptr(), stride, lns[s].data_ptr(), dims.data_ptr(), crcs[s].data_ptr(),
                             hdrs[s].data_ptr(), pkts[s].data_ptr(), st)
            pkg.pack_frames(outs[s].data_ptr(), stride, lns[s].data_ptr(), batch, pks[s].data_ptr(), batch * stride,
                            offs[s].data_ptr(), plens[s].data_ptr(), st)
            return
        if kind == "packets_packed":  # ... in the library's own form: one pass checksums AND packs where the CRC is not fused
            p.render_packets_packed(outs[s].data_ptr(), stride, lns[s].data_ptr(), dims.data_ptr(), crcs[s].data_ptr(),
                                    hdrs[s].data_ptr(), pkts[s].data_ptr(), pks[s].data_ptr(), batch * stride,
                                    offs[s].data_ptr(), plens[s].data_ptr(), st)
            return
        if kind == "fused":  # ONE call, one launch: frames + frame CRCs + headers + packet CRCs
            p.render_packets(outs[s].data_ptr(), stride, lns[s].data_ptr(), dims.data_ptr(), crcs[s].data_ptr(),
                             hdrs[s].data_ptr(), pkts[s].data_ptr(), st)
            rc = 0
        else:
            p.render(outs[s].data_ptr(), stride, lns[s].data_ptr(), st)
            rc = 0
            if kind == "separate":
                rc = L.asciichat_hip_frame_packets(outs[s].data_ptr(), stride, lns[s].data_ptr(), stride, batch,
                                                   dims.data_ptr(), crcs[s].data_ptr(), hdrs[s].data_ptr(),
                                                   pkts[s].data_ptr(), st)
        assert rc == 0, pkg.last_error()

    def timed(kind):
        for k in range(2 * S):
            step(kind, k)
        torch.cuda.synchronize()
        b = [torch.cuda.Event(enable_timing=True) for _ in range(S)]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(S)]
        for s in range(S):
            step(kind, s)
            b[s].record(lanes[s])
        for k in range(steps):
            step(kind, k)
        for s in range(S):
            e[s].record(lanes[s])
        torch.cuda.synchronize()
        return max(b[s].elapsed_time(e[t]) for s in range(S) for t in range(S)) / steps

    got = {}
    for kind in ("separate", "fused"):
        step(kind, 0)
        torch.cuda.synchronize()
        got[kind] = (crcs[0].cpu().numpy().astype("uint32").copy(), pkts[0].cpu().numpy().astype("uint32").copy(),
                     hdrs[0].cpu().numpy().copy())
    same = all((a == b).all() for a, b in zip(got["separate"], got["fused"]))
    host, lens = outs[0].cpu().numpy(), lns[0].cpu().numpy().astype("uint32")
    idx = sorted(set(int(round(i * (batch - 1) / 7)) for i in range(min(8, batch))))
    oracle_ok = all(int(got["fused"][0][i]) == orc.crc32c(host[i * stride:i * stride + int(lens[i])].tobytes()) for i in idx)
    if not (same and oracle_ok):
        raise SystemExit("bench.py: fused frame checksums differ from the stand-alone kernel's / the oracle's")
    one_launch = bool(plans[0].exact_length)  # the render writes exact-length frames itself (no slab, no second pass)
    t = {kind: statistics.median(timed(kind) for _ in range(3))
         for kind in ("render", "separate", "fused", "packets_then_pack", "packets_packed")}
    if one_launch:  # the same entry point with that form switched off: render (+ fused wire stage) + pack_frames
        for p in plans:
            p.set_exact_length(0)
        t["packets_packed_two_launches"] = statistics.median(timed("packets_packed") for _ in range(3))
        for p in plans:
            p.set_exact_length(-1)
    # the compacted copies of the two forms agree: lengths, every frame's bytes at its offset, the destination tiled
    ref = {}
    for kind in ("packets_then_pack", "packets_packed"):
        step(kind, 0)
        torch.cuda.synchronize()
        o, l = offs[0].cpu().numpy().copy(), plens[0].cpu().numpy().astype("uint32").copy()
        pk = pks[0].cpu().numpy()
        spans = sorted((int(o[i]), int(o[i]) + (int(l[i]) + 15) // 16 * 16) for i in range(batch))
        tiled = spans[0][0] == 0 and all(spans[i][1] == spans[i + 1][0] for i in range(batch - 1)) and spans[-1][1] == int(o[batch])
        ref[kind] = (tiled, l, [pk[int(o[i]):int(o[i]) + int(l[i])].tobytes() for i in idx])
    if not (ref["packets_then_pack"][0] and ref["packets_packed"][0] and (ref["packets_then_pack"][1] == ref["packets_packed"][1]).all()
            and ref["packets_then_pack"][2] == ref["packets_packed"][2]):
        raise SystemExit("bench.py: the packed output of plan_render_packets_packed differs from wire stage + pack_frames")
    forced = None
    if not plans[0].fused_crc:  # a geometry that carries the fused CRC without it being the faster form (the rows kernel)
        for p in plans:
            p.set_fused_crc(1)
        if plans[0].fused_crc:
            forced = statistics.median(timed("fused") for _ in range(3))
        for p in plans:
            p.set_fused_crc(-1)
    return {"launches_in_flight": S, "steps": steps, "fused_crc_in_render_kernel": bool(plans[0].fused_crc),
            "render_with_fused_crc_forced_ms_per_step": forced,
            "kernel_variant": plans[0].variant,
            "render_ms_per_step": t["render"], "render_plus_packet_kernel_ms_per_step": t["separate"],
            "render_with_fused_crc_and_headers_ms_per_step": t["fused"],
            "extra_ms_separate": t["separate"] - t["render"], "extra_ms_fused": t["fused"] - t["render"],
            "packed": {"wire_stage_then_pack_frames_ms_per_step": t["packets_then_pack"],
                       "render_packets_packed_ms_per_step": t["packets_packed"],
                       "exact_length_frames_written_by_the_render_kernel": one_launch,
                       "render_packets_packed_two_launches_ms_per_step": t.get("packets_packed_two_launches"),
                       "note": "the frames also compacted (device destination): plan_render_packets + pack_frames against "
                               "plan_render_packets_packed -- behind a fused render the same two launches, otherwise ONE pass "
                               "that checksums and packs instead of two passes over the slab"},
            "checked": {"frames_vs_standalone_kernel": batch, "frames_vs_oracle_crc32c": len(idx), "identical": True},
            "note": "ascii_frame_packet_t.checksum + 24-byte headers + packet CRCs for every frame of the step "
                    "(lib/network/acip/server.c:186-214); calls issued from Python: render + asciichat_hip_frame_packets "
                    "(two launches) vs asciichat_hip_plan_render_packets (one launch)"}


def tick_e2e(torch, pkg, n=256, distinct=32, ticks=(2, 4), forms=("whole_blob", "sampled_rows", "sampled_pixels_batched", "sampled_images"),
             grid=(80, 24)):
    """The end-to-end server tick (SURVEY 8f.2 + path + 8f.3), PCIe included on both sides: n clients' host blobs
    [u32 BE w][u32 BE h][RGB24] (blocks of the pinned pool, as the receive path would fill them) -> frame table ->
    plan_render_packets -> frames in use + headers packed into mapped pinned host memory.  Three publish forms: the whole
    blob (frame_table_publish: one in-place DMA of 6.2 MB per client), the sampled rows only (frame_table_publish_rows:
    24 of 1080 rows, a DMA and a launch per client) and the whole tick in one call (frame_table_publish_rows_batch: the
    sampled pixels of every client in one block, one DMA, one launch).  Never `value`: this is PCIe- and host-bound (the per-client calls are
    issued from this interpreter; tests/cabi/server_tick_port.c is the same tick in C)."""
    import numpy as np

    import orc

    sw, sh, (W, H) = 1920, 1080, grid
    L = pkg.lib()
    st = torch.cuda.current_stream().cuda_stream
    blob_bytes = 8 + sw * sh * 3
    rng = np.random.default_rng(99)
    blobs, imgs = [], []
    for k in range(distinct):
        p = L.buffer_pool_alloc(None, blob_bytes)  # > 4 MiB: the pinned, device-mapped class
        if not p:
            raise RuntimeError("buffer_pool_alloc failed")
        v = np.ctypeslib.as_array((C.c_uint8 * blob_bytes).from_address(p))
        v[:8] = np.frombuffer(sw.to_bytes(4, "big") + sh.to_bytes(4, "big"), dtype=np.uint8)
        img = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
        v[8:] = img.reshape(-1)
        blobs.append(p)
        imgs.append(img)
    table = pkg.FrameTable(n)
    tmpl = pkg.frame_setup(None, sw, sh, W, H, 0, False, False, False)
    mode = L.achip_mode_from_caps(3, 0)
    plan = None
    tab = (8 * (n + 1) + 4 * n + 15) // 16 * 16
    dims = torch.tensor([[W, H]] * n, dtype=torch.int32, device="cuda")
    crc = torch.zeros(n, dtype=torch.int32, device="cuda")
    hdr = torch.zeros(n * 24, dtype=torch.uint8, device="cuda")
    pkt = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = {}
    slot_arr = (C.c_int * n)(*range(n))
    size_arr = (C.c_size_t * n)(*([blob_bytes] * n))
    ptr_arrs = [(C.c_void_p * n)(*[blobs[(i + t) % distinct] for i in range(n)]) for t in range(distinct)]
    tmpl_arr = (pkg.Frame * 1)(tmpl)
    frames = (pkg.Frame * n)(*[pkg.Frame.from_buffer_copy(tmpl) for _ in range(n)])
    for form in forms:
        t_pub = t_all = 0.0
        dense = form == "sampled_images"
        batched = form == "sampled_pixels_batched" or dense
        n_ticks = ticks[0] if form == "whole_blob" else ticks[1] * (5 if batched else 1) * (4 if dense else 1)
        if dense:  # fresh descriptors: latest_frames rewrites them onto the sampled images
            frames = (pkg.Frame * n)(*[pkg.Frame.from_buffer_copy(tmpl) for _ in range(n)])
        for tick in range(n_ticks + 2):  # the first ticks allocate (frame buffers, staging, ring blocks): untimed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if dense:  # the images the targets sample, gathered on the ingest pool: one block, one DMA, NO launch
                table.publish_sampled_batch(slot_arr, (ptr_arrs[tick % distinct], size_arr), tmpl_arr, st)
            elif batched:  # one packed block (sampled pixels), one DMA, one scatter launch for the whole tick
                table.publish_rows_batch(slot_arr, (ptr_arrs[tick % distinct], size_arr), tmpl_arr, st)
            for i in range(0 if batched else n):
                if form == "whole_blob":
                    table.publish_at(i, blobs[(i + tick) % distinct], blob_bytes, st)
                else:
                    table.publish_rows(i, (blobs[(i + tick) % distinct], blob_bytes), [tmpl], st)
            t1 = time.perf_counter()
            if table.latest_frames(slot_arr, frames, st) != n:  # one call: every descriptor's source pointer
                raise SystemExit("bench.py: tick_e2e: a client without a frame")
            if plan is None:
                plan = pkg.Plan(mode, PALETTE_STANDARD, list(frames))
                slab = torch.empty(n * plan.stride, dtype=torch.uint8, device="cuda")
                ln = torch.zeros(n, dtype=torch.int32, device="cuda")
                hb = pkg.HostBuffer(tab + n * plan.stride)
            else:
                plan.update(frames, st)
            # the send side in one call: frames + checksums + headers, and the frames at their exact lengths in host memory
            plan.render_packets_packed(slab.data_ptr(), plan.stride, ln.data_ptr(), dims.data_ptr(), crc.data_ptr(),
                                       hdr.data_ptr(), pkt.data_ptr(), hb.dev + tab, n * plan.stride, hb.dev,
                                       hb.dev + 8 * (n + 1), st)
            hdr_host = hdr.cpu()  # 6 KB of headers (a blocking copy: also the tick's synchronisation point)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if tick > 1:
                t_pub += t1 - t0
                t_all += t2 - t0
        n_ticks += 1  # (index of the last tick, for the check below)
        v = hb.view()
        off = v[:8 * (n + 1)].view(np.uint64)
        lh = v[8 * (n + 1):8 * (n + 1) + 4 * n].view(np.uint32)
        for i in (0, n - 1):  # what arrived on the host is the oracle's frame of that client's blob
            exp = orc.convert_with_caps(imgs[(i + n_ticks) % distinct], W, H, 3, 0, False, False, False)
            if v[tab + int(off[i]):tab + int(off[i]) + int(lh[i])].tobytes() != exp:
                raise SystemExit(f"bench.py: tick_e2e ({form}) frame {i} differs from the oracle")
        rows = H
        up = n * (blob_bytes - 8) if form == "whole_blob" else n * (rows * sw * 3 + 16 * ((rows * 4 + 15) // 16))
        if batched:  # [record][row table][column table][H x W sampled pixels] per client
            up = n * (32 + 16 * ((rows * 4 + 15) // 16) + 16 * ((W * 4 + 15) // 16) + 16 * ((rows * W * 3 + 15) // 16))
        n_ticks -= 1
        if dense:
            up = n * 16 * ((rows * W * 3 + 15) // 16)
        out[form] = {"frames_per_s": n * n_ticks / t_all, "ms_per_tick": t_all / n_ticks * 1e3,
                     "publish_ms_per_tick": t_pub / n_ticks * 1e3, "ticks_timed": n_ticks,
                     "pcie_bytes_up_per_tick": int(up), "pcie_bytes_down_per_tick": int(off[n]) + tab + 24 * n,
                     "verified_frames_vs_oracle": 2}
    if "sampled_images" not in forms:
        raise ValueError("tick_e2e: the pipelined leg follows the sampled_images form")
    out["sampled_images"]["ingest_threads"] = L.asciichat_hip_ingest_threads()
    # the same tick PIPELINED, as a server runs it: tick k+1 is gathered and uploaded (one stream) while tick k renders and
    # crosses PCIe on its way out (another stream, its own output buffers); the host waits for tick k-1's output only
    s2 = torch.cuda.Stream()
    lanes2 = [torch.cuda.current_stream(), s2]
    plans = [plan, pkg.Plan(mode, PALETTE_STANDARD, list(frames))]
    slabs = [slab, torch.empty_like(slab)]
    lns = [ln, torch.zeros_like(ln)]
    crcs, hdrs, pkts = [crc, torch.zeros_like(crc)], [hdr, torch.zeros_like(hdr)], [pkt, torch.zeros_like(pkt)]
    hbs = [hb, pkg.HostBuffer(tab + n * plan.stride)]
    evs = [torch.cuda.Event(), torch.cuda.Event()]
    n_pipe = ticks[1] * 40
    t_start = None
    for tick in range(n_pipe + 4):
        if tick == 4:
            torch.cuda.synchronize()
            t_start = time.perf_counter()
        k = tick & 1
        stq = lanes2[k].cuda_stream
        if tick >= 2:
            evs[k].synchronize()  # tick - 2 used these buffers: its frames are on the host now (the consumer's cue)
        table.publish_sampled_batch(slot_arr, (ptr_arrs[tick % distinct], size_arr), tmpl_arr, stq)
        if table.latest_frames(slot_arr, frames, stq) != n:
            raise SystemExit("bench.py: tick_e2e: a client without a frame")
        plans[k].update(frames, stq)
        plans[k].render_packets_packed(slabs[k].data_ptr(), plan.stride, lns[k].data_ptr(), dims.data_ptr(), crcs[k].data_ptr(),
                                       hdrs[k].data_ptr(), pkts[k].data_ptr(), hbs[k].dev + tab, n * plan.stride, hbs[k].dev,
                                       hbs[k].dev + 8 * (n + 1), stq)
        evs[k].record(lanes2[k])
    torch.cuda.synchronize()
    t_pipe = time.perf_counter() - t_start
    last = (n_pipe + 3)
    v = hbs[last & 1].view()
    off = v[:8 * (n + 1)].view(np.uint64)
    lh = v[8 * (n + 1):8 * (n + 1) + 4 * n].view(np.uint32)
    for i in (0, n - 1):
        exp = orc.convert_with_caps(imgs[(i + last) % distinct], W, H, 3, 0, False, False, False)
        if v[tab + int(off[i]):tab + int(off[i]) + int(lh[i])].tobytes() != exp:
            raise SystemExit(f"bench.py: tick_e2e (pipelined) frame {i} differs from the oracle")
    out["sampled_images_pipelined"] = {"frames_per_s": n * n_pipe / t_pipe, "ms_per_tick": t_pipe / n_pipe * 1e3,
                                       "ticks_timed": n_pipe, "ticks_in_flight": 2, "verified_frames_vs_oracle": 2}
    plans[1].close()
    hbs[1].close()
    plan.close()
    hb.close()
    table.close()
    for p in blobs:
        L.buffer_pool_free(None, p, blob_bytes)
    out["note"] = (f"{n} clients, 1080p -> {W}x{H} truecolor, blobs in the pinned pool; publish + latest + plan_update + "
                   "plan_render_packets_packed (frames + wire stage, exact-length frames into mapped host memory) per tick; calls issued from Python")
    return out


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def usable_cpus():
    """CPUs this process may keep busy: the affinity mask capped by the cgroup's CPU quota (the GPU boxes show 256 hardware
    threads and grant 16 CPUs' worth of time: more runnable threads than that only get the process throttled)."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    quota = None
    try:
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = -(-int(q) // int(period))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            period = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0 and period > 0:
                quota = -(-q // period)
        except (OSError, ValueError):
            pass
    return max(1, min(n, quota) if quota else n), quota


def cpu_baseline(name, budget_s=12.0):
    """Times the CPU oracle (port of the reference's scalar path) on this host: 1 thread and all cores,
    on a bounded sample of the same workload (same frame shape, S-noise input, same caps)."""
    import numpy as np

    import orc

    sw, sh, W, H, cl, rm = WORKLOADS[name]
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    L = orc.lib()
    pal = orc.PALETTE_STANDARD.encode()
    nb = C.c_uint64()
    t = L.orc_bench_convert(img.ctypes.data, sw, sh, W, H, cl, rm, pal, 20, 1, C.byref(nb))
    per = max(t / 20, 1e-7)
    it1 = max(50, int(budget_s * 0.4 / per))
    t1 = L.orc_bench_convert(img.ctypes.data, sw, sh, W, H, cl, rm, pal, it1, 1, C.byref(nb))
    cores = os.cpu_count() or 1
    th, quota = usable_cpus()
    th = min(th, 256)
    itn = max(20, int(budget_s * 0.6 / per * 16 / max(16, th)))
    tn = L.orc_bench_convert(img.ctypes.data, sw, sh, W, H, cl, rm, pal, itn, th, C.byref(nb))
    return {
        "value": it1 / t1, "unit": "frames/s", "cores": 1, "kind": "port", "cpu_model": cpu_model(),
        "host_threads": cores, "cgroup_cpu_quota": quota,
        "sample": f"{it1} x ({sw}x{sh}->{W}x{H}, color_level={cl}, render_mode={rm}, uniform-noise frame) on 1 thread; "
                  f"{itn} per thread on {th} threads",
        "all_cores": {"value": itn * th / tn, "cores": th,
                      "note": "as many threads as the process may keep busy (affinity mask, cgroup CPU quota)"},
    }


def committed_profile(workload):
    """rocprofv3 summaries committed under profiles/ (NOT measured by this run; labelled with their source)."""
    path = os.path.join(ROOT, "profiles", "committed_profile.json")
    try:
        ent = json.load(open(path)).get(workload)
    except Exception:
        return None
    return ent


def maybe_spawn_ranks(args):
    """`python bench.py --gpus N` with N > 1 and no launcher around it: become N ranks, one per GPU, under
    torch.distributed.run (the reference's model is one render thread per client, src/server/render.c:1233; here one
    process per GPU).  Fails loudly when fewer than N devices are visible.  Under a launcher (WORLD_SIZE set) the flag
    must agree with the world the launcher made."""
    backend = os.environ.get("ASCIICHAT_BENCH_BACKEND", "nccl")
    if "WORLD_SIZE" in os.environ:
        if int(os.environ["WORLD_SIZE"]) != args.gpus:
            raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher created WORLD_SIZE={os.environ['WORLD_SIZE']} rank(s)")
        return
    if args.gpus <= 1:
        return
    import socket

    import torch

    # (only RCCL needs the count: a gloo run's ranks share the visible GPUs, and this process then never opens one)
    have = torch.cuda.device_count() if backend == "nccl" else args.gpus
    if have < args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} needs {args.gpus} HIP devices, {have} visible (one process per GPU; "
                         "RCCL refuses two ranks on one device)")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    # a fresh child, not exec: this process may have opened the HIP runtime (device_count above)
    raise SystemExit(subprocess.call(cmd))


def rank_comm(torch, pkg, dist, world, rank, backend):
    """The C-ABI's RCCL communicator over the ranks of this run (comm.c), its unique id broadcast through
    torch.distributed.  None for a single rank, and for a gloo test run unless a stand-in transport is named
    (ASCIICHAT_HIP_RCCL_LIB = tests/cabi/libloopback_rccl.so: the ranks share one GPU, RCCL itself would refuse them)."""
    if world <= 1 or (backend != "nccl" and not os.environ.get("ASCIICHAT_HIP_RCCL_LIB")):
        return None
    uid = torch.zeros(pkg.COMM_ID_BYTES, dtype=torch.uint8, device="cuda" if backend == "nccl" else "cpu")
    if rank == 0:
        uid.copy_(torch.frombuffer(bytearray(pkg.comm_unique_id()), dtype=torch.uint8))
    dist.broadcast(uid, 0)
    return pkg.Comm(world, rank, bytes(uid.cpu().numpy()))


def gather_leg(torch, pkg, comm, plan, batch, world, rank, reps=10):
    """What a consumer that needs every rank's frames pays: this rank's rendered block all-gathered through
    comm.c's one entry (asciichat_hip_comm_all_gather_frames) in BOTH forms -- `packed` (lengths first, the host sizes the
    second collective: the bytes in use cross the links, one stream synchronisation) and `slab` (lengths + worst-case-stride
    slab in ONE group: no host synchronisation) -- plus which one ASCIICHAT_HIP_GATHER selects (the first
    visit to a real multi-GPU node is a one-shot A/B)."""
    st = torch.cuda.current_stream().cuda_stream
    stride = plan.stride
    slab = torch.zeros(world * batch * stride, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(world * batch, dtype=torch.int32, device="cuda")
    packed = torch.zeros(world * batch * stride, dtype=torch.uint8, device="cuda")
    mine, mylen = slab.data_ptr() + rank * batch * stride, ln.data_ptr() + 4 * rank * batch
    out, where = {}, {}
    for kind, form in (("slab", 1), ("packed", 0)):
        ts = []
        for _ in range(reps + 2):
            plan.render(mine, stride, mylen, st)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            base, off, lens, blk, took = comm.all_gather_frames(slab.data_ptr(), stride, ln.data_ptr(), batch, packed.data_ptr(),
                                                                batch * stride, form, st)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        assert took == form
        where[kind] = (off, lens)
        out[kind] = {"ms": statistics.median(ts[2:]) * 1e3, "bytes_per_rank": int(blk), "bytes_total": int(blk) * world,
                     "host_synchronisations": 1 if form == 0 else 0}
    out["fixed_stride"] = out["slab"]  # (the key of rounds 2-5)
    env_form = comm.all_gather_frames(slab.data_ptr(), stride, ln.data_ptr(), batch, packed.data_ptr(), batch * stride, -1, st)[4]
    torch.cuda.synchronize()
    out["selected_by_environment"] = {"ASCIICHAT_HIP_GATHER": os.environ.get("ASCIICHAT_HIP_GATHER"), "form": ("packed", "slab")[env_form]}
    # the two must agree: every frame of every rank, byte for byte
    host_s, host_p, hl = slab.cpu().numpy(), packed.cpu().numpy(), ln.cpu().numpy().astype("uint32")
    off, lens = where["packed"]
    for i in range(0, world * batch, max(1, world * batch // 64)):
        a = host_s[where["slab"][0][i]:where["slab"][0][i] + int(hl[i])]
        b = host_p[off[i]:off[i] + lens[i]]
        if int(hl[i]) != lens[i] or not (a == b).all():
            raise RuntimeError(f"all-gather legs disagree on frame {i}")
    out["frames_compared"] = len(range(0, world * batch, max(1, world * batch // 64)))
    return out


def time_with_d2h_packed(torch, pkg, plans, n, steps, lanes=2):
    """The PCIe-inclusive rate with exact-length transfers: render, then the pack kernel writes the frames in use (and their
    offset / length tables) straight into mapped pinned host memory -- its stores are the transfer.  `lanes` batches in
    flight on separate streams so that one batch's render hides behind another's PCIe time.  After the run the host-side
    bytes of the last step are compared with a device-side render."""
    stride = plans[0].stride
    tab = (8 * (n + 1) + 4 * n + 15) // 16 * 16
    st = [torch.cuda.current_stream()] + _LANE_POOL[:lanes - 1]
    while len(st) < lanes:
        _LANE_POOL.append(torch.cuda.Stream())
        st.append(_LANE_POOL[-1])
    slabs = [torch.empty(n * stride, dtype=torch.uint8, device="cuda") for _ in range(lanes)]
    lns = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(lanes)]
    hbs = [pkg.HostBuffer(tab + n * stride) for _ in range(lanes)]

    def step(k):
        l, p = k % lanes, plans[(k % lanes) + lanes * ((k // lanes) % (len(plans) // lanes))]
        p.render_packed(slabs[l].data_ptr(), stride, lns[l].data_ptr(), hbs[l].dev + tab, n * stride, hbs[l].dev,
                        hbs[l].dev + 8 * (n + 1), st[l].cuda_stream)

    for k in range(4 * lanes):
        step(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        step(k)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    import numpy as np
    last = (steps - 1) % lanes
    v = hbs[last].view()
    off = v[:8 * (n + 1)].view(np.uint64)
    ln = v[8 * (n + 1):8 * (n + 1) + 4 * n].view(np.uint32)
    k_last = steps - 1  # (a plan that writes exact-length frames itself leaves the slab alone: render it for the comparison)
    p_last = plans[(k_last % lanes) + lanes * ((k_last // lanes) % (len(plans) // lanes))]
    p_last.render(slabs[last].data_ptr(), stride, lns[last].data_ptr(), st[last].cuda_stream)
    torch.cuda.synchronize()
    dev_slab, dev_len = slabs[last].cpu().numpy(), lns[last].cpu().numpy().astype("uint32")
    for i in range(0, n, max(1, n // 16)):
        if int(ln[i]) != int(dev_len[i]) or not (v[tab + int(off[i]):tab + int(off[i]) + int(ln[i])] ==
                                                  dev_slab[i * stride:i * stride + int(ln[i])]).all():
            raise SystemExit(f"bench.py: packed host copy of frame {i} differs from the device slab")
    total = int(off[n])
    for hb in hbs:
        hb.close()
    return {"ms_per_step": dt * 1e3, "frames_per_s": n / dt, "bytes_over_pcie_per_step": total + tab,
            "GBps": (total + tab) / dt / 1e9, "fixed_stride_bytes_per_step": n * stride + 4 * n, "lanes": lanes,
            "note": "render + pack kernel storing the bytes in use (16-byte aligned frame starts) and the offset / length "
                    "tables straight into mapped pinned host memory; no DMA, no host round trip for a size"}


LINE_TARGET_BYTES = 4096  # the stdout line the driver parses: small enough to survive any tail window
LINE_HARD_LIMIT_BYTES = 8192
_COMPACT_TOP = ("metric", "value", "unit", "n_gpus", "rccl_ranks", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data")
_COMPACT_ROOFLINE = ("bound", "achieved", "peak", "unit", "frac", "frac_timed_region", "frac_profile", "frac_profile_best", "frac_profile_n", "frac_profile_source", "traffic",
                     "traffic_source", "alg_bytes_per_launch", "kernel_ms", "launches_in_flight")
_COMPACT_CPU = ("value", "unit", "cores", "kind", "sample", "cpu_model")


def _r(v, sig=6):
    """Floats to `sig` significant digits: the line is for reading and parsing, the side file keeps full precision."""
    if isinstance(v, float) and math.isfinite(v) and v != 0.0:
        return float(f"{v:.{sig}g}")
    return v


def compact_line(full):
    """The ONE stdout line: exactly the contract's keys + roofline + cpu_baseline + verify, and a
    two-number digest (frames/s, roofline fraction) of every other workload this run measured.  Everything else -- the
    legs, the autotune tables, the notes -- lives in the side file (`--extra`, default bench_extra.json)."""
    line = {k: _r(full[k]) for k in _COMPACT_TOP if k in full}
    line.setdefault("rccl_ranks", None)
    cfg = full.get("config") or {}
    line["config"] = {k: v for k, v in cfg.items() if not isinstance(v, str) or len(v) <= 96}
    if "roofline" in full:
        line["roofline"] = {k: _r(full["roofline"][k]) for k in _COMPACT_ROOFLINE if k in full["roofline"]}
    cb = full.get("cpu_baseline")
    if cb:
        c = {k: _r(cb[k]) for k in _COMPACT_CPU if k in cb}
        if "all_cores" in cb:
            c["all_cores"] = {"value": _r(cb["all_cores"]["value"]), "cores": cb["all_cores"]["cores"]}
        line["cpu_baseline"] = c
    if full.get("verify") is not None:
        line["verify"] = full["verify"]
    one = full.get("one_launch_at_a_time")
    if one:
        line["one_launch_at_a_time"] = {"kernel_ms": _r(one["kernel_ms"]), "roofline_frac": _r(one["roofline_frac"])}
    mg = full.get("multi_gpu")
    if mg:
        line["multi_gpu"] = {"backend": mg.get("torch_distributed_backend"),
                             "per_rank_frames_per_s": [_r(v, 4) for v in mg.get("per_rank_frames_per_s") or []]}
        if "error" in mg:
            line["multi_gpu"]["error"] = mg["error"][:120]
    digest = {}
    for name, e in (full.get("other_workloads") or {}).items():
        if "frames_per_s" in e:
            digest[name] = [_r(e["frames_per_s"], 4), _r(e.get("roofline_frac"), 3)]
        else:  # grid9: a dict of legs
            for leg, g in e.items():
                if isinstance(g, dict) and "frames_per_s" in g:
                    digest[f"{name}:{leg}"] = [_r(g["frames_per_s"], 4), _r(g.get("roofline_frac"), 3)]
    for leg, g in (full.get("grid9") or {}).items():
        if isinstance(g, dict) and "frames_per_s" in g:
            digest[f"grid9:{leg}"] = [_r(g["frames_per_s"], 4), _r(g.get("roofline_frac"), 3)]
    if digest:
        line["other_workloads_fps_frac"] = digest
    sw = full.get("batch_sweep")
    if sw:  # per workload: [frames/s, roofline fraction] at every batch size, in the order of "batches"
        line["batch_sweep"] = {"batches": sw.get("batches"),
                               "fps_frac": {n: [[_r(p.get("frames_per_s"), 4), _r(p.get("roofline_frac"), 3)] for p in row.values()]
                                            for n, row in (sw.get("workloads") or {}).items()}}
    for leg in ("tick_e2e", "wire_stage", "with_d2h_packed"):
        e = full.get(leg)
        if not isinstance(e, dict):
            continue
        if leg == "tick_e2e":
            line[leg] = {k: _r(v["frames_per_s"], 4) for k, v in e.items() if isinstance(v, dict) and "frames_per_s" in v}
        elif leg == "wire_stage" and "render_ms_per_step" in e:
            line[leg] = {"render_ms": _r(e["render_ms_per_step"], 4),
                         "frames_crc_headers_ms": _r(e["render_with_fused_crc_and_headers_ms_per_step"], 4),
                         "packed_ms": _r((e.get("packed") or {}).get("render_packets_packed_ms_per_step"), 4)}
        elif "frames_per_s" in e:
            line[leg] = {"frames_per_s": _r(e["frames_per_s"], 4)}
    return line


def emit_text(full, extra_path):
    """Writes the full record to `extra_path` and returns the compact line's text; shrinks the line (digest first, then
    the optional legs) if it is over the target, and refuses outright above the hard limit."""
    if extra_path:
        try:
            with open(extra_path, "w") as f:
                json.dump(full, f, indent=1)
            print(f"[bench] full record ({len(json.dumps(full))} bytes): {extra_path}", file=sys.stderr)
        except OSError as e:
            print(f"[bench] could not write {extra_path}: {e}", file=sys.stderr)
    line = compact_line(full)
    if extra_path:
        line["extra"] = os.path.basename(extra_path)
    for drop in (None, "tick_e2e", "with_d2h_packed", "wire_stage", "other_workloads_fps_frac", "batch_sweep",
                 "one_launch_at_a_time", "multi_gpu"):
        if drop:
            line.pop(drop, None)
        text = json.dumps(line, separators=(",", ":"))
        if len(text) <= LINE_TARGET_BYTES:
            break
    if len(text) > LINE_HARD_LIMIT_BYTES:
        raise SystemExit(f"bench.py: the stdout line is {len(text)} bytes (> {LINE_HARD_LIMIT_BYTES}): refusing to print it")
    json.loads(text)
    return text


DUMP_MAX_BYTES = 64 << 20
DUMP_SAMPLE_SEED = 20251015


def dump_outputs(out_dir, last, prefix=""):
    """--dump-outputs: what the timed path handed its caller in its last step, as .npy files in `out_dir`:
    frame_lengths (every frame's byte count, float64), frame_index (the frames whose bytes follow, float64) and
    frame_bytes (those frames' bytes one after another, float32).  All frames while they fit DUMP_MAX_BYTES at the
    slab's stride, else a fixed, seeded sample of them: the same frames for the same arguments."""
    import numpy as np

    lens, slab, stride = last["lens"], last["slab"], last["stride"]
    if (lens >= 0xFFFFFFF0).any():
        raise SystemExit("bench.py: the dumped step reported overflow / bad descriptor")
    n = len(lens)
    fit = (DUMP_MAX_BYTES - 16 * n) // (4 * stride)
    if fit < 1:
        raise SystemExit(f"bench.py: --dump-outputs: one frame of stride {stride} exceeds {DUMP_MAX_BYTES} bytes as float32")
    idx = np.arange(n) if fit >= n else np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(n, fit, replace=False))
    data = [slab[i * stride:i * stride + int(lens[i])] for i in idx]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, prefix + "frame_lengths.npy"), lens.astype(np.float64))
    np.save(os.path.join(out_dir, prefix + "frame_index.npy"), idx.astype(np.float64))
    np.save(os.path.join(out_dir, prefix + "frame_bytes.npy"), np.concatenate(data).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--regions", type=int, default=1,
                    help="timed regions of --steps steps each (the median region gives value / ms_per_step); the default, "
                         "1, times exactly --steps steps")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--workload", default="1080p_80x24_truecolor", choices=sorted(WORKLOADS) + ["grid9"],
                    help="grid9 = BASELINE configs[3]: nine 1080p sources -> 3x3 grid at 160x48, sharded over the ranks "
                         "with an RCCL all-gather of the composite tiles inside every step")
    ap.add_argument("--input", default="noise", choices=INPUT_KINDS)
    ap.add_argument("--aspect", action="store_true", help="use_aspect_ratio + wants_padding for the main workload")
    ap.add_argument("--others", default="default",
                    help="'default' = every BASELINE config + the input / aspect variants of SURVEY 8(d) (N=1 only); '' = none; "
                         "or a comma list of workload names")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-wire", action="store_true", help="skip the wire-stage leg (frame CRC + packet headers)")
    ap.add_argument("--no-d2h", action="store_true", help="skip the PCIe-inclusive with_d2h leg (profiling runs)")
    ap.add_argument("--variant", type=int, default=-1)
    ap.add_argument("--input-sets", type=int, default=12,
                    help="independent batches of source frames rendered round-robin (a multiple of every stream count tried)")
    ap.add_argument("--streams", type=int, default=0,
                    help="independent batches kept in flight on separate HIP streams; 0 = pick the best of 1 / 2 / 3 / 4 for "
                         "the requested burst length (--steps) in an untimed calibration; 1 = one launch at a time")
    ap.add_argument("--extra", default=os.path.join(ROOT, "bench_extra.json"),
                    help="side file for everything that is not the contract's line (legs, tables, notes); '' = none")
    ap.add_argument("--batch-sweep", default="256,1024,4096",
                    help="frames per launch for the batch-size axis of the headline, configs[2] and the sampled-image shapes "
                         "(N = 1, the default workload only); '' = none")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last one computed (frame lengths and bytes) as DIR/*.npy")
    ap.add_argument("--no-hot", action="store_true",
                    help="skip the one-launch-at-a-time / same-batch comparison legs (profiling runs)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything besides the headline: the oracle comparison, the roofline passes "
                         "and committed profile, the legs above (--others, --batch-sweep, CPU baseline, wire stage, PCIe, "
                         "one launch at a time) and, for N > 1, the all-gather leg.  Without it a run sets up, warms up, "
                         "times the steps, writes --dump-outputs and prints the line")
    args = ap.parse_args()
    maybe_spawn_ranks(args)
    # stdout carries ONE line, the JSON: libraries that print to the process's stdout on their own (RCCL's version
    # banner, through C stdio, flushed at exit) go to stderr instead -- fd 1 is pointed at fd 2 until the line is printed
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    def emit(obj):
        import ctypes
        sys.stdout.flush()
        ctypes.CDLL(None).fflush(None)  # whatever C code buffered for "stdout" so far lands on stderr
        os.write(real_stdout, (emit_text(obj, args.extra) + "\n").encode())

    if args.others in ("none", "''", '""'):
        args.others = ""
    if args.steps < 1 or args.regions < 1:
        raise SystemExit("bench.py: --steps and --regions must be at least 1")
    regions = args.regions

    import torch

    from __graft_entry__ import load_package

    pkg = load_package()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available() or pkg.lib().asciichat_hip_device_count() <= 0:
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (this path has no CPU fallback)")
    # one process per GPU; ASCIICHAT_BENCH_BACKEND=gloo lets several ranks share a GPU for testing the N > 1 control flow
    backend = os.environ.get("ASCIICHAT_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as d

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            d.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            d.init_process_group(backend)
        dist = d

    if world > 1 and backend == "nccl" and torch.cuda.device_count() < world:
        raise SystemExit(f"bench.py: {world} ranks but {torch.cuda.device_count()} HIP device(s) visible")
    if args.workload == "grid9":
        last = {}
        g = run_grid9(torch, pkg, args.steps, regions, args.batch, dist, world, rank, backend, last=last)
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, last, f"rank{rank}_" if world > 1 else "")
        e = g[f"{args.batch}_targets"]
        if rank == 0:
            emit({
                "metric": "frames/sec, nine 1080p sources -> 3x3 grid at 160x48 truecolor, one frame per target client",
                "value": e["frames_per_s"], "unit": "frames/s", "n_gpus": world, "rccl_ranks": e.get("rccl_ranks"),
                "steps": args.steps, "warmup": 5,
                "ms_per_step": e["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": "u8", "data": "synthetic (nine uniform-random 1080p RGB24 sources in HBM on their owner rank)",
                "config": {"workload": "grid9", "targets_per_gpu": args.batch, "sources": 9, "grid": "160x48",
                           "parallelism": f"sources and target clients sharded over {world} rank(s); one RCCL all-gather of "
                                          "the composite tiles per step"},
                "roofline": {"bound": "hbm", "achieved": e["roofline_GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": e["roofline_frac"], "traffic": None, "kernel_ms": e["kernel_ms"],
                             "alg_bytes_per_launch": e["alg_bytes_per_launch"]},
                "grid9": g})
        if dist is not None:
            dist.destroy_process_group()
        return
    res = run_workload(torch, pkg, args.workload, args.batch, args.steps, args.warmup, regions, dist, seed=1234 + rank,
                       variant=args.variant, nsets=args.input_sets, streams=args.streams or 4, kind=args.input,
                       aspect=args.aspect, serial_leg=args.full and not args.no_hot, verify=args.full,
                       streams_auto=(1, 2, 3, 4) if args.streams == 0 and world == 1 else None,
                       keep_last=bool(args.dump_outputs), roofline=args.full)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, res.pop("last"), f"rank{rank}_" if world > 1 else "")
    walls = res["walls"]
    per_rank_fps, multi = None, None
    if dist is not None:  # MAX over ranks of every region's wall time
        devt = "cuda" if backend == "nccl" else "cpu"
        mine = torch.tensor([args.batch * args.steps / statistics.median(walls)], dtype=torch.float64, device=devt)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank_fps = [float(v.item()) for v in allr]
        t = torch.tensor(walls, dtype=torch.float64, device=devt)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        walls = [float(v) for v in t.tolist()]
        res["walls"] = walls
        multi = {"torch_distributed_backend": backend, "per_rank_frames_per_s": per_rank_fps}
    wall = statistics.median(walls)
    main_d = summarize(res, world, wall)
    sw, sh, W, H, cl, rm = WORKLOADS[args.workload]
    line = {
        "metric": "frames/sec, 1080p->80x24 truecolor (batch of independent client frames)",
        "value": main_d["frames_per_s"], "unit": "frames/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": main_d["ms_per_step"], "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "u8",
        "data": f"synthetic ({args.input} RGB24 frames in HBM; {res['input_sets']} batches rendered round-robin)",
        "timing": {"regions": len(walls), "steps_per_region": args.steps, "statistic": "median region",
                   "region_ms": main_d["region_ms"],
                   "issue": "asciichat_hip_render_many (C) + spin wait; barrier + synchronize on both sides of every region"},
        "config": {"workload": args.workload, "batch_per_gpu": args.batch, "global_batch": args.batch * world,
                   "src": f"{sw}x{sh}", "grid": f"{W}x{H}", "mode": res["mode"], "input": args.input,
                   "aspect_and_padding": args.aspect,
                   "parallelism": f"frames sharded over {world} rank(s), no data-path collective",
                   "kernel_variant": res["variant"], "input_sets": res["input_sets"],
                   "launches_in_flight": res["streams"]},
        "cells_per_s": main_d["cells_per_s"],
    }
    if args.full:
        line["roofline"] = {
            "bound": "hbm", "achieved": main_d["roofline_GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": main_d["roofline_frac"], "traffic": None,
            # the same algorithmic bytes over the TIMED REGIONS' own clock (ms_per_step, what `value` is made of:
            # a short region carries the queues' wake-up, so this one is the lower of the two -- VERDICT r5 weak 9)
            "frac_timed_region": res["alg_bytes_per_launch"] / (main_d["ms_per_step"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "alg_bytes_per_launch": res["alg_bytes_per_launch"], "kernel_ms": res["gpu_ms"],
            "launches_in_flight": res["streams"], "out_bytes_per_frame": res["out_bytes_per_frame"],
            "kernel_ms_note": "GPU time per step (HIP events on the launch streams, first begin -> last end of a "
                              "back-to-back run of the same schedule); with launches overlapping this is what "
                              "one launch costs, not one dispatch's begin-to-end duration",
            "traffic_note": "HBM bytes need rocprofv3 --pmc passes, which this run did not make: see "
                            "committed_profile (if present) for the committed figure and its source"}
        line["output_GBps"] = main_d["output_GBps"]
        line["verify"] = res["verify"]
    if res.get("streams_autotune"):
        line["timing"]["launches_in_flight_autotune_ms_per_step"] = {str(k): v for k, v in res["streams_autotune"].items()}
    if res["serial"] is not None:
        line["one_launch_at_a_time"] = res["serial"]
    if multi is not None:
        line["multi_gpu"] = multi
        line["rccl_ranks"] = None
    if multi is not None and args.full:
        # the C-ABI's own communicator over these ranks (comm.c): how many ranks RCCL sees, and what gathering every
        # rank's frames costs -- outside the timed regions (the metric's path has no collective), AFTER the line is
        # complete and under a watchdog: if the optional leg wedges (a rank that cannot join a collective blocks the
        # others inside RCCL, where no exception can reach them) every rank gives up after MULTI_LEG_TIMEOUT_S and rank 0
        # still prints the timing line
        def give_up():
            multi["error"] = f"the all-gather leg did not finish within {MULTI_LEG_TIMEOUT_S} s; timing line printed without it"
            if rank == 0:
                emit(line)
            sys.stdout.flush()
            os._exit(0)

        watchdog = threading.Timer(MULTI_LEG_TIMEOUT_S, give_up)
        watchdog.daemon = True
        watchdog.start()
        try:
            comm = rank_comm(torch, pkg, dist, world, rank, backend)
            if comm is not None:
                multi["rccl_ranks"] = comm.count
                multi["all_gather_of_rendered_frames"] = gather_leg(torch, pkg, comm, res["plans"][0], args.batch, world, rank)
                comm.close()
        except Exception as e:  # never lose the timing line to the optional leg
            multi["error"] = str(e)[:300]
        watchdog.cancel()
        line["rccl_ranks"] = multi.get("rccl_ranks")
    cp = committed_profile(args.workload) if args.full else None
    if cp is not None:
        line["committed_profile"] = cp
        tr = cp.get("traffic") or {}
        if "hbm_bytes_per_launch" in tr and args.batch == 256 and args.input == "noise" and not args.aspect:
            # HBM bytes per launch from the committed counter passes (FETCH_SIZE with the guide's gfx950 correction +
            # WRITE_SIZE) of this very command: not collected by this run, labelled with its file
            line["roofline"]["traffic"] = tr["hbm_bytes_per_launch"]
            line["roofline"]["traffic_source"] = "committed rocprofv3 --pmc passes: " + tr.get("file", "profiles/")
        fp = cp.get("frac_profile") or {}
        if "busy_us_per_launch" in fp and args.batch == 256 and args.input == "noise" and not args.aspect:
            # the same fraction from the COMMITTED kernel traces instead of this run's HIP events: algorithmic bytes of this
            # run / busy time per launch of the traces (union of the dispatch intervals / launches, scripts/trace_stats.py) --
            # the MEDIAN over every headline trace of the profile visit, the best and the count beside it.
            # Only while the traces are of THIS code: the entry carries the identity of the sources it was taken on.
            try:
                from scripts.source_id import source_id
                here = source_id()
            except Exception:
                here = None
            if fp.get("source_id") is not None and fp.get("source_id") == here:
                f_of = lambda us: res["alg_bytes_per_launch"] / (us * 1e-6) / 1e9 / HBM_PEAK_GBS
                line["roofline"]["frac_profile"] = f_of(fp["busy_us_per_launch"])
                if "busy_us_per_launch_best" in fp:
                    line["roofline"]["frac_profile_best"] = f_of(fp["busy_us_per_launch_best"])
                line["roofline"]["frac_profile_n"] = fp.get("n_traces", 1)
                line["roofline"]["frac_profile_source"] = fp.get("file", "profiles/")
            else:
                line["committed_profile_stale"] = {"profile_source_id": fp.get("source_id"), "tree_source_id": here,
                                                   "note": "the committed traces are of other sources than this tree: no frac_profile"}
    if rank == 0 and world == 1 and args.full:
        if not args.no_d2h:
            d2h_s, d2h_bytes = time_with_d2h(torch, res["plans"][0], args.batch, 50)
            line["with_d2h"] = {"ms_per_step": d2h_s * 1e3, "frames_per_s": args.batch / d2h_s,
                                "copied_bytes_per_step": d2h_bytes, "GBps": d2h_bytes / d2h_s / 1e9,
                                "note": "whole fixed-stride slab + lengths to pinned host memory after every launch; PCIe-bound"}
            try:
                line["with_d2h_packed"] = time_with_d2h_packed(torch, pkg, res["plans"], args.batch, 60)
            except RuntimeError as e:
                line["with_d2h_packed"] = {"error": str(e)[:200]}
        if not args.no_wire:
            try:
                line["wire_stage"] = wire_stage(torch, pkg, res)
            except (RuntimeError, AssertionError) as e:  # a plan without the entry point, an out-of-memory slab, ...
                line["wire_stage"] = {"error": str(e)[:200]}
        free_workload(torch, res)
        if not args.no_d2h and args.workload == "1080p_80x24_truecolor" and args.batch == 256:
            try:
                line["tick_e2e"] = tick_e2e(torch, pkg)
            except RuntimeError as e:
                line["tick_e2e"] = {"error": str(e)[:200]}
        if not args.no_cpu:
            line["cpu_baseline"] = cpu_baseline(args.workload)
        others = {}
        if args.others == "default":
            # every BASELINE config at its own shape (noise, full W x H), then SURVEY 8(d)'s variants: the other three
            # inputs on the metric's shape and aspect + padding on every workload
            todo = [(n, "noise", False) for n in WORKLOADS if (n != args.workload or args.input != "noise" or args.aspect) and n not in ON_REQUEST_WORKLOADS]
            todo += [(args.workload, k, False) for k in INPUT_KINDS if k != "noise"]
            todo += [(n, "noise", True) for n in WORKLOADS if n not in WORKLOAD_PALETTE and n not in HEAVY_WORKLOADS and n not in PLAIN_ONLY_WORKLOADS and n not in ON_REQUEST_WORKLOADS]
        else:
            todo = [(n, "noise", False) for n in args.others.split(",") if n in WORKLOADS and n != args.workload]
        for name, kind, aspect in todo:
            big = WORKLOADS[name][0] > 3000
            b = 1 if name == "640x480_80x24_mono" else args.batch  # K1 is a single frame (configs[0])
            t_w = time.perf_counter()
            r = run_workload(torch, pkg, name, b, 40 if not big else 20, 8, 5, None,
                             nsets=4 if big else 12, streams=(args.streams or 4) if b > 1 else 1, kind=kind,
                             aspect=aspect, serial_leg=(not args.no_hot) and kind == "noise" and not aspect)
            print(f"[bench] {name} {kind} aspect={aspect}: {time.perf_counter() - t_w:.1f} s", file=sys.stderr)
            key = name + ("" if kind == "noise" else f"+{kind}") + ("+aspect_pad" if aspect else "")
            others[key] = summarize(r)
            if name in ("4k_400x120_halfblock", "1080p_80x24_halfblock") and kind == "noise" and not aspect and not args.no_wire:
                try:  # the wire stage behind the run-structured modes (rows kernel: fused form available, not the default)
                    others[key]["wire_stage"] = wire_stage(torch, pkg, r)
                except (RuntimeError, AssertionError) as e:
                    others[key]["wire_stage"] = {"error": str(e)[:200]}
            if kind in ("bars", "gray") and not args.no_d2h:  # low-entropy video: where exact-length transfers pay most
                try:
                    others[key]["with_d2h_packed"] = time_with_d2h_packed(torch, pkg, r["plans"], b, 60)
                except RuntimeError as e:
                    others[key]["with_d2h_packed"] = {"error": str(e)[:200]}
            free_workload(torch, r)
        if args.others:
            others["grid9_1080p_160x48_truecolor"] = run_grid9(torch, pkg, 20, 5)
        line["other_workloads"] = others
        if args.batch_sweep and args.workload == "1080p_80x24_truecolor" and args.input == "noise" and not args.aspect:
            bl = [int(v) for v in args.batch_sweep.split(",") if v.strip()]
            line["batch_sweep"] = {"batches": bl, "workloads": batch_sweep(torch, pkg, bl, streams=args.streams or 4),
                                   "note": "frames per launch; uniform-noise inputs, four launches in flight where the input "
                                           "sets fit; roofline_frac = algorithmic bytes per launch / HIP-event time / 8 TB/s"}
    else:
        free_workload(torch, res)
    if rank == 0:
        emit(line)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
