#!/usr/bin/env python3
"""Timing of the area-average downscale pass (profiles/box_downscale_timing.txt).

For 256 frames of 1080p -> 80x24, 4K -> 200x60 and 4K -> 400x240, and for a lone 1080p frame -> 80x24:
  * the pass (Box.run): HIP events around launches, one at a time (synchronised after each) and four in flight on four
    streams, each with a source slab and an image slab of its own (time of a round of four / 4); medians after warm-up;
  * a read-only uint4 sweep of the same source bytes (the kernel below: a contiguous span per workgroup, eight 16-byte loads
    in flight per lane, nothing stored; the best of six span sizes), timed the same way: what the traffic alone costs here;
  * source bytes / 6.3 TB/s, the achievable HBM rate;
  * the truecolor render that follows, from the averaged images (Plan over Box.render_frames), one at a time.
Inputs are resident before anything is timed.  Every shape runs in a child process of its own under a time limit; the first
that fails ends the run.

    python3 scripts/box_downscale_bench.py [--out FILE]        (--shape NAME: one shape, in this process)
"""
import ctypes as C
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM = 6.3e12
SHAPES = {  # name -> (frames, src_w, src_h, out_w, out_h)
    "1080p->80x24 x256": (256, 1920, 1080, 80, 24),
    "4K->200x60 x256": (256, 3840, 2160, 200, 60),
    "4K->400x240 x256": (256, 3840, 2160, 400, 240),
    "1080p->80x24 x1": (1, 1920, 1080, 80, 24),
}
SWEEP_CHUNK = 8 * 256 * 16  # bytes a workgroup has in flight: eight 16-byte loads per lane
SWEEP_SRC = r"""
#include <hip/hip_runtime.h>
#include <stdint.h>
// Workgroup b reads the contiguous span [b * span16, (b + 1) * span16) of 16-byte groups, as a workgroup of the pass reads
// the rows of its box: a wave's loads cover 1 KB at a time, eight loads in flight per lane, consecutive workgroups on
// consecutive spans.  Nothing is stored unless the xor of everything equals `never`.
__global__ void __launch_bounds__(256) sweep_kernel(const uint4 *__restrict__ p, uint64_t n16, uint64_t span16, uint32_t never,
                                                    uint32_t *out) {
  const uint64_t lo = (uint64_t)blockIdx.x * span16, hi = lo + span16 < n16 ? lo + span16 : n16;
  uint64_t i = lo + threadIdx.x;
  uint4 a = make_uint4(0, 0, 0, 0);
  for (; i + 7u * 256u < hi; i += 8u * 256u) {
    uint4 v[8];
#pragma unroll
    for (int k = 0; k < 8; k++)
      v[k] = p[i + (uint64_t)k * 256u];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      a.x ^= v[k].x; a.y ^= v[k].y; a.z ^= v[k].z; a.w ^= v[k].w;
    }
  }
  for (; i < hi; i += 256u) {
    const uint4 v = p[i];
    a.x ^= v.x; a.y ^= v.y; a.z ^= v.z; a.w ^= v.w;
  }
  if ((a.x ^ a.y ^ a.z ^ a.w) == never && (a.x + a.y) == never)
    out[0] = a.x;
}
extern "C" int sweep(const void *p, uint64_t bytes, uint64_t span_bytes, uint32_t *out, void *stream) {
  const uint64_t n16 = bytes / 16u, span16 = span_bytes / 16u, blocks = (n16 + span16 - 1u) / span16;
  if (!span16 || blocks > 0x7FFFFFFFull)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(sweep_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint4 *)p, n16, span16,
                     0x9E3779B9u, out);
  return (int)hipGetLastError();
}
"""


def sweep_library():
    """the sweep kernel, compiled for gfx950 next to the product library's objects (once)"""
    d = os.path.join(ROOT, "ascii-chat_amd", "build")
    src, so = os.path.join(d, "box_sweep.hip"), os.path.join(d, "libbox_sweep.so")
    os.makedirs(d, exist_ok=True)
    if not os.path.exists(src) or open(src).read() != SWEEP_SRC:
        with open(src, "w") as f:
            f.write(SWEEP_SRC)
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", src, "-o", so])
    return so


def median_us(torch, launch, streams, reps, warm):
    """-> (one at a time, per launch with len(streams) in flight), microseconds"""
    for _ in range(warm):
        for k in range(len(streams)):
            launch(k)
    torch.cuda.synchronize()
    one, many = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(streams[0]):
            a.record()
            launch(0)
            b.record()
        torch.cuda.synchronize()
        one.append(a.elapsed_time(b) * 1e3)
    for _ in range(reps):
        starts, ends = [], []
        for k, s in enumerate(streams):
            with torch.cuda.stream(s):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch(k)
                launch(k)
                b.record()
                starts.append(a)
                ends.append(b)
        torch.cuda.synchronize()
        span = max(starts[i].elapsed_time(ends[j]) for i in range(len(streams)) for j in range(len(streams)))
        many.append(span * 1e3 / (2 * len(streams)))
    return statistics.median(one), statistics.median(many)


def run_shape(name):
    import torch

    import orc
    from __graft_entry__ import load_package
    pkg = load_package()
    assert torch.cuda.is_available() and pkg.lib().asciichat_hip_device_count() > 0, "no GPU: nothing is measured"
    n, w, h, ow, oh = SHAPES[name]
    L = C.CDLL(sweep_library())
    L.sweep.restype = C.c_int
    L.sweep.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    n_streams = 4
    streams = [torch.cuda.Stream() for _ in range(n_streams)]
    frame_bytes = 3 * w * h
    src_bytes = n * frame_bytes
    gen = torch.Generator(device="cuda").manual_seed(1)
    srcs = [torch.randint(0, 256, (src_bytes,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(n_streams)]
    boxes, images, plans, outs, lens = [], [], [], [], []
    for k in range(n_streams):
        frames = [pkg.frame_setup(srcs[k].data_ptr() + i * frame_bytes, w, h, ow, oh, 0, False, False, False) for i in range(n)]
        box = pkg.Box(frames)
        img = torch.zeros(n * box.pitch, dtype=torch.uint8, device="cuda")
        plan = pkg.Plan(pkg.MODE_TRUE_FG, orc.PALETTE_STANDARD, box.render_frames(img.data_ptr()))
        boxes.append(box)
        images.append(img)
        plans.append(plan)
        outs.append(torch.zeros(n * plan.stride, dtype=torch.uint8, device="cuda"))
        lens.append(torch.zeros(n, dtype=torch.int32, device="cuda"))
    sink = torch.zeros(4, dtype=torch.int32, device="cuda")
    spans = [SWEEP_CHUNK * k for k in (1, 2, 4, 8, 16, 32)]  # bytes per workgroup: the best of these is the sweep's figure
    reps, warm = (30, 5) if n > 1 else (200, 20)

    def pass_(k):
        boxes[k].run(images[k].data_ptr(), stream=streams[k].cuda_stream)

    span = [spans[0]]

    def sweep(k):
        assert L.sweep(srcs[k].data_ptr(), src_bytes, span[0], sink.data_ptr(), streams[k].cuda_stream) == 0

    def render(k):
        plans[k].render(outs[k].data_ptr(), plans[k].stride, lens[k].data_ptr(), streams[k].cuda_stream)

    p1, p4 = median_us(torch, pass_, streams, reps, warm)
    tried = []
    for sp in spans:
        span[0] = sp
        tried.append(median_us(torch, sweep, streams, reps, warm) + (sp,))
    s1, s4 = min(t[0] for t in tried), min(t[1] for t in tried)
    r1, r4 = median_us(torch, render, streams, reps, warm)
    floor = src_bytes / HBM * 1e6
    print(f"{name}: {src_bytes / 1e6:.1f} MB of source per launch, uniform form {int(boxes[0].uniform)}, "
          f"render geometry {plans[0].variant}")
    print(f"  pass            one at a time {p1:9.1f} us   four in flight {p4:9.1f} us per launch"
          f"   ({src_bytes / p4 / 1e6:.2f} TB/s)")
    print(f"  read-only sweep one at a time {s1:9.1f} us   four in flight {s4:9.1f} us per launch"
          f"   ({src_bytes / s4 / 1e6:.2f} TB/s; best of spans " + ", ".join(f"{sp // 1024} KiB: {a:.1f} / {b:.1f}" for a, b, sp in tried) + ")")
    print(f"  bytes / 6.3 TB/s             {floor:9.1f} us")
    print(f"  pass / sweep    one at a time {p1 / s1:9.2f}      four in flight {p4 / s4:9.2f}      (aim for the 256-frame shapes: <= 1.25)")
    print(f"  render of the averaged images (truecolor foreground) one at a time {r1:.1f} us, four in flight {r4:.1f} us per launch")
    for b, p in zip(boxes, plans):
        p.close()
        b.close()


def main():
    if "--shape" in sys.argv:
        run_shape(sys.argv[sys.argv.index("--shape") + 1])
        return 0
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    text = ["# area-average downscale pass: scripts/box_downscale_bench.py (HIP events, medians; MI355X)"]
    for name in SHAPES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name], capture_output=True, text=True,
                               timeout=240)
        except subprocess.TimeoutExpired:
            text.append(f"{name}: time limit of 240 s reached; nothing further was run")
            break
        text.append(r.stdout.rstrip())
        if r.returncode != 0:
            text.append(f"{name}: exit status {r.returncode}; nothing further was run\n{r.stderr[-2000:]}")
            break
    body = "\n".join(text) + "\n"
    sys.stdout.write(body)
    if out:
        with open(out, "w") as f:
            f.write(body)
    return 0 if "nothing further was run" not in body else 1


if __name__ == "__main__":
    sys.exit(main())
