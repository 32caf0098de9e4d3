#!/usr/bin/env python3
"""What compressing rendered frames on the device (asciichat_hip_frame_packets_zpacked) buys on real renders:
per mode the sent / original ratio beside the order-0 entropy bound and libzstd level 1 on the same bytes, the time of the
pass against asciichat_hip_frame_packets_packed on the same slab into mapped host memory (HIP events, one launch at a time;
wall clock over four streams in flight), the traffic floor, and the verdict: the pass pays for itself when
    t_zpacked + sent_bytes / pcie_rate  <  t_packed + original_bytes / pcie_rate.

Usage: zpack_timing.py [--frames 256] [--reps 30] [--out profiles/zpack_timing.txt]
"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name, plan mode, the oracle's render mode, source w x h, output w x h
MODES = [("truecolor-fg 1080p->80x24", 1, 0, 1920, 1080, 80, 24),
         ("truecolor-fg sampled 200x60", 1, 0, 200, 60, 200, 60),
         ("ansi-256-fg 1080p->80x24", 2, 0, 1920, 1080, 80, 24),
         ("mono 1080p->80x24", 0, 0, 1920, 1080, 80, 24),
         ("half-block truecolor 1080p->80x48", 5, 2, 1920, 1080, 80, 48)]
DISTINCT = 16  # source images; the batch cycles through them


def entropy_ratio(data):
    counts = np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=256).astype(np.float64)
    p = counts[counts > 0] / len(data)
    return float(-(p * np.log2(p)).sum() / 8.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    import orc
    import zhuf_ref as Z

    pkg = load_package()
    lib = pkg.lib()
    assert torch.cuda.is_available() and lib.asciichat_hip_device_count() > 0, "needs a GPU"
    n = args.frames
    lines = [f"# scripts/zpack_timing.py: {n} frames per launch, {args.reps} launches per figure (median), destination = mapped host memory",
             f"# {torch.cuda.get_device_name(0)}; libzstd {'loaded' if Z.libzstd() is not None else 'absent'}"]

    # the PCIe rate a device -> pinned host copy reaches (64 MB, median of 10)
    big = torch.zeros(64 << 20, dtype=torch.uint8, device="cuda")
    pinned = torch.zeros(64 << 20, dtype=torch.uint8).pin_memory()
    ts = []
    for _ in range(10):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pinned.copy_(big, non_blocking=True)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    rate = (64 << 20) / statistics.median(ts)
    lines.append(f"# measured device -> pinned host copy: {rate / 1e9:.1f} GB/s")
    del big, pinned

    streams = [torch.cuda.Stream() for _ in range(4)]
    for name, mode, rm, sw, sh, ow, oh in MODES:
        rng = np.random.default_rng(1)
        imgs = []
        for k in range(DISTINCT):
            img = orc.frame_smooth(sw, sh).copy()
            x0, y0 = int(rng.integers(0, sw // 2)), int(rng.integers(0, sh // 2))
            img[y0:y0 + sh // 3, x0:x0 + sw // 3] = orc.frame_hash_noise(sw // 3, sh // 3, 100 + k)
            img = np.roll(img, 37 * k, axis=1)
            imgs.append(np.ascontiguousarray(img))
        dev = torch.from_numpy(np.stack(imgs)).cuda()
        fs = [pkg.frame_setup(dev.data_ptr() + (i % DISTINCT) * sw * sh * 3, sw, sh, ow, oh, rm, False, False, False) for i in range(n)]
        plan = pkg.Plan(mode, orc.PALETTE_STANDARD, fs)
        stride = plan.stride
        slab = torch.zeros(n * stride + 16, dtype=torch.uint8, device="cuda")
        ln = torch.zeros(n, dtype=torch.int32, device="cuda")
        plan.render(slab.data_ptr(), stride, ln.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        lens = ln.cpu().numpy().view(np.uint32)
        host_slab = slab.cpu().numpy()
        frames = [host_slab[i * stride:i * stride + int(lens[i])].tobytes() for i in range(n)]
        original = int(lens.sum())
        d = torch.from_numpy(np.array([(ow, oh)] * n, dtype=np.uint32).view(np.int32)).cuda()
        sbytes = pkg.zpack_scratch_bytes(stride, n)

        def buffers():
            return dict(host=pkg.HostBuffer(n * stride), off=torch.zeros(n + 1, dtype=torch.int64, device="cuda"),
                        lo=torch.zeros(n, dtype=torch.int32, device="cuda"), crc=torch.zeros(n, dtype=torch.int32, device="cuda"),
                        pkt=torch.zeros(n, dtype=torch.int32, device="cuda"), hdr=torch.zeros(24 * n, dtype=torch.uint8, device="cuda"),
                        scratch=torch.zeros(sbytes // 8 + 1, dtype=torch.int64, device="cuda"))

        bufs = [buffers() for _ in range(4)]

        def packed(b, s):
            rc = lib.asciichat_hip_frame_packets_packed(slab.data_ptr(), stride, ln.data_ptr(), stride, n, d.data_ptr(), b["crc"].data_ptr(),
                                                        b["hdr"].data_ptr(), b["pkt"].data_ptr(), b["host"].dev, n * stride,
                                                        b["off"].data_ptr(), b["lo"].data_ptr(), s)
            assert rc == 0, pkg.last_error()

        def zpacked(b, s):
            pkg.frame_packets_zpacked(slab.data_ptr(), stride, ln.data_ptr(), stride, n, d.data_ptr(), b["crc"].data_ptr(), b["hdr"].data_ptr(),
                                      b["pkt"].data_ptr(), b["host"].dev, n * stride, b["off"].data_ptr(), b["lo"].data_ptr(),
                                      b["scratch"].data_ptr(), sbytes, s)

        def one_at_a_time(fn):
            s = torch.cuda.current_stream().cuda_stream
            ts = []
            for r in range(args.reps + 3):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn(bufs[0], s)
                b.record()
                torch.cuda.synchronize()
                if r >= 3:
                    ts.append(a.elapsed_time(b) * 1e3)
            return statistics.median(ts)

        def four_in_flight(fn):
            ts = []
            for r in range(args.reps // 3 + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(4):
                    for b, st in zip(bufs, streams):
                        fn(b, st.cuda_stream)
                torch.cuda.synchronize()
                if r >= 2:
                    ts.append((time.perf_counter() - t0) * 1e6 / 16)
            return statistics.median(ts)

        t_p1, t_z1 = one_at_a_time(packed), one_at_a_time(zpacked)
        t_p4, t_z4 = four_in_flight(packed), four_in_flight(zpacked)
        zpacked(bufs[0], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        sent_len = bufs[0]["lo"].cpu().numpy().view(np.uint32)
        offs = bufs[0]["off"].cpu().numpy()
        sent = int(sent_len.sum())
        view = bufs[0]["host"].view()
        for i in (0, n // 2, n - 1):  # what was sent is what the restatement sends, and decodes
            payload = view[int(offs[i]):int(offs[i]) + int(sent_len[i])].tobytes()
            assert payload == Z.wire(frames[i])[0], f"{name}: frame {i} differs from the restatement"
            if int(sent_len[i]) != len(frames[i]):
                assert Z.decode(payload) == frames[i]
        allb = b"".join(frames)
        ent = entropy_ratio(allb)
        z1 = sum(len(Z.zstd_compress(f, 1)) for f in frames[:64]) / max(1, sum(len(f) for f in frames[:64])) if Z.libzstd() is not None else None
        floor_bytes = 2 * original + sent
        lhs1, rhs1 = t_z1 + sent / rate * 1e6, t_p1 + original / rate * 1e6
        lhs4, rhs4 = t_z4 + sent / rate * 1e6, t_p4 + original / rate * 1e6
        block = ["", f"{name}: stride {stride}, original {original} B ({original // n} B/frame), sent {sent} B",
                  f"  sent/original {sent / original:.3f}   order-0 entropy bound {ent:.3f}   libzstd level 1 (first 64 frames) "
                  f"{'%.3f' % z1 if z1 is not None else 'n/a'}   frames sent compressed {int((sent_len != lens).sum())}/{n}",
                  f"  one launch at a time : zpacked {t_z1:8.1f} us   packed {t_p1:8.1f} us",
                  f"  four in flight       : zpacked {t_z4:8.1f} us   packed {t_p4:8.1f} us   (wall clock per launch)",
                  f"  traffic floor        : 2 x {original} B read + {sent} B written = {floor_bytes} B"
                  f" ({floor_bytes / 4.0e12 * 1e6:.1f} us at 4 TB/s of HBM; the written bytes cross PCIe: {sent / rate * 1e6:.1f} us)",
                  f"  pays for itself (one at a time) : {lhs1:8.1f} us < {rhs1:8.1f} us ?  {'YES' if lhs1 < rhs1 else 'NO'}",
                  f"  pays for itself (four in flight): {lhs4:8.1f} us < {rhs4:8.1f} us ?  {'YES' if lhs4 < rhs4 else 'NO'}"]
        lines += block
        print("\n".join(block), flush=True)
        for b in bufs:
            b["host"].close()
        plan.close()
        del dev, slab
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
