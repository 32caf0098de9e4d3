#!/usr/bin/env python3
"""What the wide zhuf form (asciichat_hip_frame_packets_zpacked_wide) buys on the frames the narrow form cannot
code -- half blocks and a multi-byte palette: per shape the sent / original ratio beside the order-0 entropy bound and libzstd
level 1 on the same bytes, the time of the pass against asciichat_hip_frame_packets_packed on the same slab into mapped host
memory (HIP events, one launch at a time; wall clock over four streams in flight), and zpack_timing.py's verdict
    t_zpacked + sent_bytes / pcie_rate  <  t_packed + original_bytes / pcie_rate.
--narrow times the NARROW form alone on the truecolor 1080p->80x24 shape and prints one line: run it alternately against two
builds of the library (ASCIICHAT_HIP_LIB) to compare them.

Usage: zpack_wide_timing.py [--frames 256] [--reps 30] [--out profiles/zpack_wide_timing.txt] [--narrow]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# name, plan mode, the oracle's render mode, palette, source w x h, output w x h
SHAPES = [("half-block truecolor 1080p->80x24", 5, 2, "STANDARD", 1920, 1080, 80, 24),
          ("truecolor-fg BLOCKS palette 1080p->80x24", 1, 0, "BLOCKS", 1920, 1080, 80, 24),
          ("half-block truecolor sampled 400x240->400x120", 5, 2, "STANDARD", 400, 240, 400, 120)]
NARROW = ("truecolor-fg 1080p->80x24 (narrow form)", 1, 0, "STANDARD", 1920, 1080, 80, 24)
DISTINCT = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--narrow", action="store_true")
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    import orc
    import zhuf_ref as Z
    import zwide_ref as W
    from zpack_timing import entropy_ratio

    pkg = load_package()
    lib = pkg.lib()
    assert torch.cuda.is_available() and lib.asciichat_hip_device_count() > 0, "needs a GPU"
    n = args.frames
    lines = [f"# scripts/zpack_wide_timing.py: {n} frames per launch, {args.reps} launches per figure (median), destination = mapped host memory",
             f"# {torch.cuda.get_device_name(0)}; libzstd {'loaded' if Z.libzstd() is not None else 'absent'}"]
    rate = None
    if not args.narrow:  # the PCIe rate a device -> pinned host copy reaches (64 MB, median of 10)
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
    print("\n".join(lines), flush=True)

    streams = [torch.cuda.Stream() for _ in range(4)]
    for name, mode, rm, pal, sw, sh, ow, oh in ([NARROW] if args.narrow else SHAPES):
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
        plan = pkg.Plan(mode, getattr(orc, "PALETTE_" + pal), fs)
        stride = plan.stride
        slab = torch.zeros(n * stride + 16, dtype=torch.uint8, device="cuda")
        ln = torch.zeros(n, dtype=torch.int32, device="cuda")
        plan.render(slab.data_ptr(), stride, ln.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        lens = ln.cpu().numpy().view(np.uint32)
        original = int(lens.sum())
        cap = int(((lens.astype(np.int64) + 15) // 16 * 16).sum()) + 4096  # what the frames take at their exact lengths
        d = torch.from_numpy(np.array([(ow, oh)] * n, dtype=np.uint32).view(np.int32)).cuda()
        sbytes = pkg.zpack_scratch_bytes(stride, n) if args.narrow else pkg.zpack_wide_scratch_bytes(stride, n)

        def buffers():
            return dict(host=pkg.HostBuffer(cap), off=torch.zeros(n + 1, dtype=torch.int64, device="cuda"),
                        lo=torch.zeros(n, dtype=torch.int32, device="cuda"), crc=torch.zeros(n, dtype=torch.int32, device="cuda"),
                        pkt=torch.zeros(n, dtype=torch.int32, device="cuda"), hdr=torch.zeros(24 * n, dtype=torch.uint8, device="cuda"),
                        scratch=torch.zeros(sbytes // 8 + 1, dtype=torch.int64, device="cuda"))

        bufs = [buffers() for _ in range(4)]

        def packed(b, s):
            rc = lib.asciichat_hip_frame_packets_packed(slab.data_ptr(), stride, ln.data_ptr(), stride, n, d.data_ptr(), b["crc"].data_ptr(),
                                                        b["hdr"].data_ptr(), b["pkt"].data_ptr(), b["host"].dev, cap, b["off"].data_ptr(),
                                                        b["lo"].data_ptr(), s)
            assert rc == 0, pkg.last_error()

        def zpacked(b, s):
            fn = pkg.frame_packets_zpacked if args.narrow else pkg.frame_packets_zpacked_wide
            fn(slab.data_ptr(), stride, ln.data_ptr(), stride, n, d.data_ptr(), b["crc"].data_ptr(), b["hdr"].data_ptr(), b["pkt"].data_ptr(),
               b["host"].dev, cap, b["off"].data_ptr(), b["lo"].data_ptr(), b["scratch"].data_ptr(), sbytes, s)

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
            return statistics.median(ts), min(ts), max(ts)

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

        if args.narrow:
            (t_a, lo_a, hi_a), t4 = one_at_a_time(zpacked), four_in_flight(zpacked)
            (t_b, lo_b, hi_b) = one_at_a_time(zpacked)
            print(f"NARROW {name}: one launch at a time {t_a:.1f} us (min {lo_a:.1f}, max {hi_a:.1f}), again {t_b:.1f} us (min {lo_b:.1f}, "
                  f"max {hi_b:.1f}); four in flight {t4:.1f} us; library {os.environ.get('ASCIICHAT_HIP_LIB', 'this tree')}", flush=True)
            return 0
        (t_p1, _, _), (t_z1, _, _) = one_at_a_time(packed), one_at_a_time(zpacked)
        t_p4, t_z4 = four_in_flight(packed), four_in_flight(zpacked)
        zpacked(bufs[0], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        sent_len = bufs[0]["lo"].cpu().numpy().view(np.uint32)
        offs = bufs[0]["off"].cpu().numpy()
        sent = int(sent_len.sum())
        view = bufs[0]["host"].view()
        host_slab = slab.cpu().numpy()
        frames = [host_slab[i * stride:i * stride + int(lens[i])].tobytes() for i in range(min(n, 64))]
        for i in (0, len(frames) - 1):  # what was sent is what the restatement sends, and libzstd decodes it
            payload = view[int(offs[i]):int(offs[i]) + int(sent_len[i])].tobytes()
            assert payload == W.wire(frames[i])[0], f"{name}: frame {i} differs from the restatement"
            if int(sent_len[i]) != len(frames[i]) and Z.libzstd() is not None:
                assert Z.zstd_decompress(payload, len(frames[i])) == frames[i]
        ent = entropy_ratio(b"".join(frames))
        z1 = sum(len(Z.zstd_compress(f, 1)) for f in frames) / max(1, sum(len(f) for f in frames)) if Z.libzstd() is not None else None
        lhs1, rhs1 = t_z1 + sent / rate * 1e6, t_p1 + original / rate * 1e6
        lhs4, rhs4 = t_z4 + sent / rate * 1e6, t_p4 + original / rate * 1e6
        block = ["", f"{name}: stride {stride}, original {original} B ({original // n} B/frame), sent {sent} B",
                 f"  sent/original {sent / original:.3f}   order-0 entropy bound (first 64 frames) {ent:.3f}   libzstd level 1 (first 64 frames) "
                 f"{'%.3f' % z1 if z1 is not None else 'n/a'}   frames sent compressed {int((sent_len != lens).sum())}/{n}",
                 f"  one launch at a time : zpacked_wide {t_z1:8.1f} us   packed {t_p1:8.1f} us",
                 f"  four in flight       : zpacked_wide {t_z4:8.1f} us   packed {t_p4:8.1f} us   (wall clock per launch)",
                 f"  the written bytes cross PCIe: {sent / rate * 1e6:.1f} us against {original / rate * 1e6:.1f} us",
                 f"  pays for itself (one at a time) : {lhs1:8.1f} us < {rhs1:8.1f} us ?  {'YES' if lhs1 < rhs1 else 'NO'}",
                 f"  pays for itself (four in flight): {lhs4:8.1f} us < {rhs4:8.1f} us ?  {'YES' if lhs4 < rhs4 else 'NO'}"]
        lines += block
        print("\n".join(block), flush=True)
        for b in bufs:
            b["host"].close()
        plan.close()
        del dev, slab, bufs
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
