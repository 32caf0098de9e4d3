#!/usr/bin/env python3
"""What compressing rendered frames on the device (asciichat_hip_frame_packets_zpacked) buys on real renders:
per mode the sent / original ratio beside the order-0 entropy bound and libzstd level 1 on the same bytes, the time of the
pass against asciichat_hip_frame_packets_packed on the same slab into mapped host memory (HIP events, one launch at a time;
wall clock over four streams in flight), the traffic floor, and the verdict: the pass pays for itself when
    t_zpacked + sent_bytes / pcie_rate  <  t_packed + original_bytes / pcie_rate.

Usage: zpack_timing.py [--frames 256] [--reps 30] [--out profiles/zpack_timing.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# name, plan mode, the oracle's render mode, source w x h, output w x h
MODES = [("truecolor-fg 1080p->80x24", 1, 0, 1920, 1080, 80, 24),
         ("truecolor-fg sampled 200x60", 1, 0, 200, 60, 200, 60),
         ("ansi-256-fg 1080p->80x24", 2, 0, 1920, 1080, 80, 24),
         ("mono 1080p->80x24", 0, 0, 1920, 1080, 80, 24),
         ("half-block truecolor 1080p->80x48", 5, 2, 1920, 1080, 80, 48)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    import orc
    import wire_timing as WT
    import zhuf_ref as Z

    pkg = load_package()
    assert torch.cuda.is_available() and pkg.lib().asciichat_hip_device_count() > 0, "needs a GPU"
    n = args.frames
    lines = [f"# scripts/zpack_timing.py: {n} frames per launch, {args.reps} launches per figure (median), destination = mapped host memory",
             f"# {torch.cuda.get_device_name(0)}; libzstd {'loaded' if Z.libzstd() is not None else 'absent'}"]
    rate = WT.pcie_rate()
    lines.append(f"# measured device -> pinned host copy: {rate / 1e9:.1f} GB/s")

    streams = [torch.cuda.Stream() for _ in range(4)]
    for name, mode, rm, sw, sh, ow, oh in MODES:
        batch = WT.Batch(pkg, orc.PALETTE_STANDARD, WT.smooth_with_noise(orc, sw, sh), mode, rm, ow, oh, n, args.reps, streams, exact_capacity=False)
        batch.buffers(pkg.zpack_scratch_bytes(batch.stride, n))
        stride, lens, original = batch.stride, batch.lens, batch.original
        frames = batch.frames(n)
        packed, zpacked = batch.packed, batch.form(pkg.frame_packets_zpacked)
        (t_p1, _, _), (t_z1, _, _) = batch.one_at_a_time(packed), batch.one_at_a_time(zpacked)
        t_p4, t_z4 = batch.four_in_flight(packed), batch.four_in_flight(zpacked)
        sent_len, offs, view = batch.sent(zpacked)
        sent = int(sent_len.sum())
        for i in (0, n // 2, n - 1):  # what was sent is what the restatement sends, and decodes
            payload = view[int(offs[i]):int(offs[i]) + int(sent_len[i])].tobytes()
            assert payload == Z.wire(frames[i])[0], f"{name}: frame {i} differs from the restatement"
            if int(sent_len[i]) != len(frames[i]):
                assert Z.decode(payload) == frames[i]
        allb = b"".join(frames)
        ent = WT.entropy_ratio(allb)
        z1 = sum(len(Z.zstd_compress(f, 1)) for f in frames[:64]) / max(1, sum(len(f) for f in frames[:64])) if Z.libzstd() is not None else None
        floor_bytes = 2 * original + sent
        (lhs1, rhs1, yes1), (lhs4, rhs4, yes4) = WT.pays(t_z1, sent, t_p1, original, rate), WT.pays(t_z4, sent, t_p4, original, rate)
        block = ["", f"{name}: stride {stride}, original {original} B ({original // n} B/frame), sent {sent} B",
                  f"  sent/original {sent / original:.3f}   order-0 entropy bound {ent:.3f}   libzstd level 1 (first 64 frames) "
                  f"{'%.3f' % z1 if z1 is not None else 'n/a'}   frames sent compressed {int((sent_len != lens).sum())}/{n}",
                  f"  one launch at a time : zpacked {t_z1:8.1f} us   packed {t_p1:8.1f} us",
                  f"  four in flight       : zpacked {t_z4:8.1f} us   packed {t_p4:8.1f} us   (wall clock per launch)",
                  f"  traffic floor        : 2 x {original} B read + {sent} B written = {floor_bytes} B"
                  f" ({floor_bytes / 4.0e12 * 1e6:.1f} us at 4 TB/s of HBM; the written bytes cross PCIe: {sent / rate * 1e6:.1f} us)",
                  f"  pays for itself (one at a time) : {lhs1:8.1f} us < {rhs1:8.1f} us ?  {yes1}",
                  f"  pays for itself (four in flight): {lhs4:8.1f} us < {rhs4:8.1f} us ?  {yes4}"]
        lines += block
        print("\n".join(block), flush=True)
        batch.close()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
