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
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# name, plan mode, the oracle's render mode, palette, source w x h, output w x h
SHAPES = [("half-block truecolor 1080p->80x24", 5, 2, "STANDARD", 1920, 1080, 80, 24),
          ("truecolor-fg BLOCKS palette 1080p->80x24", 1, 0, "BLOCKS", 1920, 1080, 80, 24),
          ("half-block truecolor sampled 400x240->400x120", 5, 2, "STANDARD", 400, 240, 400, 120)]
NARROW = ("truecolor-fg 1080p->80x24 (narrow form)", 1, 0, "STANDARD", 1920, 1080, 80, 24)


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
    import wire_timing as WT
    import zhuf_ref as Z
    import zwide_ref as W

    pkg = load_package()
    assert torch.cuda.is_available() and pkg.lib().asciichat_hip_device_count() > 0, "needs a GPU"
    n = args.frames
    lines = [f"# scripts/zpack_wide_timing.py: {n} frames per launch, {args.reps} launches per figure (median), destination = mapped host memory",
             f"# {torch.cuda.get_device_name(0)}; libzstd {'loaded' if Z.libzstd() is not None else 'absent'}"]
    rate = None
    if not args.narrow:
        rate = WT.pcie_rate()
        lines.append(f"# measured device -> pinned host copy: {rate / 1e9:.1f} GB/s")
    print("\n".join(lines), flush=True)

    streams = [torch.cuda.Stream() for _ in range(4)]
    for name, mode, rm, pal, sw, sh, ow, oh in ([NARROW] if args.narrow else SHAPES):
        batch = WT.Batch(pkg, getattr(orc, "PALETTE_" + pal), WT.smooth_with_noise(orc, sw, sh), mode, rm, ow, oh, n, args.reps, streams)
        batch.buffers(pkg.zpack_scratch_bytes(batch.stride, n) if args.narrow else pkg.zpack_wide_scratch_bytes(batch.stride, n))
        stride, lens, original = batch.stride, batch.lens, batch.original
        packed, zpacked = batch.packed, batch.form(pkg.frame_packets_zpacked if args.narrow else pkg.frame_packets_zpacked_wide)
        one_at_a_time, four_in_flight = batch.one_at_a_time, batch.four_in_flight
        if args.narrow:
            (t_a, lo_a, hi_a), t4 = one_at_a_time(zpacked), four_in_flight(zpacked)
            (t_b, lo_b, hi_b) = one_at_a_time(zpacked)
            print(f"NARROW {name}: one launch at a time {t_a:.1f} us (min {lo_a:.1f}, max {hi_a:.1f}), again {t_b:.1f} us (min {lo_b:.1f}, "
                  f"max {hi_b:.1f}); four in flight {t4:.1f} us; library {os.environ.get('ASCIICHAT_HIP_LIB', 'this tree')}", flush=True)
            return 0
        (t_p1, _, _), (t_z1, _, _) = one_at_a_time(packed), one_at_a_time(zpacked)
        t_p4, t_z4 = four_in_flight(packed), four_in_flight(zpacked)
        sent_len, offs, view = batch.sent(zpacked)
        sent = int(sent_len.sum())
        frames = batch.frames(64)
        for i in (0, len(frames) - 1):  # what was sent is what the restatement sends, and libzstd decodes it
            payload = view[int(offs[i]):int(offs[i]) + int(sent_len[i])].tobytes()
            assert payload == W.wire(frames[i])[0], f"{name}: frame {i} differs from the restatement"
            if int(sent_len[i]) != len(frames[i]) and Z.libzstd() is not None:
                assert Z.zstd_decompress(payload, len(frames[i])) == frames[i]
        ent = WT.entropy_ratio(b"".join(frames))
        z1 = sum(len(Z.zstd_compress(f, 1)) for f in frames) / max(1, sum(len(f) for f in frames)) if Z.libzstd() is not None else None
        (lhs1, rhs1, yes1), (lhs4, rhs4, yes4) = WT.pays(t_z1, sent, t_p1, original, rate), WT.pays(t_z4, sent, t_p4, original, rate)
        block = ["", f"{name}: stride {stride}, original {original} B ({original // n} B/frame), sent {sent} B",
                 f"  sent/original {sent / original:.3f}   order-0 entropy bound (first 64 frames) {ent:.3f}   libzstd level 1 (first 64 frames) "
                 f"{'%.3f' % z1 if z1 is not None else 'n/a'}   frames sent compressed {int((sent_len != lens).sum())}/{n}",
                 f"  one launch at a time : zpacked_wide {t_z1:8.1f} us   packed {t_p1:8.1f} us",
                 f"  four in flight       : zpacked_wide {t_z4:8.1f} us   packed {t_p4:8.1f} us   (wall clock per launch)",
                 f"  the written bytes cross PCIe: {sent / rate * 1e6:.1f} us against {original / rate * 1e6:.1f} us",
                 f"  pays for itself (one at a time) : {lhs1:8.1f} us < {rhs1:8.1f} us ?  {yes1}",
                 f"  pays for itself (four in flight): {lhs4:8.1f} us < {rhs4:8.1f} us ?  {yes4}"]
        lines += block
        print("\n".join(block), flush=True)
        batch.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
