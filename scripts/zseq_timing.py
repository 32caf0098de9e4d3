#!/usr/bin/env python3
"""What the sequence form of the zstd wire pass (asciichat_hip_frame_packets_zpacked_seq) buys over the wide zhuf
form and over the uncompressed packed form: per shape and input the sent / original ratio of both compressed forms beside libzstd
level 1 on the same bytes, the time of each pass on the same slab into mapped host memory (HIP events, one launch at a time;
wall clock over four streams in flight), and zpack_timing.py's verdict
    t_form + sent_bytes / pcie_rate  <  t_packed + original_bytes / pcie_rate.
--cpu computes the ratios alone, with the restatements (tests/zseq_ref.py, tests/zwide_ref.py) over the oracle's renders of the
same shapes and inputs: no GPU, no timing.

Usage: zseq_timing.py [--frames 256] [--reps 30] [--out profiles/zseq_timing.txt] [--shapes 0,1,2,3,4] [--inputs noise,smooth] [--cpu]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import wire_timing as WT  # noqa: E402

# name, plan mode, the oracle's colour level and render mode, source w x h, output w x h
SHAPES = [("truecolor-fg 1080p->80x24", 1, 3, 0, 1920, 1080, 80, 24),
          ("truecolor-fg sampled 200x60->200x60", 1, 3, 0, 200, 60, 200, 60),
          ("ANSI-256 fg 1080p->80x24", 2, 2, 0, 1920, 1080, 80, 24),
          ("half-block truecolor 1080p->80x24", 5, 3, 2, 1920, 1080, 80, 24),
          ("half-block truecolor sampled 400x240->400x120", 5, 3, 2, 400, 240, 400, 120)]
DISTINCT = WT.DISTINCT


def sources(orc, kind, sw, sh):
    """DISTINCT source images: S-noise (the metric's input: every cell changes colour) or S-smooth shifted from image to image"""
    if kind == "noise":
        return [orc.frame_hash_noise(sw, sh, 100 + k) for k in range(DISTINCT)]
    return [np.ascontiguousarray(np.roll(orc.frame_smooth(sw, sh), 37 * k, axis=1)) for k in range(DISTINCT)]


def cpu_ratios(args):
    import orc
    import zhuf_ref as Z
    import zseq_ref as S
    import zwide_ref as W
    lines = ["# scripts/zseq_timing.py --cpu: sent / original of the restatements over the oracle's renders (2 images per shape and input)"]
    for k in args.shapes:
        name, _, cl, rm, sw, sh, ow, oh = SHAPES[k]
        for kind in args.inputs:
            frames = [orc.convert_with_caps(img, ow, oh, cl, rm, False, False, False) for img in sources(orc, kind, sw, sh)[:2]]
            total = sum(len(f) for f in frames)
            seq, wide = sum(len(S.wire(f)[0]) for f in frames), sum(len(W.wire(f)[0]) for f in frames)
            z1 = sum(len(Z.zstd_compress(f, 1)) for f in frames) / total if Z.libzstd() is not None else None
            lines.append(f"{name:48s} S-{kind:6s} {total // len(frames):8d} B/frame   zseq {seq / total:.3f}   wide zhuf {wide / total:.3f}   "
                         f"libzstd level 1 {'%.3f' % z1 if z1 is not None else 'n/a'}")
            print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="0,1,2,3,4")
    ap.add_argument("--inputs", default="noise,smooth")
    ap.add_argument("--cpu", action="store_true")
    args = ap.parse_args()
    args.shapes = [int(x) for x in args.shapes.split(",")]
    args.inputs = args.inputs.split(",")
    if args.cpu:
        lines = cpu_ratios(args)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return 0
    import torch
    from __graft_entry__ import load_package
    import orc
    import zhuf_ref as Z
    import zseq_ref as S

    pkg = load_package()
    assert torch.cuda.is_available() and pkg.lib().asciichat_hip_device_count() > 0, "needs a GPU"
    n = args.frames
    lines = [f"# scripts/zseq_timing.py: {n} frames per launch, {args.reps} launches per figure (median), destination = mapped host memory",
             f"# {torch.cuda.get_device_name(0)}; libzstd {'loaded' if Z.libzstd() is not None else 'absent'}; blocks of {S.PIECE} bytes"]
    rate = WT.pcie_rate()
    lines.append(f"# measured device -> pinned host copy: {rate / 1e9:.1f} GB/s")
    print("\n".join(lines), flush=True)

    streams = [torch.cuda.Stream() for _ in range(4)]
    for k in args.shapes:
        name, mode, _, rm, sw, sh, ow, oh = SHAPES[k]
        for kind in args.inputs:
            batch = WT.Batch(pkg, orc.PALETTE_STANDARD, sources(orc, kind, sw, sh), mode, rm, ow, oh, n, args.reps, streams)
            batch.buffers(max(pkg.zpack_seq_scratch_bytes(batch.stride, n), pkg.zpack_wide_scratch_bytes(batch.stride, n)))
            stride, lens, original = batch.stride, batch.lens, batch.original
            packed, wide, seq = batch.packed, batch.form(pkg.frame_packets_zpacked_wide), batch.form(pkg.frame_packets_zpacked_seq)
            t1 = {w: batch.one_at_a_time(fn)[0] for w, fn in (("packed", packed), ("wide", wide), ("seq", seq))}
            t4 = {w: batch.four_in_flight(fn) for w, fn in (("packed", packed), ("wide", wide), ("seq", seq))}
            frames = batch.frames(DISTINCT)
            sent = {}
            for w, fn in (("wide", wide), ("seq", seq)):
                sent_len, offs, view = batch.sent(fn)
                sent[w] = (int(sent_len.sum()), int((sent_len != lens).sum()))
                if w == "seq":  # what was sent is what the restatement sends, and libzstd decodes it
                    for i in (0, len(frames) - 1):
                        payload = view[int(offs[i]):int(offs[i]) + int(sent_len[i])].tobytes()
                        assert payload == S.wire(frames[i])[0], f"{name}: frame {i} differs from the restatement"
                        if int(sent_len[i]) != len(frames[i]) and Z.libzstd() is not None:
                            assert Z.zstd_decompress(payload, len(frames[i])) == frames[i]
            z1 = sum(len(Z.zstd_compress(f, 1)) for f in frames) / max(1, sum(len(f) for f in frames)) if Z.libzstd() is not None else None
            block = ["", f"{name}, S-{kind}: stride {stride}, original {original} B ({original // n} B/frame)",
                     f"  sent/original: zseq {sent['seq'][0] / original:.3f} ({sent['seq'][1]}/{n} frames compressed)   wide zhuf "
                     f"{sent['wide'][0] / original:.3f} ({sent['wide'][1]}/{n})   libzstd level 1 (first {len(frames)} frames) "
                     f"{'%.3f' % z1 if z1 is not None else 'n/a'}",
                     f"  one launch at a time : zpacked_seq {t1['seq']:8.1f} us   zpacked_wide {t1['wide']:8.1f} us   packed {t1['packed']:8.1f} us",
                     f"  four in flight       : zpacked_seq {t4['seq']:8.1f} us   zpacked_wide {t4['wide']:8.1f} us   packed {t4['packed']:8.1f} us   "
                     f"(wall clock per launch)"]
            for w, label in (("seq", "zseq"), ("wide", "wide")):
                lhs1, rhs1, yes1 = WT.pays(t1[w], sent[w][0], t1["packed"], original, rate)
                lhs4, rhs4, yes4 = WT.pays(t4[w], sent[w][0], t4["packed"], original, rate)
                block.append(f"  {label} pays for itself against packed: one at a time {lhs1:8.1f} us < {rhs1:8.1f} us ? {yes1}   "
                             f"four in flight {lhs4:8.1f} us < {rhs4:8.1f} us ? {yes4}")
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
