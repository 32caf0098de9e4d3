"""The digital rain pass without a GPU: the restatement pinned to the reference-generated fixture, the kernel under the CPU
emulator against the restatement (byte for byte, state for state), and the drop-in ABI of the built library."""
import ctypes as C
import hashlib
import json
import os
import random
import subprocess

import numpy as np

import rain_support as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ascii-chat_amd", "libasciichat_hip.so")
NAMES = ["digital_rain_apply", "digital_rain_destroy", "digital_rain_init", "digital_rain_reset", "digital_rain_set_color",
         "digital_rain_set_color_from_filter", "digital_rain_set_fall_speed", "digital_rain_set_raindrop_length"]


def _fixture():
    return json.load(open(RS.GOLDEN))


def test_restatement_matches_fixture():
    fx = _fixture()
    assert len(fx["cases"]) >= 40
    for case in fx["cases"]:
        r = RS.Restated(case["cols"], case["rows"])
        for k, step in enumerate(case["steps"]):
            RS.apply_ops(r, step.get("ops", []))
            out = r.apply(bytes.fromhex(step["input"]), step["dt"])
            where = f"{case['name']} step {k}"
            if "output" in step:
                assert out == bytes.fromhex(step["output"]), where
            assert len(out) == step["out_len"] and hashlib.sha256(out).hexdigest() == step["sha256"], where
        grid = np.array(r.state(), dtype=np.float32)
        assert hashlib.sha256(grid.tobytes()).hexdigest() == case["final_grid_sha256"], case["name"]
        r.close()


def _both(cols, rows):
    return RS.Emulated(cols, rows), RS.Restated(cols, rows)


def test_kernel_matches_restatement_on_fixture_sequences():
    for case in _fixture()["cases"]:
        e, r = _both(case["cols"], case["rows"])
        for k, step in enumerate(case["steps"]):
            RS.apply_ops(e, step.get("ops", []))
            RS.apply_ops(r, step.get("ops", []))
            f = bytes.fromhex(step["input"])
            got = RS.emu_batch([(e, f, step["dt"])])[0]
            assert got == r.apply(f, step["dt"]), f"{case['name']} step {k}"
            assert e.grid() == r.state(), f"{case['name']} step {k}: grid"
        e.close()
        r.close()


def _fuzz_string(rng, n):
    E = b"\x1b"
    parts = [b"a", b"#", b"\n", E, E + b"[", b"[", b"m", b";", b"38", b"48", b";2;", b"0", b"12", b"255", b"999",
             "█".encode(), "é".encode(), b"\xe2\x96", b"\x80", b"\xff", b"\xf0\x9f\x98\x80", E + b"[0m", E + b"[5b",
             E + b"[38;2;", E + b"[48;2;"]
    out = b""
    while len(out) < n:
        if rng.random() < 0.3:
            out += E + b"[%d8;2;%d;%d;%dm" % (rng.choice([3, 4]), rng.randrange(300), rng.randrange(256), rng.randrange(256))
        else:
            out += rng.choice(parts)
    return out


def test_kernel_matches_restatement_on_fuzz_strings_and_long_frames():
    rng = random.Random(7)
    for trial in range(40):
        cols, rows = rng.randrange(1, 30), rng.randrange(1, 12)
        e, r = _both(cols, rows)
        if trial % 3 == 0:
            for o in (e.s, r.r):
                o.brightness_decay, o.raindrop_length = 0.6, 3.0
        n = rng.choice([5, 60, 700, 5000, 9000])  # beyond 4096: frames span chunks
        for step in range(3):
            f = _fuzz_string(rng, n)
            dt = rng.choice([0.0, 0.016, 0.5, 3.0])
            assert RS.emu_batch([(e, f, dt)])[0] == r.apply(f, dt), f"trial {trial} step {step}: {f!r}"
            assert e.grid() == r.state(), f"trial {trial} step {step}: grid"
        e.close()
        r.close()


def test_nul_ends_the_frame_and_large_grids_compute_on_demand():
    e, r = _both(130, 100)  # 130 x 101 entries: beyond the LDS table
    f = (b"\x1b[38;2;10;20;30m@" * 40 + b"\n") * 3
    for step in range(3):
        assert RS.emu_batch([(e, f + b"\0tail", 0.1)])[0] == r.apply(f, 0.1)
        assert e.grid() == r.state()


def test_multi_frame_batches_mixed_grids_and_overflow_slots():
    rng = random.Random(11)
    grids = [(8, 3), (20, 6), (3, 2), (40, 10), (12, 12)]
    pairs = [_both(*g) for g in grids]
    for step in range(4):
        frames = [_fuzz_string(rng, rng.choice([30, 200, 1500])) for _ in grids]
        dts = [0.02 * (k + 1) for k in range(len(grids))]
        out = RS.emu_batch([(pairs[k][0], frames[k], dts[k]) for k in range(len(grids))])
        for k, (e, r) in enumerate(pairs):
            assert out[k] == r.apply(frames[k], dts[k]), f"step {step} frame {k}"
            assert e.grid() == r.state(), f"step {step} frame {k}: grid"
        # a batch whose middle slot is too small for its frame: that frame reports the overflow and leaves its grid as it
        # was (its host side advances all the same), the others are whole
        f2 = [b"abc\n" * 60 for _ in grids]
        stride = 6144  # room for 240 input bytes (<= 4800 out), not for 960
        e1, r1 = pairs[1]
        big = [(pairs[k][0], f2[k] if k != 1 else f2[k] * 4, 0.05) for k in range(len(grids))]
        out = RS.emu_batch(big, dst_stride=stride, src_stride=1024)
        assert out[1] == RS.LEN_OVERFLOW
        r1.r.time = e1.s.time
        r1.r.first_frame = False
        for k, (e, r) in enumerate(pairs):
            if k != 1:
                assert out[k] == r.apply(f2[k], 0.05), f"step {step} frame {k} beside the overflow"
            assert e.grid() == r.state(), f"step {step} frame {k}: grid beside the overflow"


def test_out_stride_helper_and_abi():
    L = C.CDLL(LIB)
    L.asciichat_hip_rain_out_stride.restype = C.c_size_t
    L.asciichat_hip_rain_out_stride.argtypes = [C.c_size_t, C.c_size_t]
    for src, chars in ((36000, 1944), (0, 0), (100, 7), (1 << 20, 48000)):
        s = L.asciichat_hip_rain_out_stride(src, chars)
        assert s % 128 == 0 and src + 19 * chars + 1 <= s < src + 19 * chars + 1 + 128
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout.split("\n")
    names = sorted(ln.split()[-1] for ln in syms if ln.strip())
    for n in NAMES:
        assert n in names, n
    assert len(names) < 260
    # struct layout: what rain_support mirrors is the reference's digital_rain_t
    assert C.sizeof(RS.RainT) == 56 and C.sizeof(RS.Column) == 12
    assert (RS.RainT.num_rows.offset, RS.RainT.color_r.offset, RS.RainT.cursor_brightness.offset, RS.RainT.rainbow_mode.offset,
            RS.RainT.first_frame.offset, RS.RainT.previous_brightness.offset) == (12, 36, 40, 44, 45, 48)
    # the library's own init fills that layout (no device needed until the first apply)
    L.digital_rain_init.restype = C.POINTER(RS.RainT)
    L.digital_rain_init.argtypes = [C.c_int, C.c_int]
    L.digital_rain_destroy.argtypes = [C.POINTER(RS.RainT)]
    L.digital_rain_set_color_from_filter.argtypes = [C.POINTER(RS.RainT), C.c_int]
    assert not L.digital_rain_init(0, 5) and not L.digital_rain_init(5, -1)
    p = L.digital_rain_init(7, 3)
    ref = RS.Restated(7, 3)
    s, q = p.contents, ref.r
    for f in [n for n, _ in RS.RainT._fields_ if n not in ("columns", "previous_brightness")]:
        assert getattr(s, f) == getattr(q, f), f
    for c in range(7):
        assert (s.columns[c].time_offset, s.columns[c].speed_multiplier, s.columns[c].phase_offset) == \
            (q.columns[c].time_offset, q.columns[c].speed_multiplier, q.columns[c].phase_offset)
    for flt in list(range(13)) + [40]:
        L.digital_rain_set_color_from_filter(p, flt)
        ref.set_color_from_filter(flt)
        assert (s.color_r, s.color_g, s.color_b, s.rainbow_mode) == (q.color_r, q.color_g, q.color_b, q.rainbow_mode), flt
    L.digital_rain_destroy(p)
    ref.close()
