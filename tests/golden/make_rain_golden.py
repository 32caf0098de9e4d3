#!/usr/bin/env python3
"""Generator of tests/golden/digital_rain.json and digital_rain_edges.json: the reference's own digital rain pass on recorded
call sequences.

    python3 tests/golden/make_rain_golden.py --reference <ascii-chat source tree> [--sweep-steps N]

Compiles the reference's lib/video/anim/digital_rain.c, lib/video/rgba/color_filter.c and lib/util/utf8.c in a temporary
directory, against stand-in headers written here (logging, memory macros, errno and utf8proc reduced to what these files
need; the reference's own digital_rain.h / color_filter.h / utf8.h are copied next to them), with plain -O2: no fast-math,
no -march.  It then runs sequences of digital_rain_* calls and records, per step, the input, dt, any calls or direct
field writes before the step, the output length and SHA-256 (the full output for the hand-written strings).  Inputs are
frames the oracle (oracle/, tests/orc.py) renders in every mode, padded, with the BLOCKS palette, rainbow-recoloured, and
about thirty hand strings.

digital_rain_edges.json holds the edge cases of tests/rain_cases.py, recorded the same way: every parameter_cases() entry
(but those rain_cases.NOT_IN_FIXTURE names, with the reason) and the chosen boundary cases.  Their inputs are stored as
[hex, times] parts (the run of filler lines once), never the full output, and the final grid is hashed with every NaN
replaced by 0x7FC00000.

Last, it compares the reference with tests/cabi/rain_restatement.c over a sweep (200x60 truecolor frames, several
hundred steps with the blend) and prints how many cells and bytes differ.  Only the fixture is committed; nothing of the
reference is.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import orc  # noqa: E402
import rain_cases as RC  # noqa: E402
import rain_support as RS  # noqa: E402

STANDINS = {
    "ascii-chat/common.h": "#pragma once\n#include <stdbool.h>\n#include <stddef.h>\n#include <stdint.h>\n#include <stdlib.h>\n",
    "ascii-chat/platform/terminal.h": "#pragma once\ntypedef enum { COLOR_FILTER_NONE = 0, COLOR_FILTER_BLACK, COLOR_FILTER_WHITE, "
                                      "COLOR_FILTER_GREEN, COLOR_FILTER_MAGENTA, COLOR_FILTER_FUCHSIA, COLOR_FILTER_ORANGE, "
                                      "COLOR_FILTER_TEAL, COLOR_FILTER_CYAN, COLOR_FILTER_PINK, COLOR_FILTER_RED, "
                                      "COLOR_FILTER_YELLOW, COLOR_FILTER_RAINBOW, COLOR_FILTER_COUNT } color_filter_t;\n",
    "ascii-chat/debug/memory.h": "#pragma once\n#include <stdlib.h>\n#define SAFE_MALLOC(n, T) ((T)malloc(n))\n"
                                 "#define SAFE_CALLOC(k, n, T) ((T)calloc((k), (n)))\n"
                                 "#define SAFE_FREE(p) do { free((void *)(p)); (p) = NULL; } while (0)\n",
    "ascii-chat/log/log.h": "#pragma once\n#define log_error(...) ((void)0)\n#define log_info(...) ((void)0)\n"
                            "#define log_warn(...) ((void)0)\n#define log_debug(...) ((void)0)\n",
    "ascii-chat/asciichat_errno.h": "#pragma once\n#define SET_ERRNO(code, ...) (code)\n",
    "ascii-chat/common/error_codes.h": "#pragma once\nenum { ASCIICHAT_OK = 0, ERROR_MEMORY = 3, ERROR_INVALID_PARAM = 86 };\n",
    "ascii-chat-deps/utf8proc/utf8proc.h": "#pragma once\n#include <stdint.h>\n#include <sys/types.h>\n"
                                           "typedef uint8_t utf8proc_uint8_t; typedef int32_t utf8proc_int32_t; "
                                           "typedef ssize_t utf8proc_ssize_t; typedef int utf8proc_option_t;\n"
                                           "enum { UTF8PROC_CASEFOLD = 1, UTF8PROC_STABLE = 2, UTF8PROC_COMPOSE = 4 };\n"
                                           "utf8proc_ssize_t utf8proc_iterate(const utf8proc_uint8_t *, utf8proc_ssize_t, "
                                           "utf8proc_int32_t *);\nint utf8proc_charwidth(utf8proc_int32_t);\n"
                                           "utf8proc_ssize_t utf8proc_map(const utf8proc_uint8_t *, utf8proc_ssize_t, "
                                           "utf8proc_uint8_t **, utf8proc_option_t);\n",
}
# the utf8proc entry points utf8.c's other functions name (never called by the rain pass)
STUBS = ("#include <ascii-chat-deps/utf8proc/utf8proc.h>\n#include <stdlib.h>\n"
         "utf8proc_ssize_t utf8proc_iterate(const utf8proc_uint8_t *s, utf8proc_ssize_t n, utf8proc_int32_t *c) { abort(); }\n"
         "int utf8proc_charwidth(utf8proc_int32_t c) { abort(); }\n"
         "utf8proc_ssize_t utf8proc_map(const utf8proc_uint8_t *s, utf8proc_ssize_t n, utf8proc_uint8_t **d, "
         "utf8proc_option_t o) { abort(); }\n"
         "#include <strings.h>\nint platform_strcasecmp(const char *a, const char *b) { return strcasecmp(a, b); }\n")


def build_reference(ref, tmp):
    inc = os.path.join(tmp, "include")
    for rel, text in STANDINS.items():
        os.makedirs(os.path.dirname(os.path.join(inc, rel)), exist_ok=True)
        open(os.path.join(inc, rel), "w").write(text)
    for rel in ("ascii-chat/video/anim/digital_rain.h", "ascii-chat/video/rgba/color_filter.h", "ascii-chat/util/utf8.h"):
        os.makedirs(os.path.dirname(os.path.join(inc, rel)), exist_ok=True)
        shutil.copy(os.path.join(ref, "include", rel), os.path.join(inc, rel))
    stubs = os.path.join(tmp, "stubs.c")
    open(stubs, "w").write(STUBS)
    srcs = [os.path.join(ref, p) for p in ("lib/video/anim/digital_rain.c", "lib/video/rgba/color_filter.c", "lib/util/utf8.c")]
    so = os.path.join(tmp, "librefrain.so")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-fPIC", "-shared", "-w", "-I" + inc, *srcs, stubs, "-o", so, "-lm"])
    L = C.CDLL(so)
    P = C.POINTER(RS.RainT)
    for name, res, args in (("digital_rain_init", P, [C.c_int, C.c_int]), ("digital_rain_destroy", None, [P]),
                            ("digital_rain_apply", C.c_void_p, [P, C.c_char_p, C.c_float]), ("digital_rain_reset", None, [P]),
                            ("digital_rain_set_fall_speed", None, [P, C.c_float]),
                            ("digital_rain_set_raindrop_length", None, [P, C.c_float]),
                            ("digital_rain_set_color", None, [P, C.c_uint8, C.c_uint8, C.c_uint8]),
                            ("digital_rain_set_color_from_filter", None, [P, C.c_int])):
        getattr(L, name).restype = res
        getattr(L, name).argtypes = args
    L.free = C.CDLL(None).free
    L.free.argtypes = [C.c_void_p]
    return L


def apply_ops(L, p, ops):
    for op in ops:
        if op[0] == "filter":
            L.digital_rain_set_color_from_filter(p, op[1])
        elif op[0] == "color":
            L.digital_rain_set_color(p, *op[1:])
        elif op[0] == "reset":
            L.digital_rain_reset(p)
        elif op[0] == "fall_speed_call":
            L.digital_rain_set_fall_speed(p, op[1])
        elif op[0] == "raindrop_length_call":
            L.digital_rain_set_raindrop_length(p, op[1])
        else:
            setattr(p.contents, op[0], op[1])


def run_case(L, name, cols, rows, steps, full):
    p = L.digital_rain_init(cols, rows)
    rec = []
    for frame, dt, ops in steps:
        apply_ops(L, p, ops)
        ptr = L.digital_rain_apply(p, frame, dt)
        out = C.string_at(ptr)
        L.free(ptr)
        st = {"input": frame.hex(), "dt": dt, "out_len": len(out), "sha256": hashlib.sha256(out).hexdigest()}
        if ops:
            st["ops"] = ops
        if full:
            st["output"] = out.hex()
        rec.append(st)
    grid = [p.contents.previous_brightness[i] for i in range(cols * rows)]
    L.digital_rain_destroy(p)
    return {"name": name, "cols": cols, "rows": rows, "steps": rec,
            "final_grid_sha256": hashlib.sha256(np.array(grid, dtype=np.float32).tobytes()).hexdigest()}


def run_edge_case(L, case):
    p = L.digital_rain_init(case.cols, case.rows)
    for op in case.ops:
        if op[0] == "color":
            L.digital_rain_set_color(p, *op[1:])
        else:
            setattr(p.contents, op[0], float(op[1]))
    rec = []
    for k, (frame, dt) in enumerate(zip(case.frames, case.dts)):
        ptr = L.digital_rain_apply(p, frame, dt)
        out = C.string_at(ptr)
        L.free(ptr)
        st = {"input_parts": RC.pack_frame(frame), "dt": dt, "out_len": len(out), "sha256": hashlib.sha256(out).hexdigest()}
        if k == 0 and case.ops:
            st["ops"] = case.ops
        rec.append(st)
    grid = [p.contents.previous_brightness[i] for i in range(case.cols * case.rows)]
    L.digital_rain_destroy(p)
    return {"name": case.name, "cols": case.cols, "rows": case.rows, "steps": rec,
            "final_grid_sha256": hashlib.sha256(RC.canonical_grid_bytes(grid)).hexdigest()}


def edge_cases():
    return [c for c in RC.parameter_cases() if c.name not in RC.NOT_IN_FIXTURE] + RC.chosen_boundary_cases()


def oracle_cases():
    img = orc.frame_smooth(160, 96)
    img2 = img.copy()
    img2[20:60, 40:120] = orc.frame_hash_noise(80, 40, 9)
    w, h = 20, 6
    dts = [0.016, 0.033, 0.02]
    cases = []
    modes = [("mono", 0, 0), ("fg16", 1, 0), ("fg256", 2, 0), ("fgtrue", 3, 0), ("bg16", 1, 1), ("bg256", 2, 1),
             ("bgtrue", 3, 1), ("hbmono", 0, 2), ("hb16", 1, 2), ("hb256", 2, 2), ("hbtrue", 3, 2)]
    for name, cl, rm in modes:
        frames = [orc.convert_with_caps(im, w, h, cl, rm) for im in (img, img2)]
        cases.append((name, w, h, [(frames[k % 2], dts[k], []) for k in range(3)]))
    padded = orc.convert_with_caps(img, w, h + 4, 3, 0, wants_padding=True)
    cases.append(("padded_true", w, h + 4, [(padded, 0.02, []), (padded, 0.02, [])]))
    blocks = orc.convert_with_caps(img2, w, h, 3, 0, palette=orc.PALETTE_BLOCKS)
    cases.append(("blocks_true", w, h, [(blocks, 0.02, []), (blocks, 0.05, [])]))
    fr = orc.convert_with_caps(img2, w, h, 3, 0)
    cases.append(("rainbow_rendered", w, h, [(orc.rainbow_replace(fr, 0.7), 0.02, [["filter", 12]]),
                                             (orc.rainbow_replace(fr, 1.9), 0.5, [])]))
    mono80 = orc.convert_with_caps(img2, 80, 24, 0, 0)
    cases.append(("mono_80x24", 80, 24, [(mono80, 0.016, []), (mono80, 0.016, []), (mono80, 0.1, [["reset"]])]))
    return cases


def hand_cases():
    E = b"\x1b"
    s = []
    s.append(("empty", 4, 2, [(b"", 0.1, [])]))
    s.append(("plain", 4, 2, [(b"ab\ncd", 0.1, []), (b"ab\ncd", 0.1, [])]))
    s.append(("empty_digit_runs", 4, 2, [(E + b"[38;2;;;mx" + E + b"[48;2;;5;mY", 0.2, [])]))
    s.append(("sgr_256_kept", 4, 2, [(E + b"[38;5;196mx" + E + b"[48;5;21my", 0.2, [])]))
    s.append(("bare_esc", 4, 2, [(b"a" + E + b"b" + E, 0.2, []), (E + E + b"[31m" + E, 0.1, [])]))
    s.append(("unterminated_csi_across_newline", 4, 3, [(b"ab" + E + b"[12;\n34\nc", 0.3, [])]))
    s.append(("csi_to_end", 4, 2, [(b"x" + E + b"[12;34", 0.3, [])]))
    s.append(("invalid_utf8", 6, 2, [(b"\xff\xc3(\xe2\x82\xa1x\xf0\x9f\x98\x80\x80\xe0\x80", 0.1, [])]))
    s.append(("utf8_valid", 6, 2, [("█▓▒░é😀".encode(), 0.1, []), ("█▓▒░é😀".encode(), 0.1, [])]))
    s.append(("rep_sequence", 6, 2, [(b"a" + E + b"[5bc\n" + E + b"[38;2;1;2;3m#" + E + b"[3b", 0.1, [])]))
    s.append(("grid_narrower_shorter", 3, 2, [(b"abcdef\nghijkl\nmnopqr\nstuvwx", 0.1, []),
                                              (b"abcdef\nghijkl\nmnopqr\nstuvwx", 0.2, [])]))
    s.append(("several_events_per_cell", 4, 2,
              [(E + b"[38;2;200;100;50m" + E + b"[48;2;10;20;30mA" + E + b"[38;2;255;255;255mB\n" + E + b"[38;2;9;9;9m", 0.1, []),
               (E + b"[38;2;200;100;50m" + E + b"[48;2;10;20;30mA" + E + b"[38;2;255;255;255mB\n" + E + b"[38;2;9;9;9m", 0.1, []),
               (E + b"[38;2;200;100;50m" + E + b"[48;2;10;20;30m" + E + b"[38;2;1;1;1m\nz", 0.1, [])]))
    s.append(("colour_event_at_end", 4, 2, [(b"ab" + E + b"[38;2;100;100;100m", 0.1, []),
                                            (b"ab" + E + b"[38;2;100;100;100m", 0.1, [])]))
    s.append(("broken_colour_events", 4, 2, [(E + b"[38;2;1;2m" + E + b"[38;2;1;2;3;4m" + E + b"[38;3;1;2;3mq" + E + b"[39m", 0.1, [])]))
    s.append(("large_digits", 4, 2, [(E + b"[38;2;999;1000;256mx" + E + b"[38;2;000000012;7;0008mz", 0.1, [])]))
    s.append(("only_newlines", 2, 2, [(b"\n\n\n\n", 0.1, [])]))
    s.append(("rows_beyond_grid", 3, 1, [(b"abc\ndef\nghi\njkl", 0.1, []), (b"abc\ndef\nghi\njkl", 0.2, [])]))
    for f in range(13):
        s.append((f"filter_{f}", 4, 2, [(b"ab\ncd", 0.3, [["filter", f]]), (b"ab\ncd", 0.3, [])]))
    s.append(("rainbow_mode_long", 5, 2, [(b"abcde\nfghij", 1.1, [["filter", 12]]), (b"abcde\nfghij", 1.3, []),
                                          (b"abcde\nfghij", 2.0, [["filter", 0]])]))
    s.append(("setters_and_fields", 5, 2, [(b"abcde\nfghij", 0.1, []),
                                           (b"abcde\nfghij", 0.1, [["fall_speed_call", 5.0], ["raindrop_length_call", 4.0]]),
                                           (b"abcde\nfghij", 0.1, [["brightness_decay", 0.5], ["animation_speed", 2.0],
                                                                   ["color", 10, 20, 30]]),
                                           (b"abcde\nfghij", 0.1, [["reset"]]), (b"abcde\nfghij", 0.1, [["first_frame", True]])]))
    s.append(("cursor_heavy_short_drops", 8, 4, [(b"abcdefgh\n" * 4, 0.05, [["raindrop_length_call", 1.5]]),
                                                 (b"abcdefgh\n" * 4, 0.05, [])]))
    return s


def sweep(L, steps):
    """reference vs restatement: 200x60 truecolor frames, `steps` calls with the blend; cells whose stored brightness
    differs after a step (summed over steps) and output bytes that differ"""
    img = orc.frame_smooth(320, 180)
    frames = [orc.convert_with_caps(img, 200, 60, 3, 0), orc.convert_with_caps(np.ascontiguousarray(img[::-1]), 200, 60, 3, 0)]
    p = L.digital_rain_init(200, 60)
    rs = RS.Restated(200, 60)
    cells = cell_diff = byte_diff = steps_diff = 0
    for k in range(steps):
        dt = 0.016 + 0.001 * (k % 7)
        f = frames[k % 2]
        ptr = L.digital_rain_apply(p, f, dt)
        a = C.string_at(ptr)
        L.free(ptr)
        b = rs.apply(f, dt)
        ga = np.ctypeslib.as_array(p.contents.previous_brightness, shape=(12000,))
        gb = np.ctypeslib.as_array(rs.r.previous_brightness, shape=(12000,))
        d = int((ga.view(np.uint32) != gb.view(np.uint32)).sum())
        cells += 12000
        cell_diff += d
        if a != b:
            steps_diff += 1
            byte_diff += sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
    L.digital_rain_destroy(p)
    rs.close()
    return cells, cell_diff, byte_diff, steps_diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference ascii-chat source tree")
    ap.add_argument("--sweep-steps", type=int, default=850)
    ap.add_argument("--out", default=os.path.join(HERE, "digital_rain.json"))
    ap.add_argument("--edges-out", default=os.path.join(HERE, "digital_rain_edges.json"))
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="rain_golden_")
    try:
        L = build_reference(os.path.abspath(a.reference), tmp)
        cases = [run_case(L, n, c, r, st, False) for n, c, r, st in oracle_cases()]
        cases += [run_case(L, n, c, r, st, True) for n, c, r, st in hand_cases()]
        edges = [run_edge_case(L, c) for c in edge_cases()]
        cells, cell_diff, byte_diff, steps_diff = sweep(L, a.sweep_steps)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    doc = {"about": "digital_rain_apply sequences recorded from the reference's own digital_rain.c (make_rain_golden.py)",
           "sweep": {"cells": cells, "cells_differing": cell_diff, "output_bytes_differing": byte_diff,
                     "steps_with_output_difference": steps_diff, "steps": a.sweep_steps, "grid": [200, 60]},
           "cases": cases}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(f"{len(cases)} cases -> {a.out}")
    edoc = {"about": "digital_rain_apply on the edge cases of tests/rain_cases.py (parameter extremes, tokens at the chunk "
                     "boundary and the end of the look-ahead), recorded from the reference's own digital_rain.c "
                     "(make_rain_golden.py).  input_parts: [hex, times] pieces of the input.  Parameter values are text for "
                     "float().  final_grid_sha256 is taken with every NaN canonicalised to the bit pattern 0x7FC00000.",
            "cases": edges}
    with open(a.edges_out, "w") as f:
        json.dump(edoc, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(f"{len(edges)} edge cases -> {a.edges_out}")
    print(f"sweep: {cells} cells over {a.sweep_steps} steps: {cell_diff} stored brightness values differ, "
          f"{byte_diff} output bytes differ ({steps_diff} steps)")


if __name__ == "__main__":
    main()
