"""The digital rain pass at its boundaries and parameter extremes, without a GPU: the restatement pinned to the reference's
own pass on the edge cases (golden/digital_rain_edges.json), and the kernel under the CPU emulator against the restatement
on every case of rain_cases.py, output bytes equal and stored brightness equal bit for bit (or NaN on both sides).

The boundary sweep costs about 14 ms per emulated 4 KB chunk, some 40 000 of them: it is cut into jobs that run in worker
processes (the emulator is one process's state), at most 8: fresh interpreters running this file, not forks of the
test process, whose size by then is whatever the suite in front of it left.
"""
import hashlib
import json
import os
import subprocess
import sys

import rain_cases as RC
import rain_support as RS

WORKERS = max(1, min(8, os.cpu_count() or 1))
BATCH = 32
BIG_GRID = (130, 100)  # 130 x 101 entries: beyond ACHIP_RAIN_TABLE_MAX, brightness computed on demand
_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = RC.boundary_cases()
    return _cases


def _pair(c, grid=None):
    cols, rows = grid or (c.cols, c.rows)
    e, r = RS.Emulated(cols, rows), RS.Restated(cols, rows)
    for o in (e, r):
        RC.apply_case_ops(o, c.ops)
    return e, r


def _close(pairs):
    for e, r in pairs:
        e.close()
        r.close()


def _parallel(kind):
    """the jobs of JOBS[kind], job w of every WORKERS in worker w"""
    RS.emulator(), RS.restatement()  # built once, in front of the workers
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), kind, str(w), str(WORKERS)], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for w in range(WORKERS)]
    said = [p.communicate()[0].decode("utf-8", "replace") for p in procs]
    failed = [f"worker {w} (exit {p.returncode}): {said[w][-3000:]}" for w, p in enumerate(procs) if p.returncode != 0]
    assert not failed, "\n".join(failed)
    assert sum(int(s.split()[-1]) for s in said) == len(JOBS[kind][1]())  # every job ran


def _run_sequences(cs, pairs, tight):
    """every step of cases cs as one launch per step; tight: the slot stride is the longest output and its NUL, rounded
    up to 16, instead of 20 bytes per input byte"""
    for k in range(max(len(c.frames) for c in cs)):
        live = [(p, c) for p, c in zip(pairs, cs) if k < len(c.frames)]
        want = [r.apply(c.frames[k], c.dts[k]) for (e, r), c in live]
        stride = (max(len(w) for w in want) + 1 + 15) // 16 * 16 if tight else None
        got = RS.emu_batch([(e, c.frames[k], c.dts[k]) for (e, r), c in live], dst_stride=stride)
        for ((e, r), c), g, w in zip(live, got, want):
            assert g != RS.LEN_OVERFLOW, f"{c.name} step {k}: overflow in a slot of {stride}"
            RC.check(g, w, e.grid(), r.state(), f"{c.name} step {k}", e.cols)


def _job_plain(idx):
    cs = [cases()[i] for i in idx]
    pairs = [_pair(c) for c in cs]
    _run_sequences(cs, pairs, tight=False)
    _close(pairs)


def _job_mixed(job):
    idx, big = job
    cs = [cases()[i] for i in idx]
    pairs = [_pair(c) for c in cs]
    cs.insert(len(cs) // 2, cases()[big])
    pairs.insert(len(pairs) // 2, _pair(cases()[big], BIG_GRID))
    _run_sequences(cs, pairs, tight=True)
    _close(pairs)


def _jobs_plain():
    n = len(cases())
    return [list(range(lo, min(lo + BATCH, n))) for lo in range(0, n, BATCH)]


def _jobs_mixed():
    n = len(cases())
    nb = (n + BATCH - 1) // BATCH
    long_ones = [i for i, c in enumerate(cases()) if RC.TOKENS[c.name.split("@")[0]][1] and "@16" not in c.name]
    return [(list(range(j, n, nb)), long_ones[(j * 53) % len(long_ones)]) for j in range(nb)]


def _jobs_slots():
    idx = [i for i, c in enumerate(cases()) if "@end" in c.name]
    return [idx[lo:lo + 16] for lo in range(0, len(idx), 16)]


def test_restatement_matches_edges_fixture():
    fx = json.load(open(RS.GOLDEN_EDGES))
    names = [c["name"] for c in fx["cases"]]
    params = [c.name for c in RC.parameter_cases()]
    left_out = [n for n in params if n not in names]
    assert sorted(left_out) == sorted(RC.NOT_IN_FIXTURE) and 10 * len(left_out) <= len(params)
    assert all(c.name in names for c in RC.chosen_boundary_cases()) and len(names) == len(set(names))
    for case in fx["cases"]:
        r = RS.Restated(case["cols"], case["rows"])
        for k, step in enumerate(case["steps"]):
            RC.apply_case_ops(r, step.get("ops", []))
            out = r.apply(RC.unpack_frame(step["input_parts"]), step["dt"])
            assert (len(out), hashlib.sha256(out).hexdigest()) == (step["out_len"], step["sha256"]), f"{case['name']} step {k}"
        assert hashlib.sha256(RC.canonical_grid_bytes(r.state())).hexdigest() == case["final_grid_sha256"], case["name"]
        r.close()


def test_kernel_matches_restatement_on_parameter_extremes():
    cs = RC.parameter_cases()
    assert len(cs) >= 28 + 2 + 3
    pairs = [_pair(c) for c in cs]
    _run_sequences(cs, pairs, tight=False)
    _close(pairs)
    for c in cs:  # and one frame per launch, with the table sized by that frame alone
        pairs = [_pair(c)]
        _run_sequences([c], pairs, tight=False)
        _close(pairs)


def test_kernel_matches_restatement_on_boundary_cases():
    n = len(cases())
    assert n > 3500 and len({c.name for c in cases()}) == n
    _parallel("plain")


def test_kernel_matches_restatement_on_boundary_cases_in_mixed_batches():
    """batches drawn across the whole list (every token kind, boundary and grid beside each other, so table sizes differ
    within a launch), tight slots, and in each batch one case on a grid beyond the LDS table"""
    _parallel("mixed")


def _job_slots(idx):
    for i in idx:
        c = cases()[i]
        f = c.frames[0]
        e, r = _pair(c)
        RC.check(RS.emu_batch([(e, f, c.dts[0])])[0], r.apply(f, c.dts[0]), e.grid(), r.state(), c.name + " step 0", e.cols)
        before = e.state[:e.cols * e.rows].copy()
        want = r.apply(f, 0.0)  # dt = 0: the refused calls advance the time by nothing
        L = len(want)
        src_stride = (len(f) + 15) // 16 * 16
        if 20 * len(f) + 1 > L - 1:  # (else no slot the kernel accepts is too small)
            for stride in (L - 1, L):  # L bytes hold the output but not its NUL
                if stride == 0:
                    continue
                got = RS.emu_batch([(e, f, 0.0)], dst_stride=stride, src_stride=src_stride)[0]  # (checks the guard bytes)
                assert got == RS.LEN_OVERFLOW, f"{c.name}: slot of {stride} for {L} bytes and the NUL"
                assert e.state[:e.cols * e.rows].tobytes() == before.tobytes(), f"{c.name}: state after the overflow"
        got = RS.emu_batch([(e, f, 0.0)], dst_stride=L + 1, src_stride=src_stride)[0]
        RC.check(got, want, e.grid(), r.state(), f"{c.name}: slot of exactly {L} + 1", e.cols)
        _close([(e, r)])


def test_slots_of_exactly_the_output_length_one_more_and_one_less():
    assert sum(len(j) for j in _jobs_slots()) > 600
    _parallel("slots")


def test_told_length_beyond_the_stride_is_clamped_and_error_codes_travel():
    grids = [(20, 6), (8, 3), (20, 6), (11, 7), (20, 6)]
    pairs = [(RS.Emulated(*g), RS.Restated(*g)) for g in grids]
    stride = 96
    body = (RC.LINE * 8)[:stride - 20] + RC.E + b"[38;2;9;8;7mxy"
    for step in range(2):
        frames = [RC.LINE * 3, body + b"#" * (stride - len(body)), RC.E + b"[48;2;1;2;3mq\nzz", b"abc", RC.LINE * 4 + b"\xe2\x96"]
        assert len(frames[1]) == stride  # no NUL inside the slot: what follows it is the next frame's bytes
        told = [len(f) for f in frames]
        told[1] = stride + 100
        told[3] = 0xFFFFFFF5
        before = pairs[3][0].state.copy()
        got = RS.emu_batch([(pairs[k][0], frames[k], 0.03) for k in range(5)], src_stride=stride, src_lens=told)
        assert got[3] == 0xFFFFFFF5 and pairs[3][0].state.tobytes() == before.tobytes()
        for k in (0, 1, 2, 4):
            e, r = pairs[k]
            RC.check(got[k], r.apply(frames[k], 0.03), e.grid(), r.state(), f"step {step} frame {k}", e.cols)
    _close(pairs)


def test_grid_written_smaller_than_allocated_and_back():
    """num_columns / num_rows below the allocation change the grid's pitch; the cells beyond the smaller grid keep what
    they held (the reference never touches them), also across a frame that overflows its slot while the grid is small"""
    e, r = RS.Emulated(12, 6), RS.Restated(12, 6)
    for k, (cols, rows, dt, overflow) in enumerate(RC.SHRUNK_STEPS):
        if cols:
            for o in (e.s, r.r):
                o.num_columns, o.num_rows = cols, rows
        if overflow:
            got = RS.emu_batch([(e, RC.SHRUNK_FRAME, dt)], dst_stride=256)[0]
            assert got == RS.LEN_OVERFLOW
            r.r.time = e.s.time  # the host side advanced; the grid did not move
        else:
            RC.check_output(RS.emu_batch([(e, RC.SHRUNK_FRAME, dt)])[0], r.apply(RC.SHRUNK_FRAME, dt), f"step {k}")
        RC.check_grid(e.grid(), r.state(), f"step {k}: the grid as allocated", None)
    _close([(e, r)])


def test_descriptor_that_leaves_the_backup_field_zero():
    """a descriptor whose last field is 0 (its meaning before the field had one) keeps its backup directly behind the grid
    as written: an overflowing frame restores the state bit for bit, and the steps round it are the restatement's"""
    e, r = RS.Emulated(12, 6), RS.Restated(12, 6)
    e.backup = 0
    for k, dt in enumerate((0.05, 0.07, 0.0, 0.11)):
        RC.check_output(RS.emu_batch([(e, RC.SHRUNK_FRAME, dt)])[0], r.apply(RC.SHRUNK_FRAME, dt), f"step {k}")
        RC.check_grid(e.grid(), r.state(), f"step {k}", None)
        before = e.state[:12 * 6].tobytes()
        assert RS.emu_batch([(e, RC.SHRUNK_FRAME, dt)], dst_stride=256)[0] == RS.LEN_OVERFLOW
        assert e.state[:12 * 6].tobytes() == before, f"step {k}: the grid behind an overflow"
        r.r.time = e.s.time
    _close([(e, r)])


JOBS = {"plain": (_job_plain, _jobs_plain), "mixed": (_job_mixed, _jobs_mixed), "slots": (_job_slots, _jobs_slots)}

if __name__ == "__main__":  # a worker of _parallel: kind, worker number, workers
    fn, jobs = JOBS[sys.argv[1]]
    mine = jobs()[int(sys.argv[2])::int(sys.argv[3])]
    for job in mine:
        try:
            fn(job)
        except AssertionError as e:
            sys.exit(f"{e}")
    print("jobs done:", len(mine))
