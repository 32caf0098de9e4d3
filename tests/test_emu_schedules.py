"""The emulator's schedules (tests/hipemu/hip_emu.h) on probe kernels of their own (tests/hipemu/sched_probe_emu_driver.cpp): the
schedules bite -- a read with no barrier in front of it, which the ascending schedule can never see, fails under the others -- and
legal code is indifferent to them; the default is the loop the emulator always ran; a (policy, seed) replays; a real deadlock is
still a deadlock under every policy."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import emubuild
from emu_schedule import DEFAULT, Schedule, pick_log, scheduled

MAGIC = 0x600DF00D
SEEDS = range(8)
WAVES = 4


def _library():
    return emubuild.shared_library("libsched_probe_emu.so", "sched_probe_emu_driver.cpp", ())


@pytest.fixture(scope="module")
def probe():
    L = C.CDLL(_library())
    L.probe_word_for_all.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.probe_flag_handoff.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.probe_append_index.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.probe_only_steps.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    for f in (L.probe_word_for_all, L.probe_flag_handoff, L.probe_append_index, L.probe_only_steps):
        f.restype = None
    return L


def word_for_all(L, sched, barrier, blocks=2):
    out = np.zeros(blocks * 64 * WAVES, np.uint32)
    with scheduled(L, sched):
        L.probe_word_for_all(blocks, WAVES, int(barrier), out.ctypes.data)
    want = np.repeat(MAGIC + np.arange(blocks, dtype=np.uint32), 64 * WAVES)
    return out, want


LATES = [Schedule.late(w, k) for w in range(WAVES) for k in (1, 2, 50)]


def test_a_missing_barrier_is_invisible_in_ascending_order_and_seen_in_the_others(probe):
    out, want = word_for_all(probe, DEFAULT, barrier=False)
    assert (out == want).all(), "ascending waves: wave 0 always wrote before anybody read -- why the suite could not see such a bug"
    out, want = word_for_all(probe, Schedule.desc(), barrier=False)
    assert (out[:64] == want[:64]).all() and (out[64:64 * WAVES] == 0xCDCDCDCD).all(), "DESC: waves 3, 2, 1 read the LDS poison"
    incomplete = [s for s in SEEDS if (word_for_all(probe, Schedule.random(s), barrier=False)[0] != want).any()]
    assert incomplete, "not one of 8 RANDOM seeds ran another wave in front of wave 0"
    out, want = word_for_all(probe, Schedule.late(0, 1), barrier=False)
    assert (out[64:64 * WAVES] == 0xCDCDCDCD).all(), "LATE(0, 1): the writer's wave came last"


@pytest.mark.parametrize("sched", [DEFAULT, Schedule.desc()] + LATES + [Schedule.random(s) for s in SEEDS], ids=str)
def test_with_its_barrier_the_same_kernel_is_indifferent_to_the_schedule(probe, sched):
    out, want = word_for_all(probe, sched, barrier=True)
    assert (out == want).all(), str(sched)


def flag_handoff(L, sched, work=3):
    out = np.zeros(130, np.uint32)
    with scheduled(L, sched) as run:
        L.probe_flag_handoff(WAVES, 2, work, out.ctypes.data)
    # the producers are waves 1 and 3: 1000 * (wave + 1) + the 32 odd lanes of each of their `work` ballots
    assert (out[0:128:2] == 2000 + 32 * work).all() and (out[1:128:2] == 4000 + 32 * work).all(), (str(sched), out[:4])
    return run.naps


@pytest.mark.parametrize("sched", [DEFAULT, Schedule.desc()] + LATES + [Schedule.random(s) for s in SEEDS], ids=str)
def test_a_flag_hand_off_through_a_polling_loop_completes_under_every_schedule(probe, sched):
    flag_handoff(probe, sched)


def test_the_nap_counter_rises_with_the_lateness_of_the_awaited_wave(probe):
    """a poll = two sweeps (the two halves of its ballot), so a producer held for k sweeps costs the 64 waiting lanes about k / 2
    naps each; in ascending order the waiter loses a few polls to the producers' own work, no more"""
    base = flag_handoff(probe, DEFAULT)
    assert base <= 64 * 4, base
    for producer in (1, 3):  # the wave below the waiter, the wave above it
        n = [flag_handoff(probe, Schedule.late(producer, k)) for k in (100, 400)]
        assert n[0] >= base + 64 * 40 and n[1] >= n[0] + 64 * 140, (producer, base, n)
    assert flag_handoff(probe, Schedule.late(0, 400)) <= 64 * 4, "a wave nobody waits for costs nothing"


def append_index(L, sched, grid=(5, 2, 1)):
    n = grid[0] * grid[1] * grid[2]
    lst = np.zeros(1 + n, np.uint32)
    with scheduled(L, sched):
        L.probe_append_index(*grid, lst.ctypes.data)
    assert lst[0] == n
    return [int(v) for v in lst[1:]]


def test_workgroup_orders(probe):
    assert append_index(probe, DEFAULT) == list(range(10))
    assert append_index(probe, Schedule().workgroups("desc")) == list(range(9, -1, -1))
    perms = [append_index(probe, Schedule().workgroups("shuffle", s)) for s in range(4)]
    for p in perms:
        assert sorted(p) == list(range(10)) and p != list(range(10))
    assert len({tuple(p) for p in perms}) > 1, "the seed decides the permutation"
    assert append_index(probe, Schedule().workgroups("shuffle", 2)) == perms[2], "and the same seed gives it again"
    assert append_index(probe, Schedule.desc()) == list(range(10)), "a wave policy leaves the workgroups' order alone"


def only_steps(L, sched, steps=5, blocks=2):
    out = np.zeros(64 * WAVES, np.uint32)
    with scheduled(L, sched) as run:
        L.probe_only_steps(blocks, WAVES, steps, out.ctypes.data)
    assert (out == 32 * steps).all()
    assert run.picks == len(run.log)
    return run.log


def test_the_default_schedule_is_the_loop_the_emulator_always_ran(probe):
    """every wave, 0 .. W-1, in every sweep: a ballot is two yields, so `steps` ballots and the exit are 2 * steps + 1 sweeps"""
    assert only_steps(probe, DEFAULT) == (list(range(WAVES)) * 11) * 2
    assert only_steps(probe, Schedule.desc()) == (list(range(WAVES - 1, -1, -1)) * 11) * 2
    late = only_steps(probe, Schedule.late(2, 7), blocks=1)
    assert late[:7 * 3] == [0, 1, 3] * 7 and late[7 * 3:7 * 3 + 4] == [0, 1, 2, 3] and late.count(2) == 11


def test_a_policy_and_a_seed_replay(probe):
    logs = [only_steps(probe, Schedule.random(s)) for s in (1, 2)]
    assert logs[0] != logs[1], "two seeds, one log"
    assert only_steps(probe, Schedule.random(1)) == logs[0] and only_steps(probe, Schedule.random(2)) == logs[1]
    for log in logs:  # every wave took its 11 steps per workgroup, in no regular order
        assert [log.count(w) for w in range(WAVES)] == [22] * WAVES and log != sorted(log)
    assert Schedule.parse(str(Schedule.random(7).workgroups("shuffle", 3))) == Schedule.random(7).workgroups("shuffle", 3)
    assert Schedule.parse(str(Schedule.late(3, 40))) == Schedule.late(3, 40) and Schedule.parse(str(DEFAULT)) == DEFAULT


def test_the_default_is_back_when_the_body_raises(probe):
    with pytest.raises(ZeroDivisionError):
        with scheduled(probe, Schedule.desc()):
            1 / 0
    pick_log(probe, reset=True)
    out = np.zeros(64 * WAVES, np.uint32)
    probe.probe_only_steps(1, WAVES, 1, out.ctypes.data)
    assert pick_log(probe, reset=True)[0] == list(range(WAVES)) * 3


@pytest.mark.parametrize("sched", [DEFAULT, Schedule.desc(), Schedule.random(5), Schedule.late(0, 30), Schedule.late(1, 30)], ids=str)
@pytest.mark.parametrize("entry,message", [("probe_divergent_barrier", "hipemu: deadlock (divergent barrier?) block 0"),
                                           ("probe_ballot_after_exit", "hipemu: wave op with exited lanes (wave")])
def test_a_real_deadlock_still_aborts_with_its_message(sched, entry, message):
    """(in a process of its own, started fresh: the detection is an abort)"""
    code = (f"import ctypes, emu_schedule as S; L = ctypes.CDLL({_library()!r}); S.set_schedule(L, S.Schedule.parse({str(sched)!r})); "
            f"L.{entry}(2); print('not detected')")
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == -6 and message in r.stderr and "not detected" not in r.stdout, (str(sched), r.returncode, r.stderr[-300:])
