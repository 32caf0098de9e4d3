"""The schedules of the CPU fiber emulator (tests/hipemu/hip_emu.h), set on a loaded emulator library for the length of a `with`
block.  TESTS ONLY.

    with emu_schedule.scheduled(emu.lib(), Schedule.late(1, 300)) as run:
        got = emu.render_frames(...)
    assert run.naps > 0

Every driver library of tests/hipemu exports the same three functions from hip_emu.h; the default schedule (every runnable wave
in ascending order, workgroups in ascending order) is what the emulator always ran, and is put back when the block is left, also
by an exception: a failing test cannot leak its schedule into the next one.

To replay a failure, take the four things its message names -- policy, seed, workgroup order, case -- and run that case inside
`scheduled(library, Schedule.parse("<the text in the message>"))`: str(Schedule) and Schedule.parse are inverses, and the
emulator's generator is seeded from the seed and the workgroup's index alone."""
import contextlib
import ctypes as C
import re
from collections import namedtuple

WAVES = {"asc": 0, "desc": 1, "random": 2, "late": 3}
WORKGROUPS = {"asc": 0, "desc": 1, "shuffle": 2}
PICK_LOG_CAP = 1 << 16


class Schedule(namedtuple("Schedule", "waves seed late_wave late_sweeps late_after wg wg_seed")):
    """waves: asc | desc | random(seed) | late(late_wave, late_sweeps[, late_after]); wg: asc | desc | shuffle(wg_seed).
    late_after = B: the held wave's sweeps count from the release of the workgroup's B-th block barrier, not from its start"""
    __slots__ = ()

    def __new__(cls, waves="asc", seed=0, late_wave=0, late_sweeps=0, late_after=0, wg="asc", wg_seed=0):
        assert waves in WAVES and wg in WORKGROUPS, (waves, wg)
        return super().__new__(cls, waves, int(seed), int(late_wave), int(late_sweeps), int(late_after), wg, int(wg_seed))

    @classmethod
    def desc(cls, **kw):
        return cls("desc", **kw)

    @classmethod
    def random(cls, seed, **kw):
        return cls("random", seed=seed, **kw)

    @classmethod
    def late(cls, wave, sweeps, after=0, **kw):
        return cls("late", late_wave=wave, late_sweeps=sweeps, late_after=after, **kw)

    def workgroups(self, wg, wg_seed=0):
        return self._replace(wg=wg, wg_seed=int(wg_seed))

    def __str__(self):
        w = {"random": "RANDOM(seed=%d)" % self.seed, "late": "LATE(wave=%d, sweeps=%d, after=%d)" % (self.late_wave, self.late_sweeps, self.late_after)}
        g = "SHUFFLE(seed=%d)" % self.wg_seed if self.wg == "shuffle" else self.wg.upper()
        return "waves %s, workgroups %s" % (w.get(self.waves, self.waves.upper()), g)

    @classmethod
    def parse(cls, text):
        m = re.fullmatch(r"waves (\w+)(?:\((?:seed=(\d+)|wave=(\d+), sweeps=(\d+), after=(\d+))\))?, workgroups (\w+)(?:\(seed=(\d+)\))?", text)
        assert m, text
        return cls(m.group(1).lower(), m.group(2) or 0, m.group(3) or 0, m.group(4) or 0, m.group(5) or 0, m.group(6).lower(), m.group(7) or 0)


DEFAULT = Schedule()


def declare(lib):
    if not getattr(lib, "_hipemu_schedule_declared", False):
        lib.hipemu_set_schedule.restype = None
        lib.hipemu_set_schedule.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_uint64]
        lib.hipemu_naps.restype = C.c_uint64
        lib.hipemu_naps.argtypes = [C.c_int]
        lib.hipemu_pick_log.restype = C.c_uint64
        lib.hipemu_pick_log.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
        lib._hipemu_schedule_declared = True
    return lib


def set_schedule(lib, s):
    """(also clears the library's nap counter and pick log)"""
    declare(lib).hipemu_set_schedule(WAVES[s.waves], s.seed, s.late_wave, s.late_sweeps, s.late_after, WORKGROUPS[s.wg], s.wg_seed)


def naps(lib, reset=False):
    """calls of the twin's spin_nap since the last reset: how often a lane polled, found nothing and waited"""
    return int(declare(lib).hipemu_naps(1 if reset else 0))


def pick_log(lib, reset=False):
    """(the waves visited since the last reset, in order -- the first PICK_LOG_CAP of them, how many there were)"""
    buf = (C.c_uint8 * PICK_LOG_CAP)()
    n = int(declare(lib).hipemu_pick_log(buf, PICK_LOG_CAP, 1 if reset else 0))
    return list(buf[:min(n, PICK_LOG_CAP)]), n


class Run:
    """what a `scheduled` block saw: filled in when the block is left (and readable inside it through the library)"""

    def __init__(self, lib, schedule):
        self.lib, self.schedule, self.naps, self.picks, self.log = lib, schedule, None, None, None

    def naps_so_far(self):
        return naps(self.lib)


@contextlib.contextmanager
def scheduled(lib, schedule):
    """run the block's launches of `lib` under `schedule`; the default is back afterwards, whatever happened"""
    set_schedule(lib, schedule)
    run = Run(lib, schedule)
    try:
        yield run
    finally:
        run.naps = naps(lib)
        run.log, run.picks = pick_log(lib)
        set_schedule(lib, DEFAULT)
