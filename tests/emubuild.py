"""The one recipe by which the tests build a kernel driver of tests/hipemu into a shared library of the CPU emulator: rebuilt
when a source is newer, compiled into a private file and moved into place.  TESTS ONLY."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ascii-chat_amd", "csrc")
INC = os.path.join(ROOT, "include")
EMU_DIR = os.path.join(ROOT, "tests", "hipemu")
OUT_DIR = os.path.join(EMU_DIR, "_build")
INCLUDE = (EMU_DIR, CSRC, INC)  # EMU_DIR first: <gfx950_ops.hpp> is the emulator's twin of the product's header


def _header(name):
    """where the compiler finds `name`"""
    return next(p for p in (os.path.join(d, name) for d in INCLUDE) if os.path.exists(p))


def shared_library(so_name, driver, deps, defines=()):
    """tests/hipemu/<driver> -> the path of tests/hipemu/_build/<so_name>.  deps: the headers the driver includes beside the
    emulator's own, by name; defines: NAME=value macros, which belong into so_name too."""
    drv = os.path.join(EMU_DIR, driver)
    srcs = [drv] + [_header(h) for h in ("hip_emu.h", "gfx950_ops.hpp", *deps)]
    so = os.path.join(OUT_DIR, so_name)
    if not (os.path.exists(so) and all(os.path.getmtime(s) <= os.path.getmtime(so) for s in srcs)):
        os.makedirs(OUT_DIR, exist_ok=True)
        tmp = so + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", *["-I" + d for d in INCLUDE], *["-D" + d for d in defines],
                               drv, "-o", tmp])
        os.replace(tmp, so)  # atomic: a concurrent test process never loads a half-written library
    return so
