"""The emulator's twin of gfx950_ops.hpp (tests/hipemu/gfx950_ops.hpp), op by op: the probe kernels of tests/opsprobe/ under the
fiber emulator on the shared cases of ops_cases.py against the restatements of ops_ref.py -- the same kernels, cases and reference
test_gpu_ops.py holds the product header to on the device, so the twin is a checked model of the machine on everything the table
holds.  Plus the refusals of arguments outside an operation's domain, and the guard that keeps the probe complete: an operation
added to either header without its twin and a probe fails here."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emubuild  # noqa: E402
import ops_cases as OC  # noqa: E402

PRODUCT = os.path.join(emubuild.CSRC, "gfx950_ops.hpp")
TWIN = os.path.join(emubuild.EMU_DIR, "gfx950_ops.hpp")
PROBE = os.path.join(emubuild.ROOT, "tests", "opsprobe", "ops_probe_kernels.hpp")
# no value to compare: nothing is emitted, or a clock, or a wait
EXEMPT = {"keep_alive", "spin_nap", "wait_vmem_all", "wave_lockstep", "cycle_now", "wall_now"}
# the product's building blocks of its two scans: not part of the interface, no kernel calls them
HELPERS = {"dpp_add", "dpp_xor"}


def _library():
    return emubuild.shared_library("libops_probe_emu.so", "ops_probe_emu_driver.cpp", ("../opsprobe/ops_probe_kernels.hpp",))


@pytest.fixture(scope="module")
def emu():
    return OC.declare(C.CDLL(_library()))


@pytest.mark.parametrize("family", list(OC.FAMILIES))
def test_family_under_the_emulator(emu, family):
    OC.FAMILIES[family](emu, OC.HostBackend())


def test_a_grid_beyond_64_workgroups_is_refused(emu):
    assert emu.opsprobe_wave(OC.MAX_GRID + 1, *[None] * 10) == -1


@pytest.mark.parametrize("which,message", [(0, "wave_read_lane: lane outside its domain (64"),
                                           (1, "wave_read_lane: a lane select that differs from lane 0's outside its domain"),
                                           (2, "wave_shfl_up: distance outside its domain (64"),
                                           (3, "wave_shfl_up: distance outside its domain (-1")])
def test_the_twin_refuses_arguments_outside_the_domain(which, message):
    """(in a process of its own: the refusal is an abort)"""
    code = f"import ctypes; ctypes.CDLL({_library()!r}).opsprobe_emu_out_of_domain({which}); print('not refused')"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == -6 and "not refused" not in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert "hipemu: " + message in r.stderr, r.stderr


# ---- the guard ------------------------------------------------------------------------------------------------------------------
_DECL = re.compile(r"^(?:template <[^>]*> )?(?:__device__ )?inline [\w :*&]*?(\w+)\(", re.M)


def _strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared(path):
    """the names of the functions a header declares in namespace achip"""
    text = _strip_comments(open(path).read())
    body = text[text.index("namespace achip {"):text.index("} // namespace achip")]
    return set(_DECL.findall(body))


def exercised(names, probe_text):
    text = _strip_comments(probe_text)
    return {n for n in names if re.search(r"\b%s\s*[<(]" % re.escape(n), text)}


def check_guard(product_names, twin_names, probe_text):
    product_names = set(product_names) - HELPERS
    assert product_names == set(twin_names), (f"only in the product header: {sorted(product_names - set(twin_names))}; only in the twin: "
                                               f"{sorted(set(twin_names) - product_names)}")
    assert EXEMPT <= product_names, f"exempt names that no header declares: {sorted(EXEMPT - product_names)}"
    missing = product_names - EXEMPT - exercised(product_names, probe_text)
    assert not missing, f"operations of gfx950_ops.hpp that tests/opsprobe/ops_probe_kernels.hpp does not exercise: {sorted(missing)}"


def test_both_headers_declare_the_same_operations_and_the_probe_exercises_them():
    product, twin = declared(PRODUCT), declared(TWIN)
    assert len(product) > 40 and {"wave_inclusive_scan", "ds_store_byte", "store_u4_nt", "lds_store_fence", "agent_arrive_u32"} <= product
    assert HELPERS <= product
    for name in sorted(os.listdir(emubuild.CSRC)):  # the helpers stay inside the header
        if name != "gfx950_ops.hpp" and name.endswith((".hpp", ".h", ".hip")):
            text = open(os.path.join(emubuild.CSRC, name)).read()
            assert not any(h in text for h in HELPERS), name
    check_guard(product, twin, open(PROBE).read())


def test_the_guard_notices_an_operation_without_twin_or_probe():
    product, twin, probe = declared(PRODUCT), declared(TWIN), open(PROBE).read()
    with pytest.raises(AssertionError, match="only in the product header: \\['wave_rotate'\\]"):
        check_guard(product | {"wave_rotate"}, twin, probe)
    with pytest.raises(AssertionError, match="only in the twin: \\['wave_rotate'\\]"):
        check_guard(product, twin | {"wave_rotate"}, probe)
    with pytest.raises(AssertionError, match="does not exercise: \\['wave_rotate'\\]"):
        check_guard(product | {"wave_rotate"}, twin | {"wave_rotate"}, probe)
    with pytest.raises(AssertionError, match="does not exercise: \\['lds_store_fence'\\]"):
        check_guard(product, twin, probe.replace("lds_store_fence", "fence"))


def test_the_probe_includes_nothing_but_the_ops_header():
    text = open(PROBE).read()
    assert set(re.findall(r"#\s*include\s*[<\"]([^>\"]+)[>\"]", text)) == {"gfx950_ops.hpp", "stdint.h"}
    assert not re.search(r"#\s*(if|ifdef|ifndef|elif|else)\b", text), "no conditional compilation in the probe kernels"
