"""Pins the launch-geometry policy (achip_choose_geometry): tests/cabi/geometry_policy.c enumerates a grid of launches that
straddles every boundary the policy tests and prints one digest of (rc, variant, parts, rows_per_part) per group -- mode,
all-ASCII palette, forced geometry, caps set --, compared here with tests/golden/geometry_policy.json.  A change that is
meant to move choices regenerates the fixture (python tests/test_geometry_policy.py) and names the groups it moved."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "geometry_policy.json")
# the diagnostics switches the policy reads once per process: the small grid runs once per setting, each in its own process
ENV_RUNS = [("ASCIICHAT_HIP_STREAM_PARTS", "1"), ("ASCIICHAT_HIP_STREAM_PARTS", "3"),
            ("ASCIICHAT_HIP_ROWS_PARTS", "1"), ("ASCIICHAT_HIP_ROWS_PARTS", "5"),
            ("ASCIICHAT_HIP_ROWS_PARTS_WIDE", "0"), ("ASCIICHAT_HIP_ROWS_PARTS_WIDE", "2")]


def build(out_dir):
    exe = os.path.join(out_dir, "geometry_policy")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cabi", "geometry_policy.c"),
                           os.path.join(ROOT, "ascii-chat_amd", "csrc", "achip_host.c"), "-o", exe, "-lm"])
    return exe


def run(exe, grid, setting=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("ASCIICHAT_HIP_")}
    if setting:
        env[setting[0]] = setting[1]
    out = subprocess.run([exe, grid], env=env, capture_output=True, text=True, check=True).stdout
    groups = {}
    for line in out.splitlines():
        mode, ascii_only, forced, caps, count, digest = line.split()
        groups["mode=%s ascii=%s forced=%s caps=%s" % (mode, ascii_only, forced, caps)] = "%s %s" % (count, digest)
    return groups


def measure(exe):
    return {"full": run(exe, "full"),
            "small": {"%s=%s" % s: run(exe, "small", s) for s in ENV_RUNS}}


def differing(want, got):
    return sorted(k for k in set(want) | set(got) if want.get(k) != got.get(k))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("geometry_policy")))


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE, encoding="utf-8") as f:
        return json.load(f)


def test_full_grid_matches_fixture(harness, golden):
    got = run(harness, "full")
    assert len(got) == len(golden["full"]) >= 1000
    bad = differing(golden["full"], got)
    assert not bad, "geometry choices moved in %d groups: %s" % (len(bad), bad[:20])


@pytest.mark.parametrize("setting", ENV_RUNS, ids=["%s=%s" % s for s in ENV_RUNS])
def test_small_grid_under_switch_matches_fixture(harness, golden, setting):
    want = golden["small"]["%s=%s" % setting]
    got = run(harness, "small", setting)
    assert len(got) == len(want) >= 40
    bad = differing(want, got)
    assert not bad, "geometry choices moved under %s=%s in %d groups: %s" % (setting[0], setting[1], len(bad), bad[:20])


def test_forced_ids_that_are_no_geometry_are_refused(harness):
    out = subprocess.run([harness, "refuse"], capture_output=True, text=True, check=True).stdout
    rows = [tuple(int(x) for x in line.split()) for line in out.splitlines()]
    assert [r[0] for r in rows] == list(range(5, 16))
    for forced, tried, accepted in rows:
        assert tried >= 100 and accepted == 0, "forced id %d accepted for %d of %d launches" % (forced, accepted, tried)


if __name__ == "__main__":  # regenerate the fixture (a deliberate policy change)
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        data = measure(build(d))
    with open(FIXTURE, "w", encoding="utf-8") as f:
        json.dump(data, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE, file=sys.stderr)
