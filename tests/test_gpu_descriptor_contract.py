"""-m gpu: the frame descriptor's sampling rule (include/achip_types.h achip_frame_t) through pkg.Plan on the MI355X -- the
named cases of tests/descriptor_ref.py (hand-set ratios, padded source rows, flips, colour filters, degenerate shapes, pads)
in every geometry this build carries, an automatic plan per mode, render_crc, render_packets_packed and the length-first
path.  Sources sit inside guarded device buffers (sentinel-filled row padding and guard zones), slabs are filled with 0xEE
and checked behind each frame's NUL.

The flipped ratio-1.0 cases on sources smaller than the output (descriptor_ref.FLIP_UNCLAMPED) stay on the emulator
(tests/test_descriptor_contract.py): should the clamp of the lean loop ever regress, they address memory about 4 GB away
from the source, and such a read must not happen on a shared card."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import descriptor_ref as ref  # noqa: E402
import orc  # noqa: E402
from achip_ctypes import ALL_MODES, MODE_NAMES, MODE_TRUE_FG  # noqa: E402

PAL = orc.PALETTE_STANDARD
GEOMETRIES = (0, 1, 2, 4, 16, 17, 18, 19, 24, 25, 26, 27, 29)  # (31 / 32 share frames out: plans take them by themselves)
CASES = [c for c in ref.NAMED if c.name not in ref.FLIP_UNCLAMPED]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    assert torch.cuda.is_available(), "these tests need a GPU"
    assert pkg.lib().asciichat_hip_device_count() > 0, "libasciichat_hip.so sees no HIP device"
    torch.cuda.set_device(0)
    ref.use_host(pkg.lib(), pkg.Frame)  # descriptors built with the package's own host helpers
    return pkg, torch


def upload(gpu, cases, seed=1):
    """-> [(case, host Guarded, device buffer, package Frame)]: every guarded buffer copied whole to the device"""
    pkg, torch = gpu
    out = []
    for c, g, _ in ref.build(cases, seed):
        dev = torch.from_numpy(g.buf).cuda()
        out.append((c, g, dev, ref.make_frame(c, dev.data_ptr() + g.base)))
    return out


def expected(mode, built):
    return [ref.expected(mode, f, g.buf, PAL, base_offset=g.base) for (c, g, _, f) in built]


def render_slab(gpu, plan, n, what):
    """plan.render into a 0xEE slab: frames, NULs, nothing written behind a NUL"""
    pkg, torch = gpu
    out = torch.full((n * plan.stride,), 0xEE, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    plan.render(out.data_ptr(), plan.stride, ln.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host, lens = out.cpu().numpy(), ln.cpu().numpy().astype(np.uint32)
    res = []
    for k in range(n):
        assert lens[k] < 0xFFFFFFF0, (what, k, hex(int(lens[k])))
        s = k * plan.stride
        res.append(host[s:s + int(lens[k])].tobytes())
        assert host[s + int(lens[k])] == 0, (what, k, "NUL")
        assert (host[s + int(lens[k]) + 1:s + plan.stride] == 0xEE).all(), (what, k, "bytes behind the NUL")
    return res


@pytest.mark.parametrize("mode", ALL_MODES, ids=MODE_NAMES)
def test_every_geometry_follows_the_descriptor_rule(gpu, mode):
    pkg, torch = gpu
    built = upload(gpu, [c for c in CASES if c.sw * c.sh > 1])
    frames = [f for (_, _, _, f) in built]
    want = expected(mode, built)
    plan = pkg.Plan(mode, PAL, frames)  # the automatic choice
    assert render_slab(gpu, plan, len(frames), (MODE_NAMES[mode], "auto")) == want
    plan.close()
    # every geometry the host's policy lets a plan be forced to (set_variant must agree), rendered
    taken = ref.forced_geometries(pkg, mode, frames, GEOMETRIES)
    assert taken, MODE_NAMES[mode]
    for v in taken:
        plan = pkg.Plan(mode, PAL, frames)
        plan.set_variant(v)
        got = render_slab(gpu, plan, len(frames), (MODE_NAMES[mode], v))
        plan.close()
        for (c, _, _, _), e, r in zip(built, want, got):
            assert r == e, (MODE_NAMES[mode], v, c)
    # the 1x1 sources (the general sampler) in an automatic plan of their own
    one = upload(gpu, ref.ONE_BY_ONE)
    plan = pkg.Plan(mode, PAL, [f for (_, _, _, f) in one])
    assert render_slab(gpu, plan, len(one), (MODE_NAMES[mode], "1x1")) == expected(mode, one)
    plan.close()


@pytest.mark.parametrize("mode", ALL_MODES, ids=MODE_NAMES)
def test_render_crc_on_the_named_cases(gpu, mode):
    pkg, torch = gpu
    built = upload(gpu, [c for c in CASES if c.sw * c.sh > 1], seed=3)
    frames = [f for (_, _, _, f) in built]
    n = len(frames)
    want = expected(mode, built)
    plan = pkg.Plan(mode, PAL, frames)
    out = torch.full((n * plan.stride,), 0xEE, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    crc = torch.zeros(n, dtype=torch.int32, device="cuda")
    plan.render_crc(out.data_ptr(), plan.stride, ln.data_ptr(), crc.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host, lens, cc = out.cpu().numpy(), ln.cpu().numpy().astype(np.uint32), crc.cpu().numpy().astype(np.uint32)
    plan.close()
    for k, ((c, _, _, _), e) in enumerate(zip(built, want)):
        assert host[k * plan.stride:k * plan.stride + int(lens[k])].tobytes() == e, (MODE_NAMES[mode], c)
        assert int(cc[k]) == orc.crc32c(e), (MODE_NAMES[mode], c)


@pytest.mark.parametrize("form", ["pack", "length_first"])
def test_exact_length_forms_on_the_named_cases(gpu, form):
    """The two exact-length forms of a whole-frame truecolor plan (geometry 17), twice on the plan's cursor words: bytes at
    their offsets, frames tiling the destination.  pack: the named cases fit the one-launch PACK form's 48 KB
    (plan.exact_length), render_packets_packed takes it with the checksums.  length_first: one 200x60 frame beside them puts
    the plan's bound beyond that form, so set_exact_length(1) makes render_packed take the length-first form
    (plan.length_first) for every frame of the launch."""
    pkg, torch = gpu
    stream = torch.cuda.current_stream().cuda_stream
    cases = [c for c in CASES if c.sw * c.sh > 1]
    if form == "length_first":
        cases = cases + [ref.case("wide_lf", 300, 200, 200, 60, 0xC000 + 0x5555, 0x1_4000, stride=3 * 300 + 7, ops=ref.FLIP_Y, pl=3, pt=2)]
    built = upload(gpu, cases, seed=5)
    frames = [f for (_, _, _, f) in built]
    m = len(frames)
    want = expected(MODE_TRUE_FG, built)
    plan = pkg.Plan(MODE_TRUE_FG, PAL, frames)
    plan.set_variant(17)  # whole frames: the exact-length forms' precondition
    if form == "length_first":
        plan.set_exact_length(1)
        assert plan.stride > 48 * 1024 and not plan.exact_length and plan.length_first
    else:
        assert plan.exact_length and not plan.length_first
    dims = torch.tensor([[c.ow, c.oh] for (c, _, _, _) in built], dtype=torch.int32, device="cuda")
    slab = torch.full((m * plan.stride,), 0xEE, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(m, dtype=torch.int32, device="cuda")
    crc = torch.zeros(m, dtype=torch.int32, device="cuda")
    hdr = torch.zeros(m * 24, dtype=torch.uint8, device="cuda")
    pkt = torch.zeros(m, dtype=torch.int32, device="cuda")
    dst = torch.full((m * plan.stride,), 0xEE, dtype=torch.uint8, device="cuda")
    off = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    plen = torch.zeros(m, dtype=torch.int32, device="cuda")
    for launch in range(2):
        if form == "pack":
            plan.render_packets_packed(slab.data_ptr(), plan.stride, ln.data_ptr(), dims.data_ptr(), crc.data_ptr(), hdr.data_ptr(),
                                       pkt.data_ptr(), dst.data_ptr(), dst.numel(), off.data_ptr(), plen.data_ptr(), stream)
        else:
            plan.render_packed(slab.data_ptr(), plan.stride, ln.data_ptr(), dst.data_ptr(), dst.numel(), off.data_ptr(),
                               plen.data_ptr(), stream)
        torch.cuda.synchronize()
        assert (slab.cpu().numpy() == 0xEE).all(), (form, launch, "both forms are one launch: the slab is never written")
        o, l, d = off.cpu().numpy().astype(np.uint64), plen.cpu().numpy().astype(np.uint32), dst.cpu().numpy()
        spans = sorted((int(o[i]), int(o[i]) + (len(want[i]) + 15) // 16 * 16) for i in range(m))
        assert spans[0][0] == 0 and all(spans[i][1] == spans[i + 1][0] for i in range(m - 1)) and spans[-1][1] == int(o[m]), launch
        for i, (c, _, _, _) in enumerate(built):
            assert int(l[i]) == len(want[i]) and d[int(o[i]):int(o[i]) + int(l[i])].tobytes() == want[i], (form, launch, c)
        if form == "pack":
            cc = crc.cpu().numpy().astype(np.uint32)
            for i, (c, _, _, _) in enumerate(built):
                assert int(cc[i]) == orc.crc32c(want[i]), (launch, c)
    plan.close()
