"""The fused composite sampler on the GPU through the C ABI, on the boundary families of tests/composite_cases.py
(tests/test_composite_boundaries.py: the same cases under the CPU emulator): the materialised canvas, the fused render in mixed
batches and by-value batches through the plan's own geometry and every product geometry that carries the sampler, lone frames
shared out over workgroups, 300 frames, the geometries without the sampler, the wire entry points, plan_update between plain
and composite frames, a host descriptor with a dirty padding word and one without cells over filled tile records.  Expectations are the oracle's alone."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composite_cases as CC  # noqa: E402
import orc  # noqa: E402
from achip_ctypes import ALL_MODES, MODE_CAPS, MODE_HB_TRUE, MODE_MONO, MODE_NAMES, MODE_TRUE_FG  # noqa: E402

CASES = CC.cases()
BY_NAME = {k.name: k for k in CASES}
PAL = orc.PALETTE_STANDARD
GUARD = 0xEE

# render_variants.h: the product's geometries that carry the composite sampler (ACHIP_VARIANTS, ACHIP_STREAM_TABLE without 18's
# whole-frame form, which no plan takes, ACHIP_ROWS_VARIANT_COMP), the ones built only with ACHIP_ALL_GEOMETRIES, and the modes
# each kernel is built for (ACHIP_FRAME_VARIANT_HALFBLOCK: none of the half-block modes in geometries 1 and 2)
PRODUCT = (0, 1, 4, 16, 17, 24, 25)
ALL_GEOMETRIES_ONLY = (2, 19)
CELL_MODES, RUN_MODES, HALFBLOCK = (1, 2, 3, 4), (0, 5, 6, 7, 8), (5, 6, 7, 8)
RENDERED = {}  # kernel -> {(geometry, mode name)} that rendered composites
REFUSED = set()  # (geometry, mode name) set_variant refused
CHOSEN = {}  # what the plans took by themselves: (what, mode name) -> (geometry, parts)


def kernel_of(v):
    return "rows" if v >= 24 else "stream" if v >= 16 else "phase"


def applies(v, mode):
    if v >= 24:
        return mode in RUN_MODES
    if v >= 16:
        return mode in CELL_MODES
    return not (v in (1, 2) and mode in HALFBLOCK)


@pytest.fixture(scope="module")
def pkg():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from __graft_entry__ import load_package

    p = load_package()
    assert torch.cuda.is_available() and p.lib().asciichat_hip_device_count() > 0
    return p


class _World:
    """every case's sources uploaded once, its descriptor (premise asserted) uploaded once and shared by all its frames"""

    def __init__(self, pkg):
        import torch
        self.pkg, self.keep, self.host, self.dev = pkg, {}, {}, {}
        for k in CASES:
            t = [None if i is None else torch.from_numpy(i).cuda() for i in k.imgs]
            self.keep[k.name] = t
            self.host[k.name] = k.descriptor(pkg.lib(), [None if x is None else x.data_ptr() for x in t], pkg.Composite)
            self.dev[k.name] = self.upload(self.host[k.name])
        torch.cuda.synchronize()

    def upload(self, comp):
        d = C.c_void_p()
        assert self.pkg.lib().asciichat_hip_composite_upload(C.byref(comp), C.byref(d)) == 0 and d.value
        return d

    def frame(self, case, mode, ops=None, comp_dev=None):
        tw, th = case.term
        f = self.pkg.frame_setup(None, tw, 2 * th, tw, case.frame_height(mode), MODE_CAPS.get(mode, (3, 0))[1], True, True, False)
        assert f is not None
        f.comp = (comp_dev or self.dev[case.name]).value
        if ops:
            assert self.pkg.lib().achip_frame_set_display_ops(C.byref(f), *ops) == 0 and f.ops
        return f

    def close(self):
        for d in self.dev.values():
            self.pkg.lib().asciichat_hip_free(d)


@pytest.fixture(scope="module")
def world(pkg):
    w = _World(pkg)
    yield w
    w.close()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def render(plan, n):
    """-> [bytes | error code] of the plan's frames; the NUL behind every frame and nothing behind that"""
    import torch
    out = torch.full((n * plan.stride + 64,), GUARD, dtype=torch.uint8, device="cuda")
    ln = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    plan.render(out.data_ptr(), plan.stride, ln.data_ptr(), _stream())
    torch.cuda.synchronize()
    host, lens = out.cpu().numpy(), ln.cpu().numpy().view(np.uint32)
    res = []
    for k in range(n):
        if lens[k] >= 0xFFFFFFF0:
            res.append(int(lens[k]))
            continue
        o = k * plan.stride
        res.append(host[o:o + int(lens[k])].tobytes())
        assert host[o + int(lens[k])] == 0, "the NUL behind the frame"
    assert (host[n * plan.stride:] == GUARD).all(), "bytes behind the slab were written"
    return res


def note(plan, mode, what=None):
    RENDERED.setdefault(kernel_of(plan.variant), set()).add((plan.variant, MODE_NAMES[mode]))
    if what:
        CHOSEN[what, MODE_NAMES[mode]] = (plan.variant, plan.parts)


def check(plan, mode, cases, what):
    got = render(plan, len(cases))
    for g, k in zip(got, cases):
        assert g == k.expected(mode), (what, k.name, MODE_NAMES[mode], plan.variant, plan.parts, g if isinstance(g, int) else len(g))
    note(plan, mode)


def test_materialised_canvas(pkg, world):
    """asciichat_hip_composite (composite_kernel: the global sampler at every pixel) into a guard-filled buffer"""
    import torch
    for k in CASES:
        W, H = k.canvas_dims
        dst = torch.full((3 * W * H + 256,), GUARD, dtype=torch.uint8, device="cuda")
        assert pkg.lib().asciichat_hip_composite(C.byref(world.host[k.name]), dst.data_ptr(), None) == 0, k.name
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert np.array_equal(got[:3 * W * H].reshape(H, W, 3), k.canvas()), k.name
        assert (got[3 * W * H:] == GUARD).all(), (k.name, "bytes behind the canvas were written")


def mixed(pkg, world, mode):
    """one plan with every case's frame (the descriptor array), first as the plan chooses, then every geometry forced in turn"""
    frames = [world.frame(k, mode, (True, True, 3) if i % 2 else None) for i, k in enumerate(CASES)]
    plan = pkg.Plan(mode, PAL, frames)
    try:
        assert not plan.uniform
        note(plan, mode, "every case in one plan")
        if mode in CELL_MODES:  # 34 small frames on 256 CUs: the stream kernel's four-wave geometry, a frame's blocks shared out
            assert plan.variant == 18 and plan.parts > 1, (MODE_NAMES[mode], plan.variant, plan.parts)
        check(plan, mode, CASES, "mixed, the plan's choice")
        for v in PRODUCT + ALL_GEOMETRIES_ONLY:
            try:
                plan.set_variant(v)
            except RuntimeError:
                REFUSED.add((v, MODE_NAMES[mode]))
                assert v in ALL_GEOMETRIES_ONLY or not applies(v, mode), (v, MODE_NAMES[mode], pkg.last_error())
                check(plan, mode, CASES, f"mixed, after geometry {v} was refused")  # renders as before
                continue
            assert applies(v, mode) and plan.variant == v, (v, MODE_NAMES[mode])
            check(plan, mode, CASES, f"mixed, geometry {v}")
    finally:
        plan.close()


@pytest.mark.parametrize("mode", ALL_MODES, ids=MODE_NAMES)
def test_fused_render_mixed_and_by_value(pkg, world, mode):
    mixed(pkg, world, mode)
    for k in CASES:  # three copies of one frame: the by-value form
        plan = pkg.Plan(mode, PAL, [world.frame(k, mode)] * 3)
        try:
            assert plan.uniform, k.name
            note(plan, mode)
            got = render(plan, 3)
            assert got == [k.expected(mode)] * 3, (k.name, MODE_NAMES[mode], plan.variant, plan.parts)
        finally:
            plan.close()


@pytest.mark.parametrize("mode", ALL_MODES, ids=MODE_NAMES)
def test_lone_frames(pkg, world, mode):
    """one frame per plan: shared out over row bands (the global sampler's carry pixel) or over workgroups of the stream kernel"""
    parts = {}
    for k in CASES:
        plan = pkg.Plan(mode, PAL, [world.frame(k, mode)])
        try:
            parts[k.name] = plan.parts
            note(plan, mode, "lone " + k.name if k.name in (CC.ZERO_CELL, CC.ALL_NONE, CC.ONE_PIXEL_CELL_H) else None)
            check(plan, mode, [k], "lone frame")
        finally:
            plan.close()
    if mode != 9:  # (the serial dither is never shared out)
        assert any(p > 1 for p in parts.values()), parts
    if mode == MODE_HB_TRUE:  # a few long tokens: the phase kernel's row bands, whose carry pixel the global sampler reads
        for name in (CC.ZERO_CELL, CC.ALL_NONE, CC.ONE_PIXEL_CELL_H, CC.ONE_PIXEL_CELLS):
            assert parts[name] > 1, (name, parts[name])


@pytest.mark.parametrize("mode", [MODE_TRUE_FG, MODE_HB_TRUE, MODE_MONO], ids=["true_fg", "hb_true", "mono"])
def test_300_frames(pkg, world, mode):
    """more frames than the card has CUs"""
    k = BY_NAME[CC.ONE_PIXEL_CELL_H]
    plan = pkg.Plan(mode, PAL, [world.frame(k, mode)] * 300)
    try:
        got = render(plan, 300)
        assert got == [k.expected(mode)] * 300, (MODE_NAMES[mode], plan.variant)
        note(plan, mode, "300 frames")
    finally:
        plan.close()


@pytest.mark.parametrize("mode,variant", [(MODE_HB_TRUE, 26), (MODE_HB_TRUE, 27), (MODE_HB_TRUE, 29), (MODE_HB_TRUE, 31), (MODE_MONO, 26),
                                          (MODE_MONO, 31), (MODE_TRUE_FG, 18), (2, 18)])
def test_geometries_without_the_composite_sampler(pkg, world, mode, variant):
    """the contract of plan_set_variant on a plan with composite frames: it refuses and the plan renders as before, or the plan
    renders the right bytes; never a geometry accepted and then an error code or other bytes"""
    cases = [BY_NAME["5 equal sources at 60x30"], BY_NAME["a 1x1 source"], BY_NAME[CC.ZERO_CELL]]
    for picked in (cases, cases[:1]):
        plan = pkg.Plan(mode, PAL, [world.frame(k, mode) for k in picked])
        try:
            before = (plan.variant, plan.parts)
            try:
                plan.set_variant(variant)
            except RuntimeError:
                REFUSED.add((variant, MODE_NAMES[mode]))
                assert (plan.variant, plan.parts) == before
            check(plan, mode, picked, f"geometry {variant} asked for")
        finally:
            plan.close()


@pytest.mark.parametrize("mode", [MODE_TRUE_FG, 2, MODE_HB_TRUE, MODE_MONO], ids=["true_fg", "256_fg", "hb_true", "mono"])
def test_wire_entry_points(pkg, world, mode):
    """plan_render_crc, plan_render_packets and plan_render_packets_packed on a composite plan: the plain render's bytes, the
    oracle's checksums, headers and packet checksums; the packed call falls back to the slab form (the exact-length and
    length-first forms exclude composites), so frame i lies behind the rounded lengths of the frames in front of it"""
    import torch
    names = ["9 equal sources at 60x30", "sources of different sizes", "a 1x1 source", "10 sources at 80x30", CC.ONE_PIXEL_CELL_H,
             CC.ONE_PIXEL_CELLS, CC.ZERO_CELL, CC.ALL_NONE]
    picked = [BY_NAME[x] for x in names]
    n = len(picked)
    plan = pkg.Plan(mode, PAL, [world.frame(k, mode) for k in picked])
    try:
        assert not plan.exact_length and not plan.length_first
        plain = render(plan, n)
        exp = [k.expected(mode) for k in picked]
        assert plain == exp
        wire = [CC.wire_expect(e, *k.term) for e, k in zip(exp, picked)]
        dims = torch.from_numpy(np.array([k.term for k in picked], dtype=np.uint32).view(np.int32)).cuda()
        for entry in ("crc", "packets", "packed"):
            out = torch.full((n * plan.stride + 64,), GUARD, dtype=torch.uint8, device="cuda")
            ln = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            crc = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            pkt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            hdr = torch.full((24 * n,), GUARD, dtype=torch.uint8, device="cuda")
            cap = n * plan.stride
            dst = torch.full((cap + 64,), GUARD, dtype=torch.uint8, device="cuda")
            off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
            lo = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            if entry == "crc":
                plan.render_crc(out.data_ptr(), plan.stride, ln.data_ptr(), crc.data_ptr(), _stream())
            elif entry == "packets":
                plan.render_packets(out.data_ptr(), plan.stride, ln.data_ptr(), dims.data_ptr(), crc.data_ptr(), hdr.data_ptr(), pkt.data_ptr(), _stream())
            else:
                plan.render_packets_packed(out.data_ptr(), plan.stride, ln.data_ptr(), dims.data_ptr(), crc.data_ptr(), hdr.data_ptr(), pkt.data_ptr(),
                                           dst.data_ptr(), cap, off.data_ptr(), lo.data_ptr(), _stream())
            torch.cuda.synchronize()
            slab, lens = out.cpu().numpy(), ln.cpu().numpy().view(np.uint32)
            at = 0
            for i, e in enumerate(exp):
                what = (entry, names[i], MODE_NAMES[mode])
                assert int(lens[i]) == len(e) and slab[i * plan.stride:i * plan.stride + len(e)].tobytes() == e, what
                assert int(crc.cpu().numpy().view(np.uint32)[i]) == wire[i][0], what
                if entry != "crc":
                    assert hdr.cpu().numpy()[24 * i:24 * i + 24].tobytes() == wire[i][1], what
                    assert int(pkt.cpu().numpy().view(np.uint32)[i]) == wire[i][2], what
                if entry == "packed":
                    assert int(off.cpu().numpy()[i]) == at and int(lo.cpu().numpy().view(np.uint32)[i]) == len(e), what
                    assert dst.cpu().numpy()[at:at + len(e)].tobytes() == e, what
                    at += (len(e) + 15) // 16 * 16
            if entry == "packed":  # the offsets tile the destination, nothing behind them
                assert int(off.cpu().numpy()[n]) == at and (dst.cpu().numpy()[at:] == GUARD).all()
            assert (slab[n * plan.stride:] == GUARD).all()
    finally:
        plan.close()


@pytest.mark.parametrize("mode", [MODE_TRUE_FG, MODE_HB_TRUE, MODE_MONO], ids=["true_fg", "hb_true", "mono"])
def test_plan_update_between_plain_and_composite_frames(pkg, world, mode):
    """a plan created over plain frames, updated to composite frames and back: the sampler and the geometry follow the frames
    (a fast-sampler launch refuses a composite frame with the bad-descriptor code)"""
    import torch
    cl, rm = MODE_CAPS[mode]
    imgs = [orc.frame_hash_noise(24, 18, 90 + i) for i in range(3)]
    dev = [torch.from_numpy(i).cuda() for i in imgs]
    picked = [BY_NAME["5 equal sources at 60x30"], BY_NAME[CC.ZERO_CELL], BY_NAME["sources of different sizes"]]
    plain = [pkg.frame_setup(d.data_ptr(), 24, 18, 60, 30, rm, True, True, False) for d in dev]
    plain_exp = [orc.convert_with_caps(i, 60, 30, cl, rm, True, True, False) for i in imgs]
    comp = [world.frame(k, mode) for k in picked]
    plan = pkg.Plan(mode, PAL, plain)
    try:
        assert render(plan, 3) == plain_exp
        for _ in range(2):
            plan.update(comp, _stream())
            check(plan, mode, picked, "updated to composite frames")
            plan.update(plain, _stream())
            assert render(plan, 3) == plain_exp, (MODE_NAMES[mode], plan.variant, "back to plain frames")
    finally:
        plan.close()


def test_dirty_padding_word_in_the_host_descriptor(pkg, world):
    """composite_upload clears the word the staged sampler reads for every sample outside the tiles"""
    for name in ("5 equal sources at 60x30", "a wide source"):
        k = BY_NAME[name]
        dirty = pkg.Composite.from_buffer_copy(bytes(world.host[name]))
        dirty._pad = -1
        d = world.upload(dirty)
        try:
            for mode in (MODE_TRUE_FG, MODE_HB_TRUE, MODE_MONO, 2):
                for frames in ([world.frame(k, mode, comp_dev=d)], [world.frame(k, mode, comp_dev=d)] * 3):
                    plan = pkg.Plan(mode, PAL, frames)
                    try:
                        check(plan, mode, [k] * len(frames), "dirty padding word")
                    finally:
                        plan.close()
        finally:
            pkg.lib().asciichat_hip_free(d)


def test_hand_filled_descriptor_without_cells_is_black_for_both_samplers(pkg, world):
    """a descriptor whose cell height a caller zeroed while its tile records stay filled: the global sampler returns black for
    it, and composite_upload leaves it without placed sources so that the staged sampler does too -- the materialised canvas,
    lone frames (row bands: both samplers in one frame) and batches are the oracle's render of a black canvas"""
    import torch
    k = BY_NAME["9 equal sources at 60x30"]
    W, H = k.canvas_dims
    black = np.zeros((H, W, 3), np.uint8)
    for field in ("cell_h", "cell_w", "rows"):
        hand = pkg.Composite.from_buffer_copy(bytes(world.host[k.name]))
        setattr(hand, field, 0)
        assert hand.n_src == 9 and hand.s[8].src and hand.s[8].tile_w > 0
        dst = torch.full((3 * W * H + 256,), GUARD, dtype=torch.uint8, device="cuda")
        assert pkg.lib().asciichat_hip_composite(C.byref(hand), dst.data_ptr(), None) == 0
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert not got[:3 * W * H].any() and (got[3 * W * H:] == GUARD).all(), field
        d = world.upload(hand)
        try:
            for mode in (MODE_TRUE_FG, MODE_HB_TRUE, MODE_MONO, 2):
                cl, rm = MODE_CAPS[mode]
                exp = orc.convert_with_caps(black, k.term[0], k.frame_height(mode), cl, rm, True, True, False)
                for n in (1, 3):
                    plan = pkg.Plan(mode, PAL, [world.frame(k, mode, comp_dev=d)] * n)
                    try:
                        assert render(plan, n) == [exp] * n, (field, MODE_NAMES[mode], n, plan.variant, plan.parts)
                    finally:
                        plan.close()
        finally:
            pkg.lib().asciichat_hip_free(d)


def test_each_kernel_rendered_composites(pkg, world):
    """... and the record of which geometries and modes did (printed: run with -rP)"""
    for mode in (MODE_MONO, MODE_TRUE_FG, MODE_HB_TRUE):  # (what this test needs when it runs alone)
        if ("every case in one plan", MODE_NAMES[mode]) not in CHOSEN:
            mixed(pkg, world, mode)
    assert set(RENDERED) == {"phase", "stream", "rows"}, RENDERED
    assert {v for v, _ in RENDERED["phase"]} >= {0, 4} and {v for v, _ in RENDERED["stream"]} >= {16, 17} and \
        {v for v, _ in RENDERED["rows"]} >= {24, 25}, RENDERED
    assert (18, "true_fg") in RENDERED["stream"], "stream geometry 18 shared out, taken by the plan itself"
    print("COMPOSITE_RECORD " + json.dumps({
        "rendered": {k: sorted(v) for k, v in RENDERED.items()}, "refused": sorted(REFUSED),
        "chosen": {f"{a} / {b}": v for (a, b), v in sorted(CHOSEN.items())}}))
