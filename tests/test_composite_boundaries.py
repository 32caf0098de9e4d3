"""The fused composite sampler under the CPU emulator, on the boundary families of tests/composite_cases.py: the materialised
canvas (composite_kernel: the global sample_composite) and the fused render through every instantiation that carries the
sampler -- the phase kernel whole-frame (sample_composite_lds) and in row bands (the global sampler for the carry pixel in
front of a band), the stream kernel's and the rows kernel's general instantiations -- in every mode those are built for,
against the oracle's canvas and the frame the oracle renders from it.  (tests/test_gpu_composite.py: the same cases on the
device through the C ABI.)"""
import ctypes as C

import numpy as np
import pytest

import composite_cases as CC
import emu
import orc
from achip_ctypes import (ALL_MODES, Uniform, LEN_BADDESC, MODE_16_DITHER_BG, MODE_16_FG, MODE_CAPS, MODE_HB_TRUE, MODE_MONO, MODE_NAMES, MODE_TRUE_BG,
                          MODE_TRUE_FG)
from test_kernels_emulated import ROWS_MODES, STREAM_MODES

CASES = CC.cases()
IDS = [k.name for k in CASES]
PAL = orc.PALETTE_STANDARD

# the widest padded row a geometry holds (render_variants.h: CAP of the phase geometries, 64 * CPL of the rows geometries; the
# stream geometries bound a frame's cells only, far above these cases)
PHASE_CAP = {0: 4096, 2: 1024, 3: 256, 4: 2048}
ROWS_CAP = {24: 448, 25: 256, 28: 128}
CAP = {**PHASE_CAP, **ROWS_CAP, 16: 1 << 20, 17: 1 << 20, 20: 1 << 20}
STREAM = (16, 17, 20)
HALFBLOCK = (5, 6, 7, 8)


def phase_modes(variant):
    """ACHIP_FRAME_VARIANT_HALFBLOCK: no half-block instantiations in geometry 2"""
    return [m for m in ALL_MODES if not (variant == 2 and m in HALFBLOCK)]


def comp_frame(case, comp, mode, ops=None):
    """the frame that renders the case's canvas in `mode`: no source of its own, the canvas's size, the descriptor's address"""
    tw, th = case.term
    f = emu.Frame()
    rm = MODE_CAPS.get(mode, (3, 0))[1]
    assert emu.lib().achip_frame_setup(C.byref(f), None, tw, 2 * th, tw, case.frame_height(mode), rm, True, True, False) == 0
    f.comp = C.addressof(comp)
    if ops:
        assert emu.lib().achip_frame_set_display_ops(C.byref(f), *ops) == 0
        assert f.ops != 0
    return f


def ragged_band(rows, wp, cap):
    """rows per band that leave a ragged last band and fit the geometry's chunk; None when the frame has no such cut"""
    for r in range(2, rows):
        if rows % r and r * wp <= cap:
            return r
    return None


@pytest.fixture(scope="module")
def descriptors():
    L = emu.lib()
    return {k.name: k.host_descriptor(L) for k in CASES}  # (premises asserted)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_materialised_canvas(case, descriptors):
    """composite_kernel = the global sampler at every pixel of the canvas"""
    comp = descriptors[case.name]
    W, H = case.canvas_dims
    out = np.full((H * W * 3 + 64,), 0xEE, np.uint8)
    emu.lib().emu_composite(C.byref(comp), out.ctypes.data)
    assert np.array_equal(out[:H * W * 3].reshape(H, W, 3), case.canvas()), case.name
    assert (out[H * W * 3:] == 0xEE).all(), "bytes behind the canvas were written"


def check(case, comp, mode, variant, what, pair=True, **kw):
    """the frame with both flips and a tint set (the sampler ignores flips for composites, sample_finish skips their tint) and,
    in the emulator's small geometries, the frame without them beside it in the same launch: the oracle's bytes, or the
    row-too-wide code from a geometry that cannot hold the row.  -> whether the geometry rendered it"""
    exp = case.expected(mode)
    frames = [comp_frame(case, comp, mode, (True, True, 3))] + ([comp_frame(case, comp, mode)] if pair else [])
    got = emu.render_frames(mode, frames, PAL, variant, **kw)
    what = (case.name, MODE_NAMES[mode], variant, what)
    if case.term[0] * kw.get("rows_per_part", 1) > CAP[variant]:
        assert got == [LEN_BADDESC] * len(frames), what
        return False
    assert got == [exp] * len(frames), what
    return True


def check_phase(case, comp, variant, band_modes, pair):
    """-> how many launches rendered the case (a geometry that cannot hold the row, or the band, said so instead)"""
    wp, rows = case.term
    held = 0
    for mode in phase_modes(variant):
        if not check(case, comp, mode, variant, "whole", pair):
            continue
        held += 1
        if mode not in band_modes:
            continue
        # row bands: the carry pixel in front of a band comes from the global sampler
        for rpp in (1, ragged_band(rows, wp, CAP[variant])):
            if rpp is not None and rpp < rows:
                held += check(case, comp, mode, variant, f"{rpp} rows per band", pair, rows_per_part=rpp)
    return held


BANDED = [m for m in ALL_MODES if m != MODE_16_DITHER_BG]  # the serial dither is never cut into bands (achip_choose_geometry)
# one mode of each token builder: the short tokens, the per-cell SGRs built as words and as bytes, the half blocks
BANDED_PRODUCT = (MODE_MONO, MODE_TRUE_FG, MODE_16_FG, MODE_HB_TRUE)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_phase_kernel(case, descriptors):
    """the emulator's 64-thread geometry: every case, every mode, whole and in bands of one row and of a ragged cut"""
    held = check_phase(case, descriptors[case.name], 3, BANDED, True)
    assert held >= len(ALL_MODES) + (len(BANDED) if case.term[1] > 1 else 0), (case.name, held)


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("variant", [0, 2, 4])
def test_phase_kernel_product_geometries(case, variant, descriptors):
    """the 512- and 1024-thread geometries (0 and 4 the product's, 2 built with ACHIP_ALL_GEOMETRIES only): every case, every
    mode the geometry is built for whole, and in bands of one row and of a ragged cut in one mode of each token builder (the
    fiber emulator switches among up to 1024 fibers per workgroup: a 60x30 case takes about nine seconds here)"""
    held = check_phase(case, descriptors[case.name], variant, BANDED_PRODUCT, False)
    modes = phase_modes(variant)
    assert held >= len(modes) + (len([m for m in BANDED_PRODUCT if m in modes]) if case.term[1] > 1 else 0), (case.name, variant, held)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stream_kernel(case, descriptors):
    for variant in STREAM:
        for mode in STREAM_MODES:
            assert check(case, descriptors[case.name], mode, variant, "whole", pair=variant == 20)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_kernel(case, descriptors):
    held = 0
    for variant in (24, 25, 28):
        for mode in ROWS_MODES:
            held += check(case, descriptors[case.name], mode, variant, "whole", pair=variant == 28)
    assert held >= 2 * len(ROWS_MODES), case.name


def test_every_case_is_rendered_by_all_three_kernels():
    """the cap: at least one geometry of each kernel holds every case's row (the stream geometries bound cells, not rows), and
    the cases that are about the global sampler have more than one text row to cut into bands"""
    for k in CASES:
        assert any(k.term[0] <= c for c in PHASE_CAP.values()) and any(k.term[0] <= c for c in ROWS_CAP.values()), k.name
    for name in (CC.ZERO_CELL, CC.ALL_NONE, CC.ONE_PIXEL_CELL_H, CC.ONE_PIXEL_CELLS):
        assert next(k for k in CASES if k.name == name).term[1] > 1, name


def test_families_are_complete():
    assert {k.family for k in CASES} == set(CC.FAMILIES)
    assert any(k.term[0] > min(ROWS_CAP.values()) for k in CASES), "no case exercises a geometry's refusal"


# ---- batches ---------------------------------------------------------------------------------------------------------
BATCH_CASES = ["9 equal sources at 60x30", "sources of different sizes", CC.ONE_PIXEL_CELL_H, CC.ZERO_CELL]


@pytest.mark.parametrize("name", BATCH_CASES)
def test_batches_by_value_and_through_the_descriptor_array(name, descriptors):
    case = next(k for k in CASES if k.name == name)
    comp = descriptors[name]
    for mode, variants in ((MODE_TRUE_FG, ((3, 0), (3, 1), (20, 0), (17, 0))), (MODE_HB_TRUE, ((3, 0), (3, 1), (28, 0), (25, 0))),
                           (MODE_MONO, ((28, 0),))):
        f = comp_frame(case, comp, mode)
        uni = Uniform()
        assert emu.lib().achip_frames_uniform((emu.Frame * 3)(f, f, f), 3, C.byref(uni)) == 1 and uni.enabled, "one descriptor for the batch"
        for variant, rpp in variants:
            for uniform in (True, False):
                got = emu.render_frames(mode, [f, f, f], PAL, variant, rows_per_part=rpp, uniform=uniform)
                assert got == [case.expected(mode)] * 3, (name, MODE_NAMES[mode], variant, rpp, uniform)


# ---- one launch of the general instantiation with everything it serves ---------------------------------------------------
def _plain(img, W, H, mode, ops=None):
    f = emu.frame_for_convert(img, W, H, MODE_CAPS[mode][1], True, True)
    if ops:
        assert emu.lib().achip_frame_set_display_ops(C.byref(f), *ops) == 0
    return f


@pytest.mark.parametrize("mode,variant,rpp", [(MODE_TRUE_FG, 3, 0), (MODE_TRUE_FG, 3, 1), (MODE_TRUE_FG, 3, 4), (MODE_TRUE_FG, 20, 0), (MODE_TRUE_FG, 17, 0),
                                              (2, 20, 0), (MODE_HB_TRUE, 3, 0), (MODE_HB_TRUE, 3, 1), (MODE_HB_TRUE, 28, 0), (MODE_HB_TRUE, 25, 0),
                                              (MODE_MONO, 28, 0), (7, 3, 3)])
def test_mixed_launch(mode, variant, rpp, descriptors):
    """frames of two different composites (one with display ops set), a plain frame with both flips and a tint, a plain frame
    with a 1x1 source and a frame with neither a source nor a composite, in ONE launch: each its own oracle's bytes, the plain
    frame's tint applied and the composite's not, the last one the bad-descriptor code"""
    a = next(k for k in CASES if k.name == "sources of different sizes")
    b = next(k for k in CASES if k.name == "7 equal sources at 60x30")
    cl, rm = MODE_CAPS[mode]
    img, dot = orc.frame_hash_noise(24, 18, 7), orc.frame_hash_noise(1, 1, 9)
    bad = comp_frame(a, descriptors[a.name], mode)
    bad.comp = None
    frames = [comp_frame(a, descriptors[a.name], mode, (True, True, 3)), _plain(img, 30, 12, mode, (True, True, 3)),
              comp_frame(b, descriptors[b.name], mode), _plain(dot, 9, 5, mode), bad, comp_frame(a, descriptors[a.name], mode)]
    assert frames[0].ops and frames[1].ops
    tinted = orc.display_convert(img, 30, 12, cl, rm, True, True, True, True, 3)
    assert tinted != orc.display_convert(img, 30, 12, cl, rm, True, True, False, False, 0), "the tint and the flips show in this mode"
    exp = [a.expected(mode), tinted, b.expected(mode), orc.convert_with_caps(dot, 9, 5, cl, rm, True, True, False), LEN_BADDESC,
           a.expected(mode)]
    got = emu.render_frames(mode, frames, PAL, variant, rows_per_part=rpp)
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g == e, (MODE_NAMES[mode], variant, rpp, k)


# ---- the frame CRC riding the drain --------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [20, 17, 25, 28])
def test_fused_crc_over_composite_frames(variant, descriptors):
    names = ["9 equal sources at 60x30", "sources of different sizes", "a 1x1 source", "10 sources at 80x30", CC.ONE_PIXEL_CELL_H,
             CC.ONE_PIXEL_CELLS, CC.ZERO_CELL, CC.ALL_NONE]
    picked = [k for k in CASES if k.name in names]
    assert len(picked) == len(names)
    for mode in (ROWS_MODES if variant >= 24 else STREAM_MODES):
        frames = [comp_frame(k, descriptors[k.name], mode) for k in picked]
        dims = [k.term for k in picked]
        got, crc, hdr, pkt = emu.render_frames_crc(mode, frames, PAL, variant, dims=dims)
        for i, k in enumerate(picked):
            exp = k.expected(mode)
            what = (k.name, MODE_NAMES[mode], variant)
            assert got[i] == exp, what
            assert (crc[i], hdr[i], pkt[i]) == CC.wire_expect(exp, *k.term), what
