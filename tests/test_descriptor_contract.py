"""The frame descriptor's sampling rule (include/achip_types.h achip_frame_t) in every kernel form the emulator builds, on
descriptors that achip_frame_setup never produces: hand-set ratios (ratio 1.0 on mismatched sizes, up-sampling, the largest
accepted ratio), padded source rows, flips, colour filters, degenerate shapes, pads.  Each source sits in a guarded buffer
(tests/descriptor_ref.py) and every frame is compared byte for byte with the reference's output for the pixels the rule
addresses.  Then the refusal contract: a refused frame between two good ones, in every form that has one."""
import ctypes as C

import numpy as np
import pytest

import descriptor_ref as ref
import emu
import orc
from achip_ctypes import (ALL_MODES, MODE_16_DITHER_BG, MODE_16_FG, MODE_256_FG, MODE_CAPS, MODE_HB_16, MODE_HB_256,
                          MODE_HB_MONO, MODE_HB_TRUE, MODE_MONO, MODE_NAMES, MODE_TRUE_BG, MODE_TRUE_FG, Frame)

PAL = orc.PALETTE_STANDARD
BADDESC = 0xFFFFFFFE
STREAM_MODES = (MODE_TRUE_FG, MODE_256_FG, MODE_16_FG, MODE_TRUE_BG)
PACK_MODES = (MODE_TRUE_FG, MODE_256_FG, MODE_16_FG)
ROWS_MODES = (MODE_MONO, MODE_HB_TRUE, MODE_HB_256, MODE_HB_16, MODE_HB_MONO)
PHASE_CAPS = (4096, 2048, 1024, 256, 2048)  # render_variants.h ACHIP_VARIANTS: the longest padded row of geometries 0-4


def forced_applies(mode, frames, variant):
    """whether a plan forced to `variant` would launch these frames (achip_choose_geometry's forced_applies)"""
    L = emu.lib()
    arr = (Frame * len(frames))(*frames)
    caps = (C.c_int * len(PHASE_CAPS))(*PHASE_CAPS)
    v, p, r = C.c_int(-1), C.c_int(0), C.c_int(0)
    rc = L.achip_choose_geometry(mode, arr, len(frames), True, caps, 256, -1, variant, C.byref(v), C.byref(p), C.byref(r))
    return rc == 0 and v.value == variant


# (name, modes, variant, how): every form of every kernel family the emulator instantiates
HB_MODES = (MODE_HB_TRUE, MODE_HB_256, MODE_HB_16, MODE_HB_MONO)
FORMS = [(f"phase{v}", tuple(m for m in ALL_MODES if not (v in (1, 2) and m in HB_MODES)), v, "slab") for v in range(5)] + [
    ("bands", tuple(m for m in ALL_MODES if m != MODE_16_DITHER_BG), 0, "bands"),
    *[(f"stream{v}", STREAM_MODES, v, "slab") for v in (16, 17, 19, 20)],
    ("stream18_parts", STREAM_MODES, 18, "parts"),
    *[(f"stream{v}_crc", STREAM_MODES, v, "crc") for v in (17, 20)],
    *[(f"packed{v}", PACK_MODES, v, "packed") for v in (16, 17, 20)],
    *[(f"packed{v}_crc", PACK_MODES, v, "packed_crc") for v in (17, 20)],
    *[(f"lenfirst{v}", (MODE_TRUE_FG,), v, "lenfirst") for v in (16, 17, 20)],
    *[(f"rows{v}", ROWS_MODES, v, "slab") for v in (24, 25, 26, 27, 29)],
    *[(f"rows{v}_parts", ROWS_MODES, v, "parts") for v in (31, 32)],
    *[(f"rows{v}_crc", ROWS_MODES, v, "crc") for v in (24, 25, 26)],
]
PAIRS = [(m, name, v, how) for (name, modes, v, how) in FORMS for m in modes]


def render(mode, variant, how, frames, cursor=None):
    """-> ([bytes | error code] per frame, extras): every frame of the launch through one kernel form; slot guards and the
    packed forms' tiling and cursor words are checked on the way"""
    if how == "slab":
        return emu.render_frames(mode, frames, PAL, variant, line_phase=0), None
    if how == "bands":
        return emu.render_frames(mode, frames, PAL, variant, rows_per_part=7, line_phase=0), None
    if how == "parts":
        return emu.render_frames(mode, frames, PAL, variant, parts=3 if variant >= 24 else 4, line_phase=1), None
    if how == "crc":
        res, crc = emu.render_frames_crc(mode, frames, PAL, variant)
        return res, crc
    if how in ("packed", "packed_crc"):
        res = emu.render_frames_packed(mode, frames, PAL, variant, want_crc=how == "packed_crc", cursor=cursor)
    else:
        res = emu.render_frames_length_first(frames, PAL, variant, cursor=cursor)
    out = []
    for k in range(len(frames)):
        n = int(res["lens"][k])
        out.append(n if n >= 0xFFFFFFF0 else res["dst"][int(res["off"][k]):int(res["off"][k]) + n].tobytes())
    return out, res


def check_launch(mode, name, variant, how, built, what, refused=False):
    """every frame of `built` in one launch byte-exact against descriptor_ref -- or, `refused`, every one ACHIP_LEN_BADDESC"""
    frames = [f for (_, _, f) in built]
    got, extra = render(mode, variant, how, frames)
    exp = [BADDESC if refused else ref.expected(mode, f, g.buf) for (_, g, f) in built]
    for (c, _, _), e, r in zip(built, exp, got):
        assert r == e, (MODE_NAMES[mode], name, what, c)
    if how == "crc" or how == "packed_crc":
        crcs = extra if how == "crc" else extra["crc"]
        for (c, _, _), e, k in zip(built, exp, range(len(exp))):
            assert int(crcs[k]) == (0 if refused else orc.crc32c(e)), (MODE_NAMES[mode], name, what, c)
    if how in ("packed", "packed_crc", "lenfirst"):
        emu.check_packed(extra, exp, (MODE_NAMES[mode], name, what))


def _launch_groups(cases):
    """the sources that take the fast sampler together; the 1x1 sources (the general sampler) in launches of their own"""
    return [c for c in cases if c.sw * c.sh > 1]


RANDOM = ref.random_cases(7, 48)
_BUILT = {}


def built(key):
    """the guarded sources of one case list, built once per process (read-only for every launch)"""
    if key not in _BUILT:
        if key == "named":
            _BUILT[key] = ref.build(_launch_groups(ref.NAMED))
        elif key == "1x1":
            _BUILT[key] = ref.build(ref.ONE_BY_ONE)
        else:  # ("random", k): a quarter of the random mix
            _BUILT[key] = ref.build(RANDOM[key[1]::4], seed=100 + key[1])
    return _BUILT[key]


@pytest.mark.parametrize("mode,name,variant,how", PAIRS, ids=[f"{MODE_NAMES[m]}-{n}" for (m, n, _, _) in PAIRS])
def test_every_form_follows_the_descriptor_rule(mode, name, variant, how):
    """the named cases in one launch (and a sample of the random ones in another): a form the plan would never launch with
    these frames is not asked (forced_applies); every form it would launch renders every frame byte-exact -- none refused"""
    named = built("named")
    assert forced_applies(mode, [f for (_, _, f) in named], variant) or (how == "bands"), (name, "takes the named cases")
    # the flipped ratio-1.0 cases on smaller sources in a launch of their own, behind the others: an unclamped sampler
    # reads about 4 GB away from them (a fault, where the unflipped ones show the sentinel as wrong bytes first)
    check_launch(mode, name, variant, how, [b for b in named if b[0].name not in ref.FLIP_UNCLAMPED], "named")
    check_launch(mode, name, variant, how, [b for b in named if b[0].name in ref.FLIP_UNCLAMPED], "named, flipped")
    # a sample of the random mix: a different quarter per (mode, form), all of it over the whole matrix
    k = PAIRS.index((mode, name, variant, how)) % 4
    rnd = built(("random", k))
    assert forced_applies(mode, [f for (_, _, f) in rnd], variant) or how == "bands", (name, "takes the random cases")
    check_launch(mode, name, variant, how, rnd, "random")
    # 1x1 sources: the general sampler.  The rows geometries without it are never given one by a plan (forced_applies); the
    # packed forms are fast-sampler instantiations and refuse every 1x1 frame; the length-first form is never launched with
    # one (the launchers, and the emulator's driver, refuse the launch)
    if how == "lenfirst":
        return
    one = built("1x1")
    takes = forced_applies(mode, [f for (_, _, f) in one], variant)
    assert takes == (variant not in (26, 27, 29, 31, 32)), name
    if takes or how == "bands":
        check_launch(mode, name, variant, how, one, "1x1", refused=how in ("packed", "packed_crc"))


@pytest.mark.parametrize("mode", ALL_MODES, ids=MODE_NAMES)
@pytest.mark.parametrize("padding,aspect", [(False, False), (True, True), (False, True)])
def test_reference_composition_matches_convert_with_caps(mode, padding, aspect):
    """self-check of descriptor_ref before it judges any kernel: on the descriptors achip_frame_setup builds, `expected`
    equals the oracle's own ascii_convert_with_capabilities byte for byte"""
    for (sw, sh, W, H) in ((97, 53, 40, 12), (320, 240, 61, 19), (13, 9, 30, 20), (8, 30, 17, 5)):
        img = ref.source_image(sw, sh, sw + sh)
        if mode == MODE_TRUE_BG:  # reachable through image_print_color_background only: no aspect, no padding
            if padding or aspect:
                continue
            f = emu.frame_for_convert(img, W, H, 0)
            want = orc.print_truecolor_bg(orc.resize_nn(img, W, H), PAL)
        else:
            cl, rm = MODE_CAPS[mode]
            f = emu.frame_for_convert(img, W, H, rm, padding, aspect)
            want = orc.convert_with_caps(img, W, H, cl, rm, padding, aspect, False, PAL)
        flat = img.reshape(-1)
        assert ref.expected(mode, f, flat, PAL, base_offset=0) == want, (MODE_NAMES[mode], sw, sh, W, H, padding, aspect)


def test_plans_refuse_ratios_whose_products_wrap_32_bits():
    """(out_w - 1) * x_ratio and (out_h - 1) * y_ratio below 2^32 (achip_frame_ratios_ok): the kernels' 32-bit sample index
    never wraps, so every form samples what the rule says.  A 70 000-pixel-wide source at 80 columns wraps five columns."""
    L = emu.lib()
    L.achip_frame_ratios_ok.restype = C.c_bool
    L.achip_frame_ratios_ok.argtypes = [C.POINTER(Frame)]
    top = (1 << 32) - 1
    for (ow, oh, xr, yr, ok) in ((16, 4, top // 15, top // 3, True), (17, 4, 1 << 28, 1, False), (16, 5, top // 15, 1 << 30, False),
                                 (1, 1, top, top, True), (80, 1, int(L.achip_nn_ratio(70000, 80)), 65537, False),
                                 (80, 24, int(L.achip_nn_ratio(10000, 80)), int(L.achip_nn_ratio(10000, 24)), True),
                                 (2, 2, 1 << 31, (1 << 32) - 1, True)):
        f = ref.make_frame(ref.Case("r", 40, 30, ow, oh, xr, yr, 0, 0, 0, 0, 0), 1)
        assert L.achip_frame_ratios_ok(C.byref(f)) == ok, (ow, oh, xr, yr)
        assert ref.ratio_ok(ref.Case("r", 40, 30, ow, oh, xr, yr, 0, 0, 0, 0, 0)) == ok
    assert all(ref.ratio_ok(c) for c in ref.NAMED + ref.ONE_BY_ONE + RANDOM)


# (name, modes, variant, how) of every form with a refusal contract, and what refuses there: a 1x1 source on the fast
# sampler (the driver's general-sampler gate held open: emu_set_fast_sampler_only).  The stream kernel's CRC instantiation
# carries the general sampler (it renders a 1x1 source), and so does its shared-out instantiation (geometry 18): those forms
# have nothing here to refuse.
REFUSING = [f for f in FORMS if (f[3] in ("slab", "packed", "packed_crc", "lenfirst") or (f[3] in ("crc", "parts") and f[2] >= 24))
               and f[2] >= 16]
REFUSE_PAIRS = [(m, name, v, how) for (name, modes, v, how) in REFUSING for m in modes]


@pytest.mark.parametrize("mode,name,variant,how", REFUSE_PAIRS, ids=[f"{MODE_NAMES[m]}-{n}" for (m, n, _, _) in REFUSE_PAIRS])
def test_a_refused_frame_leaves_its_neighbours_and_the_cursor_intact(mode, name, variant, how):
    """[good, refused, good] with the fast sampler only: the 1x1 source reports ACHIP_LEN_BADDESC (a zero CRC, a header of
    zeros), its neighbours are byte-exact, and in the packed and length-first forms off_out[n] is the total, both cursor
    words are back at 0 and a second launch on the same cursor places every frame again"""
    good = ref.build([ref.case("g0", 40, 24, 20, 10, pl=2, pt=1), ref.case("g2", 30, 14, 30, 14, 65537, 65537, ops=ref.FLIP_X)])
    bad = ref.build([ref.case("src_1x1", 1, 1, 9, 5)])
    built = [good[0], bad[0], good[1]]
    frames = [f for (_, _, f) in built]
    exp = [ref.expected(mode, f, g.buf) for (_, g, f) in good]
    L = emu.lib()
    L.emu_set_fast_sampler_only.restype = C.c_int
    L.emu_set_fast_sampler_only.argtypes = [C.c_int]
    L.emu_set_fast_sampler_only(1)
    try:
        if how in ("packed", "packed_crc", "lenfirst"):
            cursor = np.zeros(2, dtype=np.uint64)
            for launch in range(2):
                got, res = render(mode, variant, how, frames, cursor=cursor)
                assert got == [exp[0], BADDESC, exp[1]], (name, launch)
                emu.check_packed(res, [exp[0], BADDESC, exp[1]], (name, launch))  # tiling, total in off_out[n], cursor at 0
                assert not cursor.any(), (name, launch, cursor)
                if how == "packed_crc":
                    assert [int(c) for c in res["crc"]] == [orc.crc32c(exp[0]), 0, orc.crc32c(exp[1])]
            return
        dims = [(20, 10), (9, 5), (30, 14)]
        if how == "crc":
            got, crc, hdr, pkt = emu.render_frames_crc(mode, frames, PAL, variant, dims=dims)
            assert crc == [orc.crc32c(exp[0]), 0, orc.crc32c(exp[1])], name
            assert hdr[1] == bytes(24), name
        else:
            got, _ = render(mode, variant, how, frames)
        assert got == [exp[0], BADDESC, exp[1]], name
    finally:
        L.emu_set_fast_sampler_only(0)


def test_the_plan_takes_the_largest_ratio_and_refuses_the_next():
    """On the mock plan (the product's host C, kernels under the emulator): (out_w - 1) * x_ratio == 2^32 - 1 is accepted and
    rendered exactly, 2^32 is refused with ASCIICHAT_HIP_ERR_INVALID_PARAM, in x and in y -- and so is the 70 000-pixel-wide
    source at 80 columns whose columns wrap, whatever geometry is asked for (the forms would disagree on it: the lean loop's
    split multiply is exact, the others wrap)"""
    import mockgpu
    pkg = mockgpu.package()
    top = (1 << 32) - 1
    (c, g, f), = ref.build([ref.case("largest", 50, 30, 16, 4, top // 15, top // 3, pl=1, pt=1)])
    for mode in (MODE_TRUE_FG, MODE_256_FG, MODE_MONO, MODE_HB_TRUE):
        plan = pkg.Plan(mode, PAL, [ref.as_frame(pkg.Frame, f)])
        out = np.full(plan.stride + 16, 0xEE, dtype=np.uint8)
        ln = np.zeros(1, dtype=np.uint32)
        plan.render(out.ctypes.data, plan.stride, ln.ctypes.data)
        assert out[:int(ln[0])].tobytes() == ref.expected(mode, f, g.buf), MODE_NAMES[mode]
        plan.close()
    wide = np.ascontiguousarray(ref.source_image(70000, 2, 5))
    L = emu.lib()
    for (sw, sh, ow, oh, xr, yr) in ((50, 30, 17, 4, 1 << 28, top // 3), (50, 30, 16, 5, top // 15, 1 << 30),
                                     (70000, 2, 80, 1, int(L.achip_nn_ratio(70000, 80)), int(L.achip_nn_ratio(2, 1)))):
        bad = ref.make_frame(ref.Case("wraps", sw, sh, ow, oh, xr, yr, 0, 0, 0, 0, 0), wide.ctypes.data if sw == 70000 else g.src)
        for mode in (MODE_TRUE_FG, MODE_256_FG, MODE_MONO):
            with pytest.raises(RuntimeError, match=r"2\^32"):
                pkg.Plan(mode, PAL, [ref.as_frame(pkg.Frame, bad)])


def test_plans_refuse_to_force_the_shared_out_rows_geometries():
    """a forced geometry renders whole frames, without the hand-off words a shared-out rows kernel (31-34) publishes to even
    as one part: set_variant refuses those geometries and the plan keeps rendering what it rendered before"""
    import mockgpu
    pkg = mockgpu.package()
    (c, g, f), = ref.build([ref.case("g", 40, 24, 20, 10, pl=1)])
    plan = pkg.Plan(MODE_MONO, PAL, [ref.as_frame(pkg.Frame, f)])
    before = plan.variant
    for v in (31, 32, 33, 34):
        with pytest.raises(RuntimeError, match="shares frames out"):
            plan.set_variant(v)
        assert plan.variant == before
    out = np.full(plan.stride + 16, 0xEE, dtype=np.uint8)
    ln = np.zeros(1, dtype=np.uint32)
    plan.render(out.ctypes.data, plan.stride, ln.ctypes.data)
    assert out[:int(ln[0])].tobytes() == ref.expected(MODE_MONO, f, g.buf)
    plan.close()


def test_forced_geometries_agree_with_the_policy_on_the_mock():
    """the GPU test renders every geometry a plan may be forced to: on the mock plan (the product's host C), set_variant takes
    exactly the geometries achip_choose_geometry says apply to the named cases (descriptor_ref.forced_geometries), every
    mode keeps at least one, and the shared-out rows geometries are refused"""
    import mockgpu
    pkg = mockgpu.package()
    frames = [ref.as_frame(pkg.Frame, f) for (_, _, f) in built("named")]
    want = {MODE_16_DITHER_BG: [0, 1, 2, 3, 4]}
    for mode in ALL_MODES:
        taken = ref.forced_geometries(pkg, mode, frames, (0, 1, 2, 3, 4, 16, 17, 18, 19, 20, 24, 25, 26, 27, 29))
        if mode in HB_MODES:
            assert taken == [0, 3, 4, 24, 25, 26, 27, 29], MODE_NAMES[mode]
        elif mode in STREAM_MODES:
            assert taken == [0, 1, 2, 3, 4, 16, 17, 18, 19, 20], MODE_NAMES[mode]
        elif mode == MODE_MONO:
            assert taken == [0, 1, 2, 3, 4, 24, 25, 26, 27, 29], MODE_NAMES[mode]
        else:
            assert taken == want[mode], MODE_NAMES[mode]
