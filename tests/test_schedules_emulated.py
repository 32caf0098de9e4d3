"""The emulated kernels under more than one schedule (tests/hipemu/hip_emu.h, tests/emu_schedule.py).

The ascending schedule, which every other emulated test runs, is the most regular one there is: lower waves always first, every
wave one step per sweep, workgroups in launch order.  The hot kernels are the ones whose correctness depends on what the OTHER
waves have done so far -- decoupled look-backs over LDS words, segment waits backwards and forwards, "the last span to arrive
combines", places claimed with one atomic add.  Here the frames, cases and checks of the existing emulated tests of each family
run again under DESC, LATE and RANDOM wave schedules, and -- where the launch's workgroups do not wait for one another -- under
other workgroup orders.  The expectation is always what those tests compare with (the oracle, the restatements), never the
ascending run of the kernel itself; every wave schedule here is one the hardware may produce, so a difference is a kernel bug.

LATE comes in two forms.  LATE(w, k) as hip_emu.h defines it holds wave w during the first k sweeps of each workgroup.  Every
render kernel ends its prologue in a block barrier, so that form makes EVERY wave wait at the barrier for the held one, and
nobody in a look-back: in today's kernels its nap counts equal the ascending run's.  LATE(w, k, after=1) starts the k sweeps when the prologue's barrier is released: the late-arriving predecessor in
the middle of the hand-offs.  Both forms run, at k = 1, a middle value and LARGE_K.

A failure names the case and the schedule; `with scheduled(library, Schedule.parse("<that text>"))` around the case replays it.
"""
import numpy as np
import pytest

import crc_cases as CC
import emu
import orc
import raster_support as RAS
import zhuf_ref as Z
import zpack_cases as ZC
import zpack_support as ZS
import zseq_cases as SC
import zwide_support as WS
import zwire as ZW
from achip_ctypes import (MODE_16_FG, MODE_256_FG, MODE_CAPS, MODE_HB_256, MODE_HB_16, MODE_HB_MONO, MODE_HB_TRUE, MODE_MONO, MODE_NAMES,
                          MODE_TRUE_BG, MODE_TRUE_FG)
from emu_schedule import DEFAULT, Schedule, scheduled
from test_kernels_emulated import TORTURE, oracle_convert, run_frames

# a poll of a look-back or of a segment wait is two ballots = four sweeps, so a wave held for LARGE_K sweeps costs each lane that
# waits for it some LARGE_K / 4 naps: far above the handful an ascending run loses, far below the 2^21 polls of a time-out
KS = (1, 30, 300)
LARGE_K = KS[-1]
TEST_SEEDS, PRODUCT_SEEDS = range(8), range(3)
WG_ORDERS = [Schedule().workgroups("desc")] + [Schedule().workgroups("shuffle", s) for s in range(4)]

# waves per workgroup of every geometry used below (render_variants.h); TEST = the emulator's own small geometries
WAVES = {3: 16, 2: 16, 20: 2, 16: 16, 17: 8, 18: 4, 28: 2, 30: 4, 33: 2, 34: 2, 24: 8, 25: 8, 26: 16, 27: 16, 29: 8, 31: 4, 32: 4}
TEST = {20, 28, 30, 33, 34}


def wave_schedules(waves, test_geometry, held=None, seeds=None):
    """DESC; LATE of every wave (test geometries) or of waves 0, 1 and the last (product geometries), from the workgroup's start
    and from its first barrier, at three k; RANDOM with 8 / 3 seeds.  held / seeds: other waves to hold, other seeds"""
    if held is None:
        held = range(waves) if test_geometry else sorted({0, 1 % waves, waves - 1})
    if seeds is None:
        seeds = TEST_SEEDS if test_geometry else PRODUCT_SEEDS
    late = [Schedule.late(w, k, after) for after in (0, 1) for w in held for k in KS]
    return [Schedule.desc()] + late + [Schedule.random(s) for s in seeds]


def under(lib, what, schedules, run):
    """run() -- which checks its own results -- under the default and under every schedule -> {schedule: naps}"""
    naps = {}
    for s in [DEFAULT] + list(schedules):
        try:
            with scheduled(lib, s) as r:
                run()
        except AssertionError as e:
            raise AssertionError(f"case [{what}] under [{s}]: {e}") from None
        naps[s] = r.naps
    return naps


def assert_the_wait_paths_ran(naps, what):
    """the coverage condition: a schedule of the sweep made lanes wait more often than the ascending run did, and a wave held
    LARGE_K sweeps behind the prologue was waited for"""
    asc = naps[DEFAULT]
    assert max(naps.values()) > asc, (what, "no schedule reached a wait path the ascending run does not reach")
    held = [n for s, n in naps.items() if s.waves == "late" and s.late_after == 1 and s.late_sweeps == LARGE_K]
    assert max(held) > asc + 64 * (LARGE_K // 8), (what, "nobody waited for a held wave", asc, held)


# ---- the render kernels --------------------------------------------------------------------------------------------------------
def render(mode, frames, palette, variant, **kw):
    """emu.render_frames with the guard bytes in front of the slab, behind every frame and behind the slab checked"""
    return emu.render_frames(mode, frames, palette, variant, line_phase=0, **kw)


def convert_case(img, mode, W, H, palette, variant, pad=False, **kw):
    """-> (name, run) of one frame against the oracle"""
    rm = MODE_CAPS.get(mode, (3, 0))[1]
    exp = oracle_convert(img, mode, W, H, palette, pad, pad)
    f = emu.frame_for_convert(img, W, H, rm, pad, pad)
    name = f"{MODE_NAMES[mode]} {W}x{H} geometry {variant} source {img.shape} palette {palette!r} pad {pad} {kw}"

    def run():
        got = render(mode, [f], palette, variant, **kw)[0]
        assert isinstance(got, bytes) and len(got) == len(exp) and got == exp, ("length", got if isinstance(got, int) else len(got), len(exp))
    run.keep = (img, f)
    return name, run


def sweep(cases, variant, wait_paths, each=()):
    """every case under the geometry's wave schedules; wait_paths: the coverage condition on the naps summed over the cases, and
    for the cases named in `each` on the case's own naps, so that a case whose wait path is never reached cannot hide"""
    total = {}
    for name, run in cases:
        naps = under(emu.lib(), name, wave_schedules(WAVES[variant], variant in TEST), run)
        for s, n in naps.items():
            total[s] = total.get(s, 0) + n
        if name in each:
            assert_the_wait_paths_ran(naps, name)
    if wait_paths:
        assert_the_wait_paths_ran(total, f"geometry {variant}")
    return total


def _u8_frames():
    """test_stream_kernel_truecolor_with_multibyte_palettes' frames: long stretches without an ASCII cell, more than 64 blocks of
    geometry 20 between two ASCII cells (the RLE look-back walks further back), a colour that returns behind a multi-byte island"""
    wide = orc.frame_hash_noise(1920, 54, 11)
    wide[:, 600:1400] = (3, 3, 3)
    wide[10:30, 800:1000] = (250, 250, 250)
    flat = np.zeros((40, 97, 3), np.uint8)
    flat[:, :] = (200, 220, 240)
    flat[20:, 50:] = (1, 2, 3)
    far = np.full((50, 120, 3), 240, np.uint8)
    far[0, 0:3] = (2, 2, 2)
    far[-1, -5:] = (2, 2, 2)
    return [(wide, 200, 12), (flat, 97, 40), (far, 120, 50), (255 - far, 120, 50)]


def _lean_frames():
    """test_stream_kernel_lean_loop_orders_and_samplers' two cell orders: samples 72 bytes apart (slot-major), ratio 1.0 (lane-major)"""
    wide = orc.frame_hash_noise(1920, 54, 11)
    wide[:, 700:1300] = wide[20, 700]
    dense = orc.frame_hash_noise(97, 31, 5)
    dense[7:9, :] = (9, 200, 31)
    dense[8, 40:] = (255, 255, 255)
    return [(wide, 80, 24), (dense, 97, 31)]


STREAM_MODES = [MODE_TRUE_FG, MODE_256_FG, MODE_16_FG, MODE_TRUE_BG]


@pytest.mark.parametrize("variant", [20, 16, 17, 18])
def test_stream_kernel_look_back(variant):
    """render_stream.hpp stream_lookback / stream_lookback_rle: a prefix found at once, 64 own counts taken and the walk going on,
    a spin on a predecessor that has not published.  Geometry 20 with the frames of 188 blocks (windows beyond 64 predecessors);
    16 and 17 whole frames; 18 a frame's blocks shared out over four workgroups (which wait for one another: ascending order)"""
    kw = dict(parts=4) if variant == 18 else {}
    cases, each = [], []
    for mode in STREAM_MODES:
        pad = mode != MODE_TRUE_BG
        big = (200, 60) if variant == 20 and mode == MODE_256_FG else (97, 31)  # (188 blocks; the U8 frames below: 94)
        cases.append(convert_case(TORTURE, mode, *big, orc.PALETTE_STANDARD, variant, pad, **kw))
        each.append(cases[-1][0])
    cases.append(convert_case(TORTURE, MODE_16_FG, 65, 3, orc.PALETTE_STANDARD, variant, **kw))
    for img, W, H in _lean_frames():  # both cell orders of the lean loop
        cases.append(convert_case(img, MODE_TRUE_FG, W, H, orc.PALETTE_STANDARD, variant, **kw))
    if variant != 18:  # ACHIP_STREAM_MODE_TRUE_FG_U8: the RLE look-back (the driver picks it by the palette, whole frames only)
        for img, W, H in _u8_frames() if variant == 20 else _u8_frames()[:2]:
            cases.append(convert_case(img, MODE_TRUE_FG, W, H, orc.PALETTE_BLOCKS, variant))
            each.append(cases[-1][0])
        cases.append(convert_case(TORTURE, MODE_TRUE_FG, 80, 24, "é漢😀 .m", variant))
    sweep(cases, variant, wait_paths=True, each=each)  # (each: the frames beyond 64 predecessors, the BLOCKS-palette frames)


ROWS_MODES = [MODE_MONO, MODE_HB_TRUE, MODE_HB_256, MODE_HB_16, MODE_HB_MONO]
# (geometry, parts, [(W, H)]): the emulator's 28 (blocks of several rows), 30 (WIDE: four 64-cell segments; 256 = a row of the
# maximum segment count), 33 (PARTS), 34 (WIDE + PARTS: 128 = two segments, the maximum); the product's plain 24 / 25,
# sixteen-wave 26, WIDE 27 (3840: twelve segments, the widest row the existing tests render) / 29 (2560: eight segments, the
# maximum), PARTS 31, WIDE + PARTS 32 (512: four segments, the maximum).  Launches with parts > 1 wait for one another.
ROWS_GEOMETRIES = [(28, 0, [(100, 9), (37, 11)]), (30, 0, [(256, 3), (200, 7), (129, 6)]), (33, 4, [(60, 7), (64, 9)]),
                   (34, 3, [(128, 7), (100, 6)]), (24, 0, [(440, 4)]), (25, 0, [(250, 6), (80, 24)]), (26, 0, [(90, 33)]),
                   (27, 0, [(1000, 2), (3840, 1)]), (29, 0, [(640, 3), (2560, 1)]), (31, 6, [(80, 24), (120, 9)]), (32, 3, [(512, 3), (300, 5)])]


@pytest.mark.parametrize("variant,parts,dims", ROWS_GEOMETRIES, ids=[f"geometry{g[0]}" for g in ROWS_GEOMETRIES])
def test_rows_kernel_segment_waits(variant, parts, dims):
    """render_rows.hpp rows_seg_wait / rows_seg_back (segments wait for the neighbouring segments of their row, backwards AND
    forwards) and the blocks' look-back: mono and the half-block modes on flat frames (only flat areas make segments wait: one run
    per row, its count summed over the segments), 7-cell blocks that straddle the boundaries, and the torture image"""
    kw = dict(parts=parts) if parts else {}
    cases = []
    W, H = dims[0]
    each = []
    for mode in ROWS_MODES:
        cases.append(convert_case(run_frames(W, 2 * H, "flat"), mode, W, H, orc.PALETTE_STANDARD, variant, **kw))
        each.append(cases[-1][0])
    cases.append(convert_case(run_frames(W, 2 * H, "blocks"), MODE_HB_256, W, H, orc.PALETTE_STANDARD, variant, **kw))
    cases.append(convert_case(TORTURE, MODE_HB_TRUE, W, H, orc.PALETTE_STANDARD, variant, **kw))
    for W, H in dims[1:]:
        for mode in (MODE_MONO, MODE_HB_TRUE):
            cases.append(convert_case(run_frames(W, 2 * H, "flat"), mode, W, H, orc.PALETTE_STANDARD, variant, **kw))
            each.append(cases[-1][0])
    sweep(cases, variant, wait_paths=True, each=each)  # (each: the flat frames)


@pytest.mark.parametrize("variant", [3])
def test_frame_kernel_chunks_and_staging(variant):
    """render_kernels.hpp render_frames_kernel (geometry 3): frames of several chunks, and the half-block modes'
    OR-filled staging, whose groups other threads zero again -- ordered by a barrier (test_tall_padding_crosses_threads_groups'
    tall padding: the newline fill of one thread lands in groups that others zero).  Only barriers order this kernel's waves, so
    no schedule may tell, and nobody naps"""
    from achip_ctypes import ALL_MODES
    cases = [convert_case(TORTURE, mode, 97, 31, orc.PALETTE_STANDARD, variant, mode != MODE_TRUE_BG) for mode in ALL_MODES]
    cases += [convert_case(orc.frame_hash_noise(320, 200, 17), mode, 200, 60, orc.PALETTE_STANDARD, variant) for mode in (MODE_TRUE_FG, MODE_HB_TRUE, MODE_MONO)]
    small = orc.frame_hash_noise(7, 2, 3)
    cases += [convert_case(small, mode, W, H, "@", variant, True) for (W, H, mode) in ((1, 2001, 5), (40, 2500, 6))]
    naps = sweep(cases, variant, wait_paths=False)
    assert not any(naps.values()), "the frame kernel has no polling loop"


# ---- fused CRC, PACK, length-first ---------------------------------------------------------------------------------------------
def _crc_case(mode, imgs, dims, variant):
    rm = MODE_CAPS.get(mode, (3, 0))[1]
    frames = [emu.frame_for_convert(im, w, h, rm) for im, (w, h) in zip(imgs, dims)]
    exp = [oracle_convert(im, mode, w, h, orc.PALETTE_STANDARD) for im, (w, h) in zip(imgs, dims)]
    want = [(orc.crc32c(e),) + orc.ascii_frame_packet(e, w, h) for e, (w, h) in zip(exp, dims)]

    def run():
        got, crc, hdr, pkt = emu.render_frames_crc(mode, frames, orc.PALETTE_STANDARD, variant, dims=dims)
        for k in range(len(frames)):
            assert got[k] == exp[k], ("frame", k)
            assert (crc[k], hdr[k], pkt[k]) == want[k], ("checksum, header, packet checksum of frame", k)
    run.keep = (imgs, frames)
    return f"fused CRC {MODE_NAMES[mode]} geometry {variant} dims {dims}", run


@pytest.mark.parametrize("variant", [20, 16, 17, 28, 25, 24])
def test_fused_crc(variant):
    """the frame's CRC computed while its bytes sit in LDS, blocks placed as they finish, the finishing wave writing header and
    packet CRC: checksums, headers and packet CRCs against orc.crc32c and orc's packet header"""
    imgs = [orc.frame_hash_noise(120, 90, i) for i in range(3)] + [run_frames(64, 48, "flat")]
    dims = [(80, 24), (60, 7), (33, 40), (100, 50)] if variant != 24 else [(440, 3), (80, 24), (60, 7), (300, 5)]
    modes = STREAM_MODES if variant in (20, 16, 17) else [MODE_MONO, MODE_HB_TRUE, MODE_HB_256]
    if variant == 16:
        modes = [MODE_TRUE_FG, MODE_256_FG]
    cases = [_crc_case(mode, imgs, dims, variant) for mode in modes]
    sweep(cases, variant, wait_paths=True)


def check_packed_all(res, expected, what, capacity):
    """what emu.py states for the PACK forms (exact lengths, 16-byte aligned starts, the pieces tile [0, total) in SOME order,
    error frames take no room, zero padding, the cursor re-armed) and: every frame's bytes the oracle's (check_packed compares
    them), nothing at or behind the total, nothing at or behind the capacity"""
    emu.check_packed(res, expected, what)
    total = int(res["off"][len(expected)])
    assert total == sum((len(e) + 15) // 16 * 16 for e in expected if not isinstance(e, int)), what
    assert (res["dst"][min(total, capacity):] == 0xEE).all(), (what, "bytes behind the packed frames or the capacity")


def _pack_frames(mode):
    imgs = [orc.frame_hash_noise(120, 90, 40 + i) for i in range(5)] + [TORTURE]
    dims = [(80, 24), (60, 7), (33, 40), (1, 50), (3, 2), (80, 24)]
    frames = [emu.frame_for_convert(im, w, h, 0) for im, (w, h) in zip(imgs, dims)]
    expected = [oracle_convert(im, mode, w, h, orc.PALETTE_STANDARD) for im, (w, h) in zip(imgs, dims)]
    return imgs, dims, frames, expected


def _pack_case(mode, variant, want_crc, stride=None):
    imgs, dims, frames, expected = _pack_frames(mode)
    if stride:  # a frame that does not fit its bound takes no room
        expected = [e if len(e) <= stride else 0xFFFFFFFF for e in expected]
    want = [(orc.crc32c(e),) + orc.ascii_frame_packet(e, w, h) for e, (w, h) in zip(expected, dims) if not isinstance(e, int)]

    def run():
        res = emu.render_frames_packed(mode, frames, orc.PALETTE_STANDARD, variant, dims=dims, want_crc=want_crc, stride=stride)
        check_packed_all(res, expected, "packed", len(frames) * res["stride"])
        if want_crc:
            got = [(int(res["crc"][k]), res["hdr"][24 * k:24 * k + 24].tobytes(), int(res["pkt"][k])) for k, e in enumerate(expected) if not isinstance(e, int)]
            assert got == want, "checksums, headers, packet checksums"
        return res
    run.keep = (imgs, frames)
    return f"PACK {MODE_NAMES[mode]} geometry {variant} crc {want_crc} stride {stride}", run


def _length_first_case(variant):
    """test_stream_kernel_length_first_exact_length_frames' frames: far beyond the 48 KB of the LDS-image form among them"""
    imgs = [TORTURE, orc.frame_hash_noise(1920, 54, 11), orc.frame_hash_noise(200, 60, 5), orc.frame_bars(64, 48, 3), orc.frame_smooth(33, 17)]
    dims = [(97, 31), (80, 24), (200, 60), (17, 9), (33, 40)]
    frames = [emu.frame_for_convert(im, w, h, 0, True, True) for im, (w, h) in zip(imgs, dims)]
    want = [oracle_convert(im, MODE_TRUE_FG, w, h, orc.PALETTE_STANDARD, True, True) for im, (w, h) in zip(imgs, dims)]
    assert max(len(w) for w in want) > 48 * 1024

    def run():
        cur = np.zeros(2, dtype=np.uint64)
        r = emu.render_frames_length_first(frames, orc.PALETTE_STANDARD, variant, cursor=cur)
        r["cursor"] = cur
        check_packed_all(r, want, "length first", len(frames) * r["stride"])
        return r
    run.keep = (imgs, frames)
    return f"length first geometry {variant}", run


@pytest.mark.parametrize("variant", [20, 16, 17])
def test_pack_and_length_first(variant):
    """the stream kernel's PACK form (the frame staged whole in LDS, its place claimed with one atomic add) with and without the
    fused CRC, and LENGTH-FIRST (frames beyond 48 KB: the lean loop twice, lengths first)"""
    cases = [_pack_case(mode, variant, want_crc) for mode in (MODE_TRUE_FG, MODE_256_FG, MODE_16_FG) for want_crc in (True, False)]
    cases.append(_pack_case(MODE_TRUE_FG, variant, True, stride=2048))
    cases.append(_length_first_case(variant))
    sweep(cases, variant, wait_paths=True)


# ---- the wire passes -----------------------------------------------------------------------------------------------------------
# crc_kernels.hpp: the frame kernel's workgroups are 1024 threads (waves 0, 1 and 15 held), the span kernels' 256 (every wave)
CRC_FRAME_SCHEDULES = wave_schedules(16, False)
CRC_SPAN_SCHEDULES = wave_schedules(4, True)


def _crc_run(b, **kw):
    import test_crc_boundaries as TB
    return lambda: TB._check(b, "", **kw)


@pytest.fixture(params=[0, 1], ids=["spans+finish", "one launch"])
def one_launch(request):
    emu.lib().emu_set_crc_one_launch(request.param)
    yield request.param
    emu.lib().emu_set_crc_one_launch(0)


def test_crc_frame_kernel():
    """crc_kernels.hpp crc32c_frame_kernel: frame tails at every length class of a workgroup (the thinned family) and the error /
    empty batches: wave partials combined through LDS behind barriers"""
    for b in (CC.frame_tails(2), CC.error_and_empty()[0]):
        under(emu.lib(), f"crc {b.name}", CRC_FRAME_SCHEDULES, _crc_run(b))


def test_crc_span_kernels(one_launch):
    """the span kernels with the small spans the families force, spans + finish and the one-launch form (the last span to arrive
    combines -- in ascending order always the highest-numbered one): every wave schedule, then other workgroup orders"""
    batches = list(CC.span_edges())[::2] + list(CC.span_batches())[:2]
    for b in batches:
        under(emu.lib(), f"crc {b.name} one_launch={one_launch}", CRC_SPAN_SCHEDULES, _crc_run(b))
    if one_launch:  # workgroups that do not wait for one another: the combiner is a different span each time, span 0 included
        for b in batches + [CC.wide_spans()]:
            under(emu.lib(), f"crc {b.name} one launch", WG_ORDERS + [Schedule.desc().workgroups("shuffle", 9)], _crc_run(b))


def test_crc_copy_forms_under_workgroup_orders(one_launch):
    """pack_frames_kernel's layout through the COPY forms: every workgroup recomputes the offsets from the lengths, so the places
    ARE frame order whatever the order of the workgroups (crc_ref.check_packed's premise, which therefore stays)"""
    import test_crc_boundaries as TB
    for b in CC.span_edges()[:3]:
        for _, cap in CC.pack_capacities(b):
            under(emu.lib(), f"crc copy {b.name} capacity {cap}", WG_ORDERS + [Schedule.desc()], lambda: TB._run_packed(b, cap))


# zpack.h ACHIP_ZPACK_BLOCK = 256 (the plan and close kernels); the measure / encode / build / place workgroups are up to 1024
# threads.  At the product's piece a run costs seconds: waves 0, 1 and the last, 3 seeds.  In the small-piece libraries it costs
# milliseconds: every wave of a four-wave workgroup and the last of a sixteen-wave one, 8 seeds.
WIRE_SCHEDULES = wave_schedules(16, False)
WIRE_SMALL_SCHEDULES = wave_schedules(16, True, held=(0, 1, 2, 3, 15))


def _wire(form_support, named, piece=None):
    frames = [f for _, f in named] if isinstance(named[0], tuple) else list(named)
    dims = ZS.dims_of(len(frames))
    kw = dict(piece=piece) if piece else {}

    def run():
        out, cap = form_support.emu_run(frames, dims, **kw)
        form_support.check(frames, dims, out, cap, "", **kw)
        assert (out["dst"][cap:] == ZW.FILL).all(), "a store at or behind dst + capacity"
    return run


WIRE_FAMILIES = ["zpack tails", "zpack tail gain and symbols", "zpack ratio and cuts", "zpack chunk steps", "zpack histograms",
                 "zpack batches", "zpack whole pieces", "zwide", "zseq", "zseq cuts"]


@pytest.mark.parametrize("family", WIRE_FAMILIES)
def test_wire_pass_histograms_and_streams(family):
    """zpack_kernels.hpp / zseq_kernels.hpp: histograms built with LDS atomics from several waves, streams cut over lanes and
    waves -- over the boundary families, with the small-piece libraries where the families use them.  The four kernels of a form
    are separate launches whose workgroups do not wait for one another: workgroup orders too"""
    small = ZC.SMALL_PIECE
    narrow, narrow_small = ZW.emulator(ZW.FORMS[0]), ZW.emulator(ZW.FORMS[0], small)
    sched = WIRE_SCHEDULES
    if family == "zpack tails":
        runs = [(narrow_small, _wire(ZS, fam(small), small), fam.__name__) for fam in (ZC.tail_lengths, ZC.tail_phases)]
        sched = WIRE_SMALL_SCHEDULES
    elif family == "zpack tail gain and symbols":
        runs = [(narrow_small, _wire(ZS, fam(small), small), fam.__name__) for fam in (ZC.tail_gain, ZC.tail_symbols)]
        sched = WIRE_SMALL_SCHEDULES
    elif family == "zpack ratio and cuts":
        runs = [(narrow, _wire(ZS, fam()), fam.__name__) for fam in (ZC.ratio_frames, ZC.stream_cut_frames)]
    elif family == "zpack chunk steps":
        runs = [(narrow, _wire(ZS, ZC.chunk_step_frames()), "chunk_step_frames"),
                (narrow, _wire(ZS, ZC.tail_lengths_long() + ZC.one_per_tail_kind()), "tails at the real piece size")]
    elif family == "zpack histograms":  # the measure kernel's LDS-atomic histograms: every histogram of the family
        runs = [(narrow, _wire(ZS, [(name, f) for name, _, f in ZC.histograms()]), "histograms")]
    elif family == "zpack batches":  # more frames than the plan kernel has threads
        runs = [(narrow, _wire(ZS, ZC.short_batch(257)), "short_batch(257)")]
    elif family == "zpack whole pieces":
        runs = [(narrow, _wire(ZS, ZC.piece_batch(Z.PIECE)), "piece_batch")]
    elif family == "zwide":
        runs = [(ZW.emulator(WS.FORM), _wire(WS, list(WS.wide_cases().values())), "wide cases")]
    elif family == "zseq":
        runs = [(ZW.emulator(SC.FORM), _wire(SC, list(SC.cases().values())), "zseq cases")]
    else:
        runs = [(ZW.emulator(SC.FORM, SC.SMALL), _wire(SC, list(SC.cases(SC.SMALL).values()), SC.SMALL), "zseq cuts")]
        sched = WIRE_SMALL_SCHEDULES
    for lib, run, name in runs:
        under(lib, f"{family}: {name}", sched + WG_ORDERS, run)


# ---- the rasteriser and the digital rain pass ----------------------------------------------------------------------------------
RASTER_WAVES = 4  # raster_kernels.hpp RASTER_BLOCK = 256


@pytest.mark.parametrize("name", ["chunk boundaries", "pen across rows", "overhang 3x3"])
def test_rasteriser(name):
    """raster_kernels.hpp: several resolve passes and LDS staging, ordered by barriers; one workgroup per frame and pass"""
    case = RAS.cases()[name]

    def run():
        pixels, start, pitch, status = RAS.emu_run(case)
        RAS.check(name, case, pixels, start, pitch, status)
    under(RAS.emulator(), f"raster {name}", wave_schedules(RASTER_WAVES, True, seeds=PRODUCT_SEEDS) + WG_ORDERS, run)


RAIN_WAVES = 4  # rain_kernels.hpp ACHIP_RAIN_BLOCK = 256


def test_digital_rain_chunk_boundaries():
    """rain_kernels.hpp at its chunk boundaries (rain_cases.chosen_boundary_cases: every kind of token at the 4096-byte chunk
    boundary, the long ones at the end of the staged look-ahead too) against the restatement, outputs and stored brightness"""
    import rain_cases as RC
    import rain_support as RNS
    import test_rain_boundaries as TR
    cs = RC.chosen_boundary_cases()

    def run():
        pairs = [TR._pair(c) for c in cs]
        try:
            TR._run_sequences(cs, pairs, tight=False)
        finally:
            TR._close(pairs)
    under(RNS.emulator(), "rain chunk boundaries", wave_schedules(RAIN_WAVES, True, seeds=PRODUCT_SEEDS) + WG_ORDERS, run)


# ---- launches whose workgroups do not wait for one another: workgroup orders ------------------------------------------------------
@pytest.mark.parametrize("variant", [20, 17])
def test_pack_and_length_first_under_workgroup_orders(variant):
    """the places now genuinely differ from frame order (asserted: at least one order puts a later frame in front of an earlier
    one), and everything emu.py states for these forms still holds"""
    for name, run in [_pack_case(MODE_TRUE_FG, variant, True), _pack_case(MODE_256_FG, variant, False),
                      _pack_case(MODE_TRUE_FG, variant, True, stride=2048), _length_first_case(variant)]:
        out_of_order = 0
        for s in WG_ORDERS + [Schedule.desc().workgroups("desc"), Schedule.random(4).workgroups("shuffle", 5)]:
            try:
                with scheduled(emu.lib(), s):
                    res = run()
            except AssertionError as e:
                raise AssertionError(f"case [{name}] under [{s}]: {e}") from None
            offs = [int(o) for o, ln in zip(res["off"], res["lens"]) if ln < 0xFFFFFFF0]
            out_of_order += offs != sorted(offs)
        assert out_of_order, (name, "no workgroup order moved a frame")


def test_one_workgroup_per_frame_launches_are_indifferent_to_the_order():
    """render (frame, stream and rows kernels, a ragged batch each) and raster: bytes independent of the order (box and yuv: below)"""
    imgs = [orc.frame_hash_noise(120, 90, i) for i in range(5)] + [orc.frame_bars(64, 48, 3), orc.frame_smooth(33, 17)]
    dims = [(80, 24), (60, 7), (33, 40), (80, 1), (1, 50), (17, 9), (128, 2)]
    for mode, variant in ((MODE_TRUE_FG, 2), (MODE_HB_TRUE, 3), (MODE_TRUE_FG, 20), (MODE_256_FG, 17), (MODE_MONO, 28), (MODE_HB_TRUE, 25), (MODE_HB_256, 30)):
        rm = MODE_CAPS.get(mode, (3, 0))[1]
        frames = [emu.frame_for_convert(im, w, h, rm) for im, (w, h) in zip(imgs, dims)]
        exp = [oracle_convert(im, mode, w, h, orc.PALETTE_STANDARD) for im, (w, h) in zip(imgs, dims)]

        def run():
            assert render(mode, frames, orc.PALETTE_STANDARD, variant) == exp
        under(emu.lib(), f"ragged batch {MODE_NAMES[mode]} geometry {variant}", WG_ORDERS, run)
    for name in ("batch of 40", "flags"):
        case = RAS.cases()[name]

        def run():
            pixels, start, pitch, status = RAS.emu_run(case)
            RAS.check(name, case, pixels, start, pitch, status)
        under(RAS.emulator(), f"raster {name}", WG_ORDERS, run)


ANY_ORDER = WG_ORDERS + [Schedule.desc(), Schedule.random(3).workgroups("shuffle", 7)]


def test_box_launches_are_indifferent_to_the_order():
    """box_kernels.hpp through box_support's cases, one frame a launch and five geometries in one launch (test_box_emulated's),
    against box_ref: workgroup orders, and DESC / RANDOM waves beside them"""
    import box_ref as BR
    import box_support as BS
    for name, case in BS.cases().items():
        img, ow, oh, stride, off, fl = case
        h, w = img.shape[:2]
        buf, start, _ = BS.place(img, stride, off)
        f = BS.frame_for(buf.ctypes.data + start, w, h, ow, oh, stride, fl)
        exp = BS.expected(name, case)

        def run():
            images, pitch, _ = BS.emu_run([f])
            BS.check_images(images, pitch, [f], [exp], name)
        under(BS.emulator(), f"box {name}", ANY_ORDER, run)
    shapes = [(48, 9, 16, 3, 0, 0, 0), (33, 7, 5, 2, 99, 3, BS.FLIP_X), (4, 4, 7, 3, 0, 0, BS.FLIP_Y), (130, 20, 9, 5, 400, 0, 0),
              (64, 300, 2, 1, 0, 0, 3)]
    frames, keep, exps = [], [], []
    for k, (w, h, ow, oh, stride, off, fl) in enumerate(shapes):
        img = BS.noise(w, h, 100 + k) if k != 4 else np.full((h, w, 3), 255, dtype=np.uint8)
        buf, start, _ = BS.place(img, stride, off)
        keep.append(buf)
        frames.append(BS.frame_for(buf.ctypes.data + start, w, h, ow, oh, stride, fl))
        exps.append(BR.box_ref(img, ow, oh, bool(fl & BS.FLIP_X), bool(fl & BS.FLIP_Y)))

    def run_mixed():
        images, pitch, _ = BS.emu_run(frames)
        BS.check_images(images, pitch, frames, exps, "mixed")
    under(BS.emulator(), "box five geometries in one launch", ANY_ORDER, run_mixed)


def test_yuv_launches_are_indifferent_to_the_order():
    """yuv_kernels.hpp through yuv_support's cases: the sampled pass (every case of test_sampled_pass_matches_the_restatement) and
    the whole conversions of every format, against yuv_ref, images and guard bytes as yuv_support checks them"""
    import yuv_ref as YR
    import yuv_support as YS
    for name, case in YS.sample_cases().items():
        def run():
            buf, start, pitch = YS.emu_run(case)
            YS.check_images(name, case, buf, start, pitch)
        under(YS.emulator(), f"yuv sampled {name}", ANY_ORDER, run)
    whole = YS.whole_cases()
    for fmt in YS.FORMATS:
        for name, case in whole[fmt].items():
            def run():
                buf, start = YS.emu_convert(case)
                YS.check_whole(f"{YR.NAMES[fmt]} {name}", case.src, buf, start, case.row_stride())
            under(YS.emulator(), f"yuv whole {YR.NAMES[fmt]} {name}", ANY_ORDER, run)


# ---- launches whose workgroups DO wait for one another ---------------------------------------------------------------------------
# Split frames (part_publish / part_wait) and the PARTS geometries 18 and 31-34 stay on ascending workgroup order for the byte
# checks above: the emulator runs workgroups one at a time to completion, so a part that runs before its predecessor can only
# wait out its bounded polls.  What it does then is the contract next to ACHIP_PART_POISON:
def test_a_part_that_runs_before_its_predecessor_gives_up_cleanly():
    """test_split_ragged_batch_and_policy's batch in five-row bands under workgroup order DESC: every part of a split frame
    runs before its predecessors, waits its bounded 2^21 polls and gives up -- the frame's length comes back as an error code,
    no byte is stored outside the frame's slot, and the frame of ONE band in the same launch is the oracle's.
    The poison propagates in effect, not as a published word: a part publishes its own byte count BEFORE it waits, but every part
    waits for ALL of its predecessors (render_kernels.hpp, "add up the predecessors'"), so a successor of a part that gave up
    gives up on the same missing predecessor, emits nothing, and the last part reports the error -- what the lengths below show"""
    imgs = [orc.frame_hash_noise(120, 90, i) for i in range(4)]
    dims = [(80, 24), (60, 7), (33, 40), (80, 1)]
    frames = [emu.frame_for_convert(im, w, h, 0) for im, (w, h) in zip(imgs, dims)]
    exp = [oracle_convert(im, MODE_TRUE_FG, w, h, orc.PALETTE_STANDARD) for im, (w, h) in zip(imgs, dims)]
    with scheduled(emu.lib(), DEFAULT) as r:
        assert render(MODE_TRUE_FG, frames, orc.PALETTE_STANDARD, 2, rows_per_part=5) == exp
    assert r.naps == 0, "in launch order no part waits"
    with scheduled(emu.lib(), Schedule().workgroups("desc")) as r:
        got = render(MODE_TRUE_FG, frames, orc.PALETTE_STANDARD, 2, rows_per_part=5)  # (checks the guard bytes round every slot)
    assert all(isinstance(g, int) and g >= 0xFFFFFFF0 for g in got[:3]), [g if isinstance(g, int) else len(g) for g in got]
    assert got[3] == exp[3]
    assert r.naps >= 1 << 21, "the parts polled to their bound"
