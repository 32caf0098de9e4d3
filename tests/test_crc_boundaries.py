"""The stand-alone checksum wire pass at its group, round and span boundaries without a GPU: every family of crc_cases.py
through crc32c_frame_kernel / crc32c_span_kernel / crc32c_finish_kernel / crc_packets_kernel under the CPU emulator, with the
span geometry the product's launcher chooses for the family forced (emu_crc32c's own choice restates an older launcher),
against the bitwise oracle (crc_ref.py): every element of every output array, in both one-launch settings where there are
spans.  The reference's own GF(2) restatement is checked against the oracle on real frames first.

The emulator's DPP reductions, readlane, agent-scope atomics and LDS table images are C++ stand-ins: only test_gpu_crc.py
checks the real ones.  What this run leaves out is named in crc_cases.EMU_LEFT_OUT."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import crc_cases as CC  # noqa: E402
import crc_ref as R  # noqa: E402
import emu  # noqa: E402
import orc  # noqa: E402


# ---- the reference's restatement, before it serves as one --------------------------------------------------------------------
def test_packet_crc_restatement_against_the_oracle_on_real_frames():
    rng = np.random.default_rng(7)
    for n in (0, 1, 13, 65535, 65536, (1 << 24) - 1, 1 << 24, (1 << 24) + 17):
        for f in (bytes(n), rng.integers(0, 256, n, dtype=np.uint8).tobytes()):
            for w, h in ((80, 24), (0xFFFFFFFF, 0)):
                assert R.packet_crc_from_frame_crc(w, h, n, orc.crc32c(f)) == orc.ascii_frame_packet(f, w, h), (n, w, h)
    for code in CC.ERR:
        assert R.packet_crc_from_frame_crc(80, 24, code, 0x12345678) == (bytes(24), 0)


def test_families_assert_their_premises():
    """building a family runs its asserts; the counts are the issue's"""
    assert CC.frame_tails().n == 207 and CC.frame_tails(2).n == 49 + 70
    assert len(CC.error_and_empty()) == 4 and CC.long_frames().n == 12
    assert len(CC.span_edges()) == 11 and {b.n for b in CC.span_edges()} == {3}
    assert [b.parts for b in CC.span_batches()] == [63, 64, 65, 128, 128, 128, 129, 129]
    assert CC.wide_spans().n == 65 and [b.parts for b in CC.len_bits()] == [1029, 258]
    assert [c[0] for c in CC.packets_only()] == [1, 256, 257, 600]


def test_the_product_launcher_takes_the_path_each_family_is_named_for():
    """achip_crc_parts is host arithmetic: the product library answers without a GPU"""
    if os.environ.get("ASCIICHAT_HIP_CRC_FRAME_MAX") or os.environ.get("ASCIICHAT_HIP_CRC_SMALL_SPANS"):
        pytest.skip("the diagnostic override is set")
    from __graft_entry__ import load_package
    p = load_package()
    p.build()
    L = p.lib()
    L.achip_crc_parts.restype = C.c_int
    L.achip_crc_parts.argtypes = [C.c_uint32, C.c_int]
    for b in _all_batches() + list(CC.pack_batches()):
        assert L.achip_crc_parts(b.max_len, b.n) == b.parts, b


def _all_batches():
    return ([CC.frame_tails(), CC.frame_content()] + list(CC.error_and_empty()) + [CC.long_frames()] + list(CC.span_edges()) +
            list(CC.span_batches()) + [CC.wide_spans()] + list(CC.len_bits()))


# ---- the kernels under the emulator ------------------------------------------------------------------------------------------
def _aligned(a):
    """a 16-byte aligned copy, as device allocations are -> (keep-alive, address, view)"""
    raw = np.empty(a.size + 16, dtype=np.uint8)
    at = -raw.ctypes.data % 16
    raw[at:at + a.size] = a
    return raw, raw.ctypes.data + at, raw[at:at + a.size]


def _run(b, slack_seed=0, with_dims=True, headers=True, fixed=None):
    """one emulated call over batch b with the product's geometry forced -> (crc, hdr | None, pkt | None)"""
    L = emu.lib()
    keep, base, _ = _aligned(b.slab(slack_seed))
    ln, d = b.len_words(), b.dim_words()
    crc = np.full(b.n, R.SENTINEL_WORD, dtype=np.uint32)
    hdr = np.full(24 * b.n, R.SENTINEL_BYTE, dtype=np.uint8)
    pkt = np.full(b.n, R.SENTINEL_WORD, dtype=np.uint32)
    L.emu_crc32c(base, b.stride, None if fixed is not None else ln.ctypes.data, fixed or 0, b.max_len, b.n, b.parts, b.rounds,
                 d.ctypes.data if with_dims else None, crc.ctypes.data, hdr.ctypes.data if headers else None,
                 pkt.ctypes.data if headers else None)
    del keep
    return (crc, hdr, pkt) if headers else (crc, None, None)


def _check(b, what, **kw):
    crc, hdr, pkt = _run(b, **kw)
    R.check_outputs(b.expect(), b.lens, crc, hdr, pkt, with_dims=kw.get("with_dims", True), what=f"{b.name} {what}")
    return crc, hdr, pkt


@pytest.fixture(params=[0, 1], ids=["spans+finish", "one launch"])
def one_launch(request):
    emu.lib().emu_set_crc_one_launch(request.param)
    yield request.param
    emu.lib().emu_set_crc_one_launch(0)


def test_frame_tails():
    """(a) and slack independence: the same outputs with the slack bytes regenerated"""
    b = CC.frame_tails()
    first = _check(b, "")
    again = _check(b, "slack regenerated", slack_seed=1)
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    _check(b, "CRC only", headers=False)


def test_frame_content():
    b = CC.frame_content()
    _check(b, "")
    _check(b, "no dims", with_dims=False)


@pytest.mark.parametrize("k", range(4))
def test_error_and_empty(k):
    b = CC.error_and_empty()[k]
    _check(b, "")
    _check(b, "no dims", with_dims=False)
    _check(b, "CRC only", headers=False)


def test_long_frames_in_one_workgroup():
    _check(CC.long_frames(), "")


def _fixed_expect(b, fixed, slack_seed=0):
    s = b.slab(slack_seed)
    return np.array([orc.crc32c(s[i * b.stride:i * b.stride + fixed].tobytes()) for i in range(b.n)], dtype=np.uint32)


def test_a_fixed_length_without_length_words(one_launch):
    """len == NULL on each path: every slot's first fixed_len bytes, slack and all"""
    for b, fixed in ((CC.error_and_empty()[0], 19999), (CC.long_frames(), 196601), (CC.span_edges()[0], 180229),
                     (CC.wide_spans(), 65537)):
        crc, _, _ = _run(b, headers=False, fixed=fixed)
        assert np.array_equal(crc, _fixed_expect(b, fixed)), (b, fixed)


def test_span_edges(one_launch):
    for b in CC.span_edges():
        _check(b, "")
    b = CC.span_edges()[5]
    first = _check(b, "again")
    again = _check(b, "slack regenerated", slack_seed=1)
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    _check(b, "no dims", with_dims=False)
    _check(b, "CRC only", headers=False)


def test_span_batches(one_launch):
    for b in CC.span_batches():
        _check(b, "")


def test_wide_spans(one_launch):
    _check(CC.wide_spans(), "")


def test_len_bits(one_launch):
    for b in CC.len_bits():
        _check(b, "")


def test_one_launch_leaves_its_counters_at_zero_and_runs_again_on_them():
    """the caller's arrival counters (a plan's): zero after the launch, and a second launch on them with other data is right"""
    L = emu.lib()
    L.emu_set_crc_counters.restype = None
    L.emu_set_crc_counters.argtypes = [C.c_void_p]
    L.emu_set_crc_one_launch(1)
    try:
        e, f, g = CC.span_edges(), CC.span_batches(), CC.span_batches_swapped()
        for first, second in ((e[5], e[9]), (f[0], g[0]), (f[1], g[1]), (f[3], f[4])):
            counters = np.zeros(first.n, dtype=np.uint32)
            assert first.n == second.n and first.parts == second.parts
            L.emu_set_crc_counters(counters.ctypes.data)
            _check(first, "first launch")
            assert not counters.any(), (first, counters)
            _check(second, "second launch", slack_seed=3)
            assert not counters.any(), (second, counters)
    finally:
        L.emu_set_crc_counters(None)
        L.emu_set_crc_one_launch(0)


# ---- (i) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CC.packets_only(), ids=lambda c: f"n={c[0]}")
def test_packets_from_known_checksums(case):
    """crc_packets_kernel through the mock launcher: headers byte for byte, packet CRCs against the GF(2) restatement"""
    import mockgpu
    L = mockgpu.package().lib()
    n, lens, crcs, dims = case
    want_hdr, want_pkt = CC.packets_expect(case)
    for d in (dims, None):
        hdr = np.full(24 * n, R.SENTINEL_BYTE, dtype=np.uint8)
        pkt = np.full(n, R.SENTINEL_WORD, dtype=np.uint32)
        assert L.asciichat_hip_packets_from_crc(lens.ctypes.data, crcs.ctypes.data, n, d.ctypes.data if d is not None else None,
                                                hdr.ctypes.data, pkt.ctypes.data, None) == 0
        if d is None:
            want_hdr, want_pkt = CC.packets_expect((n, lens, crcs, np.zeros_like(dims)))
        assert np.array_equal(hdr, want_hdr) and np.array_equal(pkt, want_pkt), (n, np.flatnonzero(pkt != want_pkt)[:4])


# ---- (j) ---------------------------------------------------------------------------------------------------------------------
def _run_packed(b, cap):
    L = emu.lib()
    L.emu_crc32c_pack.restype = None
    L.emu_crc32c_pack.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    slab = b.slab()
    keep, base, _ = _aligned(slab)
    total = b.packed()[0][b.n]
    keep2, dbase, dst = _aligned(np.full(total + 64, R.SENTINEL_BYTE, dtype=np.uint8))
    ln, d = b.len_words(), b.dim_words()
    crc = np.full(b.n, R.SENTINEL_WORD, dtype=np.uint32)
    hdr = np.full(24 * b.n, R.SENTINEL_BYTE, dtype=np.uint8)
    pkt = np.full(b.n, R.SENTINEL_WORD, dtype=np.uint32)
    off = np.full(b.n + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    lo = np.full(b.n, R.SENTINEL_WORD, dtype=np.uint32)
    L.emu_crc32c_pack(base, b.stride, ln.ctypes.data, b.max_len, b.n, b.parts, b.rounds, d.ctypes.data, crc.ctypes.data,
                      hdr.ctypes.data, pkt.ctypes.data, dbase, cap, off.ctypes.data, lo.ctypes.data)
    what = f"{b.name} packed, capacity {cap}"
    R.check_outputs(b.expect(), b.lens, crc, hdr, pkt, what=what)
    R.check_packed(slab, b.stride, b.lens, cap, off, lo, dst, what=what)
    del keep, keep2


def test_pack_edges_in_one_workgroup():
    for b in (CC.frame_tails(2),) + CC.error_and_empty():
        for _, cap in CC.pack_capacities(b):
            _run_packed(b, cap)


def test_pack_edges_in_spans(one_launch):
    for b in CC.span_edges():
        for _, cap in CC.pack_capacities(b):
            _run_packed(b, cap)


def test_pack_offsets_of_more_frames_than_threads():
    """the capacity 'total' alone: the other three are named in crc_cases.EMU_LEFT_OUT"""
    b = CC.short_pack_batch()
    assert len(CC.EMU_LEFT_OUT) == 1 and "1100" in CC.EMU_LEFT_OUT[0][0]
    (name, cap), = [c for c in CC.pack_capacities(b) if c[0] == "total"]
    _run_packed(b, cap)
