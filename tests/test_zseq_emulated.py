"""The zseq wire form without a GPU: the build and place kernels (and the zhuf pass's plan and close kernels at this form's
piece size) under the CPU emulator against the restatement (tests/zseq_ref.py) and the oracle's CRC -- destination, offsets,
sent lengths, headers, checksums and packet checksums byte for byte, nothing stored outside the frames -- at the product's
piece size and, from a second library built with ACHIP_ZSEQ_PIECE=512, over frames of many blocks; the kernels' constant
tables; and what the product library decides before it needs a device."""
import pytest

import zhuf_ref as Z
import zpack_support as ZS
import zseq_cases as SC
import zseq_ref as S
import zwide_support as WS
import zwire as ZW

CASES = SC.cases()
CUTS = SC.cases(SC.SMALL)
SMALL = SC.SMALL


def test_mixed_batch_equals_the_restatement():
    frames = list(CASES.values())
    dims = ZS.dims_of(len(frames))
    out, cap = SC.emu_run(frames, dims)
    SC.check(frames, dims, out, cap, "mixed")


def test_block_cut_batch_at_a_small_piece_equals_the_restatement():
    frames = list(CUTS.values())
    dims = ZS.dims_of(len(frames))
    out, cap = SC.emu_run(frames, dims, piece=SMALL)
    SC.check(frames, dims, out, cap, "cuts", piece=SMALL)


def test_the_kernels_tables_are_the_restatements():
    """stateTable, deltaNbBits, deltaFindState of the three predefined distributions; baselines and extra bits of the codes"""
    w = SC.emulator().emu_zseq_tables()
    words = [w[k] for k in range(512)]
    (ll, ml, of) = S.device_tables()
    assert words[0:64] == ll[0] and words[64:128] == ml[0] and words[128:160] == of[0]
    for at, t in ((0, ll), (36, ml), (89, of)):
        assert words[160 + at:160 + at + len(t[1])] == t[1]
        assert [x - (1 << 32) if x >> 31 else x for x in words[288 + at:288 + at + len(t[2])]] == t[2]
    assert words[416:452] == [b | (x << 24) for b, x in zip(S.LL_BASE, S.LL_BITS)]
    assert words[452:505] == [b | (x << 24) for b, x in zip(S.ML_BASE, S.ML_BITS)]


def _piece_frames():
    """frames of 3 to 9 blocks of 512 bytes: text, half blocks, a multi-byte palette, an RLE and a raw block among them"""
    a = SC.text(3 * SMALL + 77, 70)
    b = WS.halfblock_truecolor(20, 6, 71)[:4 * SMALL + 511]
    c = SC.text(SMALL, 72) + b"\xe2" * SMALL + SC.rnd(SMALL, 73) + SC.text(300, 74)
    d = WS.utf8_truecolor(20, 6, 75)
    return [a, b, SC.ERR, c, d, b"", SC.text(2 * SMALL + 3, 76)]


def test_frames_of_many_blocks():
    frames = _piece_frames()
    assert [i["kind"] for i in SC.infos_of(frames[3], SMALL)] == [2, 1, 0, 2]
    assert all(S.wire(f, SMALL)[2] == Z.FLAG_COMPRESSED for f in frames if not isinstance(f, int) and f)
    dims = ZS.dims_of(len(frames))
    out, cap = SC.emu_run(frames, dims, piece=SMALL)
    SC.check(frames, dims, out, cap, "pieces", piece=SMALL)


def test_a_stride_wider_than_the_longest_frame():
    frames = _piece_frames()
    dims = ZS.dims_of(len(frames))
    out, cap = SC.emu_run(frames, dims, piece=SMALL, stride=8 * SMALL + 48)
    SC.check(frames, dims, out, cap, "wide stride", piece=SMALL)


@pytest.mark.parametrize("short", [1, 16, 17, 700])
def test_tight_capacity(short):
    frames = [CASES[k] for k in ("127 sequences", "error code", "one byte value (RLE)", "1024 bytes (as it is: the size floor)",
                                 "half-block truecolor 20x6", "empty")]
    dims = ZS.dims_of(len(frames))
    _, total = SC.expect(frames, dims)
    out, cap = SC.emu_run(frames, dims, capacity=total - short)
    SC.check(frames, dims, out, cap, f"capacity -{short}")
    assert (out["dst"][cap:] == ZS.FILL).all()


def test_capacities_that_end_inside_a_block():
    frames = _piece_frames()
    dims = ZS.dims_of(len(frames))
    exp, total = SC.expect(frames, dims, SMALL)
    at = Z.blocks(exp[0]["payload"])
    for cap in (exp[0]["off"] + at[1][2] + 40, exp[0]["off"] + at[2][2] + 3, exp[3]["off"] + 100, total - 1):
        out, cap = SC.emu_run(frames, dims, capacity=cap, piece=SMALL)
        SC.check(frames, dims, out, cap, f"capacity {cap}", piece=SMALL)
        assert (out["dst"][cap:] == ZS.FILL).all()


def test_more_frames_than_threads_of_the_plan():
    """257 small frames (the plan kernel walks more than one per thread): error codes, empty frames, frames below the size
    floor whose blocks still compress, and a coded frame every seventh"""
    pool = [CASES["a match at position 6 of the frame"], SC.ERR, b"abcdabcd" * 40, b"", CASES["5 bytes"], SC.rnd(100, 9), b"\xe2" * 300]
    frames = [pool[i % len(pool)] for i in range(257)]
    dims = ZS.dims_of(257)
    out, cap = SC.emu_run(frames, dims)
    SC.check(frames, dims, out, cap, "257 frames")


def test_library_refuses_before_it_needs_a_device_and_needs_one_after():
    ZW.check_refusals(ZW.SEQ)
