"""The wide zhuf form without a GPU: the wide instantiations of the four kernels under the CPU emulator against the
restatement (tests/zwide_ref.py) and the oracle's CRC -- destination, offsets, sent lengths, headers, checksums and packet
checksums byte for byte, nothing stored outside the frames, the tables and trees in the scratch records -- and what the
product library decides before it needs a device."""
import numpy as np
import pytest

import zhuf_ref as Z
import zpack_support as ZS
import zwide_ref as W
import zwide_support as WS
import zwire as ZW

CASES = WS.wide_cases()
SMALL = 2048  # the second emulator library's ACHIP_ZPACK_PIECE


@pytest.fixture(scope="module")
def mixed():
    frames = list(CASES.values())
    dims = ZS.dims_of(len(frames))
    out, cap = WS.emu_run(frames, dims)
    return frames, dims, out, cap


def test_mixed_batch_equals_the_restatement(mixed):
    frames, dims, out, cap = mixed
    WS.check(frames, dims, out, cap, "mixed")


def test_tables_and_trees_in_the_scratch_records(mixed):
    frames, _, out, _ = mixed
    assert WS.check_records(frames, out) >= 20


def test_the_batch_takes_every_path():
    """frames sent as they are and as zhuf frames; RLE, raw and Huffman blocks; both forms of the tree"""
    kinds, forms = set(), set()
    for name, f in CASES.items():
        if isinstance(f, int):
            continue
        _, _, flags = WS.wire_of(f)
        kinds.add(("zhuf" if flags else "as is", (W.encode(f)[9] >> 1) & 3))
        forms.add(WS.info_of(f).get("form") if flags else None)
    assert {("zhuf", 1), ("zhuf", 2), ("as is", 0), ("as is", 2)} <= kinds and {"direct", "fse"} <= forms


def test_frames_without_a_byte_above_0x80_come_out_as_the_narrow_form():
    """zpack_support.small_cases() through the wide kernels: checked against the NARROW restatement wherever no byte is above
    0x80, and equal to what the narrow kernels store"""
    cases = ZS.small_cases()
    frames = [f for f in cases.values() if isinstance(f, int) or not f or max(f) <= 0x80]
    assert len(frames) == len(cases) - 1
    dims = ZS.dims_of(len(frames))
    wide, cap = WS.emu_run(frames, dims)
    ZS.check(frames, dims, wide, cap, "narrow cases, wide kernels")
    narrow, _ = ZS.emu_run(frames, dims)
    for k in ("dst", "off", "len_out", "crc", "hdr", "pkt"):
        assert np.array_equal(wide[k], narrow[k]), k


@pytest.mark.parametrize("short", [1, 16, 17, 700])
def test_tight_capacity(short):
    frames = [CASES[k] for k in ("top 129 (odd count of weights)", "error code", "one byte value above 0x80 (RLE)",
                                 "half blocks below the size floor (as it is)", "half-block truecolor 20x6", "empty")]
    dims = ZS.dims_of(len(frames))
    _, total = WS.expect(frames, dims)
    out, cap = WS.emu_run(frames, dims, capacity=total - short)
    WS.check(frames, dims, out, cap, f"capacity -{short}")
    assert (out["dst"][cap:] == ZS.FILL).all()


def _piece_frames():
    """frames of 2 and 3 pieces of 2048 bytes with bytes above 0x80: Huffman blocks with FSE trees at several phases, a
    1023-byte second piece (Size_Format 1 with an FSE tree), a raw and an RLE piece among them"""
    a = WS.skewed_high(2 * SMALL + 700, 50, top=0xE2, symbols=40)
    b = WS.skewed_high(SMALL, 51, top=0x9F, symbols=25) + WS.skewed_high(1023, 90, top=0xE2, symbols=30)
    c = WS.skewed_high(SMALL + 5, 52, top=0xFF, symbols=90)[:SMALL] + b"\xe2" * SMALL + WS.skewed_high(333, 53, top=0x81, symbols=9)
    d = WS.skewed_high(SMALL, 54, top=0xC3, symbols=12) + bytes(np.random.default_rng(55).integers(0, 256, 900, dtype=np.uint8))
    e = WS.halfblock_truecolor(20, 6, 56)
    return [a, b, WS.ERR, c, d, b"", e]


def test_frames_of_two_and_three_pieces():
    frames = _piece_frames()
    for f, blocks in ((frames[0], [2, 2, 2]), (frames[1], [2, 2]), (frames[3], [2, 1, 2]), (frames[4], [2, 0])):
        assert [k for k, _, _ in Z.blocks(W.encode(f, piece=SMALL))] == blocks and WS.wire_of(f, SMALL)[2] == Z.FLAG_COMPRESSED
    body = W.huf_block_body(frames[1][SMALL:])
    assert (body[0] >> 2) & 3 == 1 and body[3] < 128  # Size_Format 1, an FSE tree
    dims = ZS.dims_of(len(frames))
    out, cap = WS.emu_run(frames, dims, piece=SMALL)
    WS.check(frames, dims, out, cap, "pieces", piece=SMALL)
    assert WS.check_records(frames, out, piece=SMALL) >= 10


def test_capacities_that_end_inside_a_block():
    frames = _piece_frames()
    dims = ZS.dims_of(len(frames))
    exp, total = WS.expect(frames, dims, SMALL)
    at = Z.blocks(exp[0]["payload"])
    for cap in (exp[0]["off"] + at[1][2] + 40, exp[0]["off"] + at[2][2] + 3, exp[3]["off"] + 100, total - 1):
        out, cap = WS.emu_run(frames, dims, capacity=cap, piece=SMALL)
        WS.check(frames, dims, out, cap, f"capacity {cap}", piece=SMALL)
        assert (out["dst"][cap:] == ZS.FILL).all()


def test_library_refuses_before_it_needs_a_device_and_needs_one_after():
    ZW.check_refusals(ZW.WIDE)
