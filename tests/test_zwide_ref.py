"""The wide zhuf form as tests/zwide_ref.py restates it: every case goes encode -> decode (the subset decoder,
its FSE part written from the format) and encode -> libzstd's ZSTD_decompress, and must give back the original bytes; every
family asserts with the restatement that it is the case it claims to be."""
import numpy as np
import pytest

import zhuf_ref as Z
import zpack_support as ZS
import zwide_ref as W
import zwide_support as WS

CASES = WS.wide_cases()


def test_libzstd_is_the_judge_here():
    assert Z.libzstd() is not None


@pytest.mark.parametrize("name", [k for k, v in CASES.items() if not isinstance(v, int)])
def test_every_case_round_trips(name):
    f = CASES[name]
    z = W.roundtrip(f)
    payload, csz, flags = W.wire(f)
    if "raw" in name or "as it is" in name or len(f) <= 1024:
        assert (payload, csz, flags) == (f, 0, 0), name
    else:
        assert (payload, csz, flags) == (z, len(z), Z.FLAG_COMPRESSED) and 5 * len(z) < 4 * len(f), name


@pytest.mark.parametrize("top,form", [(128, "direct"), (129, "fse"), (130, "fse"), (254, "fse"), (255, "fse")])
def test_largest_symbols(top, form):
    """128 weights go in the direct form as before; 129 is the first FSE tree; odd and even counts of weights start the
    two states in either order"""
    f = next(v for k, v in CASES.items() if k.startswith("top %d" % top))
    info = WS.info_of(f)
    assert max(f) == top and info["form"] == form and info["coded"]
    if form == "direct":
        assert W.encode(f) == Z.encode(f)
    else:
        body = W.huf_block_body(f)
        hl = 2 + ((body[0] >> 2) & 3)
        assert 2 <= body[hl] <= 127  # the header byte: the FSE form's byte count


def test_two_symbols_all_symbols_and_the_raw_ones():
    t = []
    f = CASES["two symbols, one above 0x80"]
    z = W.encode(f, t)
    assert sorted(d for d in t[0] if d) == [1, 1] and Z.blocks(z)[0][0] == 2 and WS.info_of(f)["form"] == "fse"
    t = []
    f = CASES["all 256 symbols skewed"]
    z = W.encode(f, t)
    assert all(d > 0 for d in t[0]) and Z.blocks(z)[0][0] == 2
    f = CASES["256 equal counts (raw)"]
    lens = W.code_lengths([f.count(bytes([s])) for s in range(256)])
    assert lens == [8] * 256 and W.fse_tree([1] * 255) is None  # one weight value: the guard
    assert Z.blocks(W.encode(f)) == [(0, len(f), 9)]
    f = CASES["uniform bytes (raw by size)"]
    assert W.huf_block_candidate(f) is not None and W.huf_block_body(f) is None and Z.blocks(W.encode(f)) == [(0, len(f), 9)]
    f = CASES["one byte value above 0x80 (RLE)"]
    assert Z.blocks(W.encode(f)) == [(1, len(f), 9)]


def test_normalisation_takes_both_branches():
    dec, add = WS.info_of(CASES["normalisation decrements"]), WS.info_of(CASES["normalisation adds"])
    assert dec["dec"] > 0 and dec["form"] == "fse" and dec["coded"]
    assert add["add"] > 0 and add["dec"] == 0 and add["form"] == "fse" and add["coded"]


@pytest.mark.parametrize("z", [0, 1, 2, 3, 4, 6])
def test_zero_runs_in_the_description(z):
    """z absent weight values in one run: none at all, then 2-bit counts 0, 1, 2, a "11" flag + 0, and a flag + 2"""
    info = WS.info_of(CASES["zero run of %d weight values" % z])
    assert info["form"] == "fse" and info["coded"]
    assert info["runs"] == ([] if z == 0 else [z - 1])


@pytest.mark.parametrize("residue", [0, 7])
def test_bitstream_ends_on_and_before_a_byte(residue):
    info = WS.info_of(CASES["bitstream of %d bits mod 8" % residue])
    assert info["bits"] % 8 == residue and info["coded"]


@pytest.mark.parametrize("csize", [1023, 1024])
def test_literals_sections_of_1023_and_1024_bytes(csize):
    """a block that gains over a piece with 1023 bytes of literals section has at least 1024 literals, so both carry
    Size_Format 2; Size_Format 1 with an FSE tree is the 1023-byte piece below, which no frame sends as a block of its own
    at the product's piece size (the emulated tests send it as a second piece)"""
    f = CASES["csize %d" % csize]
    body = W.huf_block_body(f)
    assert body is not None and max(f) > 0x80 and WS.csize_of(body) == csize and (body[0] >> 2) & 3 == 2
    short = WS.skewed_high(1023, 90, top=0xE2, symbols=30)
    body = W.huf_block_body(short)
    assert body is not None and (body[0] >> 2) & 3 == 1 and WS.csize_of(body) < 1023
    W.roundtrip(short)


def test_half_blocks():
    f = CASES["half blocks below the size floor (as it is)"]
    assert len(f) <= 1024 and W.wire(f) == (f, 0, 0) and Z.blocks(W.encode(f))[0][0] == 2  # coded, yet sent as it is
    for name in ("half-block truecolor 20x6", "utf-8 palette truecolor 20x6"):
        f = CASES[name]
        assert max(f) > 0x80 and Z.wire(f) == (f, 0, 0)  # the narrow form sends it as it is
        payload, csz, flags = W.wire(f)
        assert flags == Z.FLAG_COMPRESSED and 5 * csz < 4 * len(f)


def test_frames_without_a_byte_above_0x80_are_the_narrow_form():
    for name, f in ZS.small_cases().items():
        if isinstance(f, int) or (f and max(f) > 0x80):
            continue
        assert W.encode(f) == Z.encode(f) and W.wire(f) == Z.wire(f), name
    f = ZS.small_cases()["0x81 present (raw)"]
    assert Z.blocks(Z.encode(f))[0][0] == 0 and Z.blocks(W.encode(f))[0][0] == 2


def test_the_decoder_refuses_what_is_outside_the_subset():
    body = W.huf_block_body(CASES["top 255"])
    z = W.encode(CASES["top 255"])
    at = z.index(body)
    hl = 2 + ((body[0] >> 2) & 3)
    bad = bytearray(z)
    bad[at + hl + 1] = (bad[at + hl + 1] & 0xF0) | 2  # Accuracy_Log 7
    with pytest.raises(Z.FormatError):
        W.decode(bytes(bad))
    with pytest.raises(Z.FormatError):
        W.decode(z[:-1])


def test_random_pieces_against_libzstd():
    """300 pieces with a largest symbol of 129 .. 255, from 2 symbols to all of them, flat to steep; the largest tree met
    is printed"""
    r = np.random.default_rng(1)
    largest = 0
    for _ in range(300):
        top = int(r.integers(129, 256))
        m = int(r.integers(2, top + 2))
        n = int(r.integers(50, 5000))
        syms = np.concatenate([r.choice(top, m - 1, replace=False), [top]]).astype(np.uint8)
        p = r.dirichlet(np.ones(m) * float(r.choice([0.05, 0.3, 1, 5])))
        f = bytes(syms[r.choice(m, n, p=p)]) + bytes([top])
        info = {}
        W.huf_block_candidate(f, None, info)
        largest = max(largest, info.get("tree", 0))
        W.roundtrip(f)
    print("largest tree: %d bytes behind its header byte" % largest)
    assert 0 < largest <= W.MAX_TREE
