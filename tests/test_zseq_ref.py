"""The zseq wire form (sequence form) as tests/zseq_ref.py restates it: every case of tests/zseq_cases.py (each
asserts its premise when it is built) goes encode -> decode (the subset decoder written from the format) and encode ->
libzstd's ZSTD_decompress, and must give back the original bytes; the coding tables, the code tables and the wire rule."""
import numpy as np
import pytest

import zhuf_ref as Z
import zpack_support as ZS
import zseq_cases as SC
import zseq_ref as S
import zwide_ref as W
import zwide_support as WS

CASES = SC.cases()
CUTS = SC.cases(SC.SMALL)


def test_libzstd_is_the_judge_here():
    assert Z.libzstd() is not None


@pytest.mark.parametrize("name", [k for k, v in CASES.items() if not isinstance(v, int)])
def test_every_case_round_trips(name):
    f = CASES[name]
    z = S.roundtrip(f)
    payload, csz, flags = S.wire(f)
    if len(f) <= 1024 or 5 * len(z) >= 4 * len(f):
        assert (payload, csz, flags) == (f, 0, 0), name
        assert "as it is" in name or "no sequence" in name or len(f) <= 1024, name
    else:
        assert (payload, csz, flags) == (z, len(z), Z.FLAG_COMPRESSED), name


@pytest.mark.parametrize("name", [k for k, v in CUTS.items() if not isinstance(v, int)])
def test_block_cut_cases_round_trip_at_a_small_piece(name):
    f = CUTS[name]
    z = S.roundtrip(f, SC.SMALL)
    assert [k for k, _, _ in Z.blocks(z)] == [i["kind"] for i in SC.infos_of(f, SC.SMALL)]


def test_the_batch_takes_every_path():
    kinds, lit_forms = set(), set()
    for f in CASES.values():
        if isinstance(f, int):
            continue
        flags = S.wire(f)[2]
        for info in SC.infos_of(f):
            kinds.add(("zseq" if flags else "as is", info["kind"]))
            if info["kind"] == 2:
                lit = info["lit_section"]
                lit_forms.add("raw" if lit[0] & 3 == 0 else "fse" if lit[2 + ((lit[0] >> 2) & 3)] < 128 else "direct")
    assert {("zseq", 0), ("zseq", 1), ("zseq", 2), ("as is", 0), ("as is", 2)} <= kinds and lit_forms == {"raw", "fse", "direct"}


def test_code_tables():
    """the baselines follow from the extra bits; codes at every step of both tables"""
    for base, bits, first in ((S.LL_BASE, S.LL_BITS, 16), (S.ML_BASE, S.ML_BITS, 32)):
        for c in range(first, len(base) - 1):
            assert base[c + 1] == base[c] + (1 << bits[c])
    assert [S.ll_code(v) for v in (0, 15, 16, 17, 18, 23, 24, 63, 64, 127, 128, 8191)] == [0, 15, 16, 16, 17, 19, 20, 24, 25, 25, 26, 31]
    assert [S.ml_code(v) for v in (3, 4, 34, 35, 36, 37, 42, 43, 66, 67, 98, 99, 130)] == [0, 1, 31, 32, 32, 33, 35, 36, 39, 40, 41, 42, 42]
    assert [S.of_code(d) for d in (1, 4, 5, 12, 13, 28, 29, 60, 61, 64)] == [2, 2, 3, 3, 4, 4, 5, 5, 6, 6]


def test_predefined_tables_against_the_decoding_tables():
    """the coding table walks the decoding table backwards: from every state of the decoder, the symbol it emits and the bits
    it reads lead the encoder (put) from the state reached back to that state"""
    for dist, log in ((S.LL_DIST, S.LL_LOG), (S.ML_DIST, S.ML_LOG), (S.OF_DIST, S.OF_LOG)):
        size = 1 << log
        st, dnb, dfs = S.coding_table(dist, log)
        table = S._decoding_table(dist, log)
        assert sorted(st) == list(range(size, 2 * size))
        for cell, (sym, nb, base) in enumerate(table):
            for low in range(1 << nb):
                state = size + base + low  # the decoder's next state, as the encoder numbers it
                enc_nb = (state + dnb[sym]) >> 16
                assert enc_nb == nb and state & ((1 << nb) - 1) == low
                assert st[(state >> nb) + dfs[sym]] == size + cell


def test_one_sequence_and_many():
    f = b"abcdabcd" + SC.rnd(30, 1)
    infos = SC.infos_of(f)
    assert infos[0]["seqs"] == [(4, 4, 4)]
    S.roundtrip(f)
    f = SC.units([(4, 4, 4)] * 2040, 3)[:8192 * 2]
    assert max(len(i["seqs"]) for i in SC.infos_of(f)) > 1000  # the two-byte sequence count
    S.roundtrip(f)


def test_wide_cases_travel_no_larger_than_in_the_wide_form_where_they_hold_matches():
    """the truecolor stand-ins of the issue: smaller than the wide form's payload"""
    for f in (ZS.ansi_truecolor(80, 24, 1), WS.halfblock_truecolor(80, 24, 2)):
        S.roundtrip(f)
        assert len(S.wire(f)[0]) < len(W.wire(f)[0])


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("level,mode,what", [(3, 0, "truecolor fg"), (3, 2, "half-block truecolor")])
def test_real_renders_travel_smaller_than_in_the_wide_form(kind, level, mode, what):
    """the issue's condition over the oracle's 1080p -> 80x24 renders of the S-noise and the S-smooth input: the zseq payload is
    smaller than the wide form's (scripts/zseq_timing.py --cpu records the ratios: profiles/zseq_timing.txt), and libzstd reads it"""
    import orc
    img = orc.frame_noise(1920, 1080) if kind == "noise" else orc.frame_smooth(1920, 1080)
    f = orc.convert_with_caps(img, 80, 24, level, mode, False, False, False)
    z = S.roundtrip(f)
    seq, wide = S.wire(f), W.wire(f)
    print(f"{what}, S-{kind}: {len(f)} bytes, zseq {len(seq[0]) / len(f):.3f}, wide zhuf {len(wide[0]) / len(f):.3f}")
    assert seq == (z, len(z), Z.FLAG_COMPRESSED) and wide[2] == Z.FLAG_COMPRESSED
    assert len(seq[0]) < len(wide[0])


def test_the_decoder_refuses_what_is_outside_the_subset():
    f = CASES["a match at position 6 of the frame"]
    z = S.encode(f)
    info = SC.infos_of(f)[0]
    at = 12 + len(info["lit_section"])
    assert z[at] == len(info["seqs"]) and z[at + 1] == 0
    bad = bytearray(z)
    bad[at + 1] = 0x40  # Offsets in RLE_Mode
    with pytest.raises(Z.FormatError):
        S.decode(bytes(bad))
    bad = bytearray(z)
    bad[-1] = 0  # no end mark
    with pytest.raises(Z.FormatError):
        S.decode(bytes(bad))
    with pytest.raises(Z.FormatError):
        S.decode(z[:-1])


def test_random_frames_against_libzstd():
    """200 frames between noise and text at piece sizes 512, 2048 and 8192: alphabets of 2 .. 256 symbols, runs and copies"""
    r = np.random.default_rng(2)
    seqs = 0
    for k in range(200):
        n = int(r.integers(1, 6000))
        m = int(r.integers(2, 257))
        f = bytearray(r.integers(0, m, n, dtype=np.uint8).tobytes())
        for _ in range(int(r.integers(0, 40))):  # copies from a little way back
            at, d, ln = int(r.integers(0, n)), int(r.integers(1, 90)), int(r.integers(1, 200))
            for j in range(at, min(n, at + ln)):
                if j - d >= 0:
                    f[j] = f[j - d]
        piece = (512, 2048, 8192)[k % 3]
        S.roundtrip(bytes(f), piece)
        seqs += sum(len(i.get("seqs", [])) for i in SC.infos_of(bytes(f), piece))
    assert seqs > 2000
