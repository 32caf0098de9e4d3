"""The zhuf form as tests/zhuf_ref.py restates it: every case goes encode -> decode (the subset decoder,
written from the format) and encode -> libzstd's ZSTD_decompress, and must give back the original bytes; every code table has
maxBits <= 11 and a Kraft sum of exactly 1."""
import os
import struct

import numpy as np
import pytest

import orc
import zhuf_ref as Z
import zpack_support as ZS


def test_libzstd_is_the_judge_here():
    """libzstd.so.1 loads on the machines that run the CPU suite: the libzstd leg of every case below really runs"""
    assert Z.libzstd() is not None
    raw = b"\x28\xb5\x2f\xfd\xa0\x03\x00\x00\x00" + b"\x19\x00\x00" + b"abc"  # one raw block, last
    assert Z.zstd_decompress(raw, 3) == b"abc" == Z.decode(raw)
    with pytest.raises(Z.FormatError):
        Z.zstd_decompress(raw[:-1], 3)


def _tables(frame):
    t = []
    z = Z.encode(frame, t)
    for lens in t:
        Z.check_table(lens)  # maxBits <= 11, Kraft sum exactly 1
    return z, t


def _blocks(z):
    """[(type, size)] of a zhuf frame"""
    at, out, last = 9, [], False
    while not last:
        h = int.from_bytes(z[at:at + 3], "little")
        last, kind, size = bool(h & 1), (h >> 1) & 3, h >> 3
        out.append((kind, size))
        at += 3 + (1 if kind == 1 else size)
    assert at == len(z)
    return out


@pytest.mark.parametrize("n", [0, 1, 5, 1024, 1025, 1026, 1027, 1028, 16, 17, 18])
def test_lengths(n):
    f = ZS.skewed(n, 100 + n)
    z = Z.roundtrip(f)
    _tables(f)
    assert struct.unpack("<I", z[5:9])[0] == n and z[:5] == b"\x28\xb5\x2f\xfd\xa0"
    payload, csz, flags = Z.wire(f)
    if n <= 1024:
        assert (payload, csz, flags) == (f, 0, 0)
    else:
        assert (payload, csz, flags) == (z, len(z), 2) and 5 * len(z) < 4 * n


@pytest.mark.parametrize("n,blocks", [(131072, 1), (131073, 2), (262145, 3)])
def test_pieces(n, blocks):
    f = ZS.skewed(n, 7 + blocks)
    z = Z.roundtrip(f)
    b = _blocks(z)
    assert len(b) == blocks and all(k == 2 for k, _ in b[:n // 131072])
    if n % 131072 == 1:
        assert b[-1] == (1, 1)  # the last piece, one byte: all its bytes are equal


def test_one_and_two_distinct_bytes():
    assert _blocks(Z.roundtrip(b"a" * 2000)) == [(1, 2000)]
    assert len(Z.encode(b"a" * 2000)) == 13
    f = ZS.small_cases()["two byte values"]
    z, t = _tables(f)
    Z.roundtrip(f)
    assert _blocks(z)[0][0] == 2 and sorted(d for d in t[0] if d) == [1, 1]


def test_fibonacci_counts_reach_the_limiter():
    f = ZS.fibonacci()
    hist = [0] * 129
    for b in f:
        hist[b] += 1
    lens = Z.code_lengths(hist)
    Z.check_table(lens)
    assert max(lens) == 11 and sum(1 for d in lens if d) == 20
    # the rarest symbols share the limit, a more frequent symbol never has the longer code
    order = sorted((c, s) for s, c in enumerate(hist) if c)
    assert all(lens[a[1]] >= lens[b[1]] for a, b in zip(order, order[1:]))
    Z.roundtrip(f)


def test_rfc_example_codes():
    codes, max_bits = Z.canonical_codes([1, 2, 3, 0, 4, 4])  # weights 4, 3, 2, 0, 1, (1)
    assert max_bits == 4 and codes == [1, 1, 1, 0, 0, 1]


def test_all_129_symbols_and_the_largest_symbol():
    f = ZS.small_cases()["all 129 symbols"]
    z, t = _tables(f)
    Z.roundtrip(f)
    assert _blocks(z)[0][0] == 2 and all(d > 0 for d in t[0])
    body = z[12:]
    hl = 2 + ((body[0] >> 2) & 3)
    assert body[hl] == 127 + 128  # 128 weights listed, the 129th implied
    g = ZS.small_cases()["S = 128"]
    z, t = _tables(g)
    Z.roundtrip(g)
    assert t[0][128] > 0 and _blocks(z)[0][0] == 2


def test_a_byte_above_0x80_goes_raw():
    f = ZS.small_cases()["0x81 present (raw)"]
    z = Z.roundtrip(f)
    assert _blocks(z) == [(0, len(f))] and Z.wire(f) == (f, 0, 0)
    hb = "▀".encode() * 700  # E2 96 80: every half-block frame
    assert _blocks(Z.roundtrip(hb))[0][0] == 0


def test_uniform_seven_bit_bytes_are_sent_as_they_are():
    f = ZS.uniform7(40000, 3)
    z = Z.roundtrip(f)
    assert 8 * len(z) >= 7 * len(f) and Z.wire(f) == (f, 0, 0)


def _with_sizes(target_regen=None, target_csize=None):
    """a piece whose regenerated (or compressed) literals size is exactly the target"""
    if target_regen is not None:
        return ZS.skewed(target_regen, 50 + target_regen)
    def csize_of(f):
        body = Z.huf_block_body(f)
        fmt = (body[0] >> 2) & 3
        return (int.from_bytes(body[:2 + fmt], "little") >> 4) >> {1: 10, 2: 14, 3: 18}[fmt]

    for seed in range(70, 76):  # prefixes of one skewed stream: the compressed size grows by a bit or two per byte
        stream = ZS.skewed(4 * target_csize, seed)
        n = 2 * target_csize
        for _ in range(8):  # coarse: proportional steps
            n = max(64, min(len(stream), n * target_csize // csize_of(stream[:n])))
        for k in range(max(64, n - 40), min(len(stream), n + 40)):
            if csize_of(stream[:k]) == target_csize:
                return stream[:k]
    raise AssertionError("no piece of that compressed size")


@pytest.mark.parametrize("which,size,fmt", [("regen", 1023, 1), ("regen", 1024, 2), ("regen", 16383, 2), ("regen", 16384, 3),
                                            ("csize", 1023, 2), ("csize", 1024, 2), ("csize", 16383, 3), ("csize", 16384, 3)])
def test_the_three_literals_header_formats(which, size, fmt):
    f = _with_sizes(**{"target_" + which: size})
    body = Z.huf_block_body(f)
    assert body is not None and (body[0] & 3) == 2 and (body[0] >> 2) & 3 == fmt
    Z.roundtrip(f)


def test_compressed_size_1023_in_the_short_format():
    """both sizes below 1024: a piece of 1023 regenerated bytes keeps the 3-byte header whatever it compresses to"""
    body = Z.huf_block_body(ZS.skewed(1023, 9))
    assert (body[0] >> 2) & 3 == 1 and len(body) < 1023


def test_either_side_of_the_ratio():
    """a skewed frame padded with uniform bytes until 5 * zlen passes 4 * len: the frame before goes compressed, that one as
    it is"""
    base = ZS.skewed(6000, 31, spread=0.7)
    pad = ZS.uniform7(60000, 32)

    def over(k):
        f = base + pad[:k]
        return 5 * len(Z.encode(f)) >= 4 * len(f)

    lo, hi = 0, len(pad)  # bisect to a crossing: not over at lo, over at hi
    assert not over(lo), "the unpadded frame already misses the ratio"
    assert over(hi), "never crossed the ratio"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if over(mid):
            hi = mid
        else:
            lo = mid
    below, above = base + pad[:lo], base + pad[:hi]
    zb = Z.roundtrip(below)
    assert 5 * len(zb) < 4 * len(below) and Z.wire(below) == (zb, len(zb), 2)
    za = Z.roundtrip(above)
    assert 5 * len(za) >= 4 * len(above) and Z.wire(above) == (above, 0, 0)
    assert len(above) == len(below) + 1


ORACLE = os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_build"))


@pytest.mark.skipif(not ORACLE, reason="oracle/_build is not present")
@pytest.mark.parametrize("cl,rm", [(3, 0), (2, 0), (1, 0), (0, 0), (3, 1), (3, 2)])
def test_one_real_frame_per_mode(cl, rm):
    img = orc.frame_smooth(320, 180)
    img[40:100, 60:200] = orc.frame_hash_noise(140, 60, 5)
    f = orc.convert_with_caps(img, 80, 24, cl, rm, False, False, False)
    z, _ = _tables(f)
    assert Z.roundtrip(f) == z
    if rm == 2:
        assert Z.wire(f) == (f, 0, 0)  # half blocks: E2 96 80
