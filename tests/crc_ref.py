"""The reference of the checksum wire pass for tests/crc_cases.py.  TESTS ONLY.

Frame CRC, header and packet CRC are the bitwise oracle's (orc.crc32c, orc.ascii_frame_packet; pinned on RFC 3720 in
test_crc_wire.py); the packed layout is packed_reference (pack_frames_kernel's: frame i at the sum of the 16-byte rounded
lengths in front of it).  Nothing here calls the emulator or includes the kernels' helpers.

packet_crc_from_frame_crc() is for crc_packets_kernel at lengths where no frame can be held in memory: the packet CRC from
the frame's CRC and length alone, in integer polynomial arithmetic over GF(2).  Polynomials are Python ints, bit k the
coefficient of x^k; a CRC register (reflected: bit 31 is x^0) is one bit reversal away.  The register after message M from
register I is I * x^(8|M|) + M * x^32 mod P, so two registers after the same frame from different starts differ by
(I1 + I2) * x^(8|M|), with x^(8|M|) by square-and-multiply.  test_crc_boundaries.py checks it against
orc.ascii_frame_packet on real frames before anything else relies on it."""
import struct

import numpy as np

import orc

ERR_FROM = 0xFFFFFFF0  # lengths from here up are the render kernels' error codes
POLY_REFLECTED = 0x82F63B78


def packed_reference(slab, stride, lens):
    """off[i] = sum_{j<i} round16(len_ok[j]); frame i's bytes at off[i]"""
    off, out = [], bytearray()
    for i, l in enumerate(lens):
        l = 0 if l >= 0xFFFFFFF0 else int(l)
        off.append(len(out))
        out += slab[i * stride:i * stride + l].tobytes()
        out += bytes((-l) % 16)
    return off + [len(out)], bytes(out)


# ---- GF(2)[x] mod P, natural bit order ------------------------------------------------------------------------------------
def _rev32(v):
    return int(f"{v & 0xFFFFFFFF:032b}"[::-1], 2)


_P = (1 << 32) | _rev32(POLY_REFLECTED)  # x^32 + ... + 1 (0x1EDC6F41 with its leading term)


def _mod(a):
    while a.bit_length() > 32:
        a ^= _P << (a.bit_length() - 33)
    return a


def _mul(a, b):
    p = 0
    while b:
        if b & 1:
            p ^= a
        a <<= 1
        b >>= 1
    return _mod(p)


def _x_pow(e):
    r, base = 1, 2
    while e:
        if e & 1:
            r = _mul(r, base)
        base = _mul(base, base)
        e >>= 1
    return r


def _register_after(data, reg=0xFFFFFFFF):
    """the reflected CRC register after `data`, bit by bit"""
    for b in data:
        reg ^= b
        for _ in range(8):
            reg = (reg >> 1) ^ POLY_REFLECTED if reg & 1 else reg >> 1
    return reg


def header_bytes(w, h, length, crc):
    """ascii_frame_packet_t {width, height, original_size, compressed_size = 0, checksum, flags = 0}, network byte order"""
    return struct.pack(">6I", w, h, length, 0, crc, 0)


_XPOW = {}


def packet_crc_from_frame_crc(w, h, length, crc):
    """-> (header, CRC of header || frame) for a frame of `length` bytes whose CRC-32C is `crc`; an error code as length
    gives the zero header and packet CRC 0"""
    if length >= ERR_FROM:
        return header_bytes(0, 0, 0, 0), 0
    hdr = header_bytes(w, h, length, crc)
    if length not in _XPOW:
        _XPOW[length] = _x_pow(8 * length)
    after_frame = _rev32(crc ^ 0xFFFFFFFF)                       # from 0xFFFFFFFF
    start = _rev32(_register_after(hdr)) ^ 0xFFFFFFFF            # the two starting registers' difference
    return hdr, _rev32(after_frame ^ _mul(start, _XPOW[length])) ^ 0xFFFFFFFF


# ---- what a call over a batch of tests/crc_cases.py must leave -------------------------------------------------------------
def expect(frames, lens, dims):
    """frames[i]: bytes, or None behind an error code.  -> dict(crc uint32[n], hdr uint8[24 n], pkt uint32[n],
    hdr0 / pkt0: the same without dims (zero dimensions in the headers))"""
    n = len(frames)
    crc = np.zeros(n, dtype=np.uint32)
    pkt = np.zeros(n, dtype=np.uint32)
    pkt0 = np.zeros(n, dtype=np.uint32)
    hdr, hdr0 = bytearray(), bytearray()
    for i, f in enumerate(frames):
        if lens[i] >= ERR_FROM:
            assert f is None
            hdr += header_bytes(0, 0, 0, 0)
            hdr0 += header_bytes(0, 0, 0, 0)
            continue
        assert len(f) == lens[i]
        w, h = dims[i]
        hd, pk = orc.ascii_frame_packet(f, w, h)
        crc[i] = orc.crc32c(f)
        assert hd == header_bytes(w, h, len(f), int(crc[i]))
        hdr += hd
        pkt[i] = pk
        hd0, pk0 = orc.ascii_frame_packet(f, 0, 0)
        hdr0 += hd0
        pkt0[i] = pk0
    return dict(crc=crc, hdr=np.frombuffer(bytes(hdr), dtype=np.uint8), pkt=pkt,
                hdr0=np.frombuffer(bytes(hdr0), dtype=np.uint8), pkt0=pkt0)


# ---- comparing a call's outputs ---------------------------------------------------------------------------------------------
SENTINEL_WORD = 0x5A5A5A5A  # what the tests prefill output words with
SENTINEL_BYTE = 0xEE        # ... and header and destination bytes


def _same(got, want, what, lens):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if bad.size:
        k = int(bad[0])
        i = k // (got.size // len(lens))
        raise AssertionError(f"{what}: {bad.size} elements differ, the first at {k} (frame {i}, length word {lens[i]:#x}): "
                             f"{int(got[k]):#x}, expected {int(want[k]):#x}")


def check_outputs(exp, lens, crc, hdr=None, pkt=None, with_dims=True, what=""):
    """every element of every output array against expect()'s; hdr / pkt None: the call was made without them"""
    _same(crc, exp["crc"], f"{what}: frame CRC", lens)
    if hdr is not None:
        _same(hdr, exp["hdr" if with_dims else "hdr0"], f"{what}: header bytes", lens)
    if pkt is not None:
        _same(pkt, exp["pkt" if with_dims else "pkt0"], f"{what}: packet CRC", lens)


def check_packed(slab, stride, lens, cap, off, len_out, dst, what=""):
    """the COPY forms' side of a call over `slab`: dst is the whole destination array (prefilled with SENTINEL_BYTE, longer
    than cap)"""
    n = len(lens)
    want_off, want = packed_reference(slab, stride, lens)
    _same(off, np.array(want_off, dtype=np.uint64), f"{what}: offsets and total", list(lens) + [0])
    _same(len_out, np.array(lens, dtype=np.uint32), f"{what}: copied lengths", lens)
    for i in range(n):
        if lens[i] >= ERR_FROM:
            continue
        o, l = want_off[i], int(lens[i])
        if o + (l + 15) // 16 * 16 <= cap:  # frames travel in whole groups: the last one must fit too
            assert dst[o:o + l].tobytes() == want[o:o + l], (what, "frame bytes", i, l)
        elif o < cap:  # untouched from the first group that would cross the capacity
            g0 = o + (cap - o) // 16 * 16
            assert (dst[g0:cap] == SENTINEL_BYTE).all(), (what, "a frame that does not fit was stored", i, l)
    assert (dst[cap:] == SENTINEL_BYTE).all(), (what, "bytes at or behind dst + capacity changed")
    assert (dst[want_off[n]:] == SENTINEL_BYTE).all(), (what, "bytes behind the packed frames changed")
