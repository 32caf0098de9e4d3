"""Wide zhuf form test support: the cases the restatement, the emulated and the GPU tests share, the wide kernels under the
CPU emulator (tests/hipemu/zwide_emu_driver.cpp), and the check of a call's outputs against the restatement
(tests/zwide_ref.py), as zpack_support.check does it for the narrow form.  TESTS ONLY."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import orc
import zhuf_ref as Z
import zpack_support as ZS
import zwide_ref as W

FILL, ERR = ZS.FILL, ZS.ERR
HALF = "▀".encode()  # E2 96 80


# ---- inputs ------------------------------------------------------------------------------------------------------------
def from_lengths(lens, seed, least=2048):
    """a piece whose symbols get exactly these code lengths: dyadic counts 2^(K - length), shuffled; at least `least` bytes"""
    assert sum(2.0 ** -d for d in lens.values()) == 1.0
    k = max(lens.values())
    while sum(1 << (k - d) for d in lens.values()) < least:
        k += 1
    a = np.concatenate([np.full(1 << (k - d), s, dtype=np.uint8) for s, d in sorted(lens.items())])
    np.random.default_rng(seed).shuffle(a)
    return bytes(a)


def zero_run(z, top=0xE2, max_bits=11):
    """a piece whose table description skips z absent weight values in one run (z = 0: none at all): weights 1 and
    z + 2 .. max_bits present, weight 0 too (symbols below `top` are absent)"""
    a = z + 2
    syms = list(range(0x20, 0x20 + (1 << (a - 1)))) + [top - k for k in range(max_bits - a + 1)]
    assert len(set(syms)) == len(syms)
    lens = {s: max_bits for s in syms[:1 << (a - 1)]}
    for k, w in enumerate(range(max_bits, a - 1, -1)):  # (the weight of `top` is not listed: it takes the last value)
        lens[top - k] = max_bits + 1 - w
    return from_lengths(lens, 40 + z)


def skewed_high(n, seed, top=0xFF, spread=0.3, symbols=None):
    """n bytes with a geometric histogram over `symbols` distinct values ending at `top`"""
    r = np.random.default_rng(seed)
    m = top + 1 if symbols is None else symbols
    order = r.permutation(top)[:m - 1]
    pal = np.concatenate([[top], order]).astype(np.uint8)
    idx = np.minimum(r.geometric(spread, n) - 1, m - 1)
    idx[:m] = np.arange(m)  # every symbol is there
    r.shuffle(idx)
    return bytes(pal[idx])


def halfblock_truecolor(w, h, seed):
    """a synthetic truecolor half-block frame: ESC[38;2;..m ESC[48;2;..m + E2 96 80 per cell"""
    r = np.random.default_rng(seed)
    rows = []
    for _ in range(h):
        rows.append("".join("\x1b[38;2;%d;%d;%dm\x1b[48;2;%d;%d;%dm▀" % tuple(r.integers(0, 256, 6)) for _ in range(w)))
    return ("\x1b[0m\n".join(rows) + "\x1b[0m").encode()


def utf8_truecolor(w, h, seed, palette=" ░▒▓█"):
    """a synthetic truecolor-foreground frame over a palette of multi-byte glyphs"""
    r = np.random.default_rng(seed)
    rows = []
    for _ in range(h):
        rows.append("".join("\x1b[38;2;%d;%d;%dm%s" % (*r.integers(0, 256, 3), palette[int(r.integers(0, len(palette)))]) for _ in range(w)))
    return ("\x1b[0m\n".join(rows) + "\x1b[0m").encode()


def info_of(piece):
    """what the restatement's encoder met in one piece: form, dec, add, runs, bits, tree; "coded": the block gains"""
    info = {}
    body = W.huf_block_body(piece, None, info)
    info["coded"] = body is not None
    return info


def _search(make, want, what, tries=400):
    for seed in range(tries):
        f = make(seed)
        if want(info_of(f)):
            return f
    raise AssertionError("no piece with " + what)


def stream_bits(residue):
    """a piece whose weights' FSE bitstream holds residue (mod 8) bits before its end mark"""
    return _search(lambda s: skewed_high(1500 + 7 * s, 300 + s, top=0x90 + s % 100, symbols=20 + s % 90),
                   lambda i: i["coded"] and i["form"] == "fse" and i["bits"] % 8 == residue, "%d bits mod 8" % residue)


def csize_of(body):
    fmt = (body[0] >> 2) & 3
    return (int.from_bytes(body[:2 + fmt], "little") >> 4) >> {1: 10, 2: 14, 3: 18}[fmt]


def with_csize(target):
    """a piece with a byte above 0x80 whose literals section is exactly `target` bytes: a prefix of one skewed stream"""
    for seed in range(80, 90):
        stream = skewed_high(4 * target, seed, top=0xE2, symbols=40, spread=0.35)
        n = 2 * target
        for _ in range(8):
            n = max(64, min(len(stream), n * target // csize_of(W.huf_block_candidate(stream[:n]))))
        for k in range(max(64, n - 40), min(len(stream), n + 40)):
            if csize_of(W.huf_block_candidate(stream[:k])) == target:
                return stream[:k]
    raise AssertionError("no piece of that compressed size")


_cases = None


def wide_cases():
    """name -> frame bytes (or an error code): the families of the wide form; every one of them is a single piece"""
    global _cases
    if _cases is not None:
        return _cases
    r = np.random.default_rng(77)
    out = {
        "error code": ERR,
        "empty": b"",
        "top 128 (direct form)": ZS.skewed(2500, 10) + b"\x80" * 3,
        "top 129 (odd count of weights)": ZS.skewed(2500, 11) + b"\x81" * 3,
        "top 130 (even count)": ZS.skewed(2500, 12) + b"\x82" * 5,
        "top 254": skewed_high(3000, 13, top=254, symbols=60),
        "top 255": skewed_high(3000, 14, top=255, symbols=61),
        "two symbols, one above 0x80": bytes(r.integers(0, 2, 3000, dtype=np.uint8) * 0xA1 + 0x41),
        "all 256 symbols skewed": skewed_high(6000, 15, spread=0.08),
        "256 equal counts (raw)": bytes(r.permutation(np.repeat(np.arange(256, dtype=np.uint8), 8))),
        "uniform bytes (raw by size)": bytes(r.integers(0, 256, 3000, dtype=np.uint8)),
        "one byte value above 0x80 (RLE)": b"\xe2" * 2000,
        "half blocks below the size floor (as it is)": (HALF * 340)[:1020],
        "half-block truecolor 20x6": halfblock_truecolor(20, 6, 16),
        "utf-8 palette truecolor 20x6": utf8_truecolor(20, 6, 17),
        "another error code": 0xFFFFFFFF,
        "bitstream of 0 bits mod 8": stream_bits(0),
        "bitstream of 7 bits mod 8": stream_bits(7),
        "csize 1023": with_csize(1023),
        "csize 1024": with_csize(1024),
    }
    for z in (0, 1, 2, 3, 4, 6):
        out["zero run of %d weight values" % z] = zero_run(z)
    out["normalisation decrements"] = zero_run(5, top=0xF0)  # three lone weight values rounded up to 1: 66 cells asked for
    # all 256 symbols: one at length 1, 50 / 107 / 98 at lengths 8 / 9 / 10 -- the floors of 64 c / 255 come to 63
    lens = {0x20: 1}
    rest = [x for x in range(256) if x != 0x20]
    lens.update({x: 8 for x in rest[:50]})
    lens.update({x: 9 for x in rest[50:157]})
    lens.update({x: 10 for x in rest[157:]})
    out["normalisation adds"] = from_lengths(lens, 61)
    _cases = out
    return out


# ---- expectation -------------------------------------------------------------------------------------------------------
_wire = {}


def wire_of(frame, piece=W.PIECE):
    if (frame, piece) not in _wire:
        _wire[frame, piece] = W.wire(frame, piece)
    return _wire[frame, piece]


def expect(frames, dims, piece=W.PIECE):
    """-> per frame dict(sent, payload, hdr, crc, pkt, off), total"""
    res, off = [], 0
    for f, (w, h) in zip(frames, dims):
        if isinstance(f, int):
            res.append(dict(sent=0, len_out=f, payload=b"", hdr=bytes(24), crc=0, pkt=0, off=off, flags=0))
            continue
        payload, csz, flags = wire_of(f, piece)
        crc = orc.crc32c(f)
        hdr = Z.packet_header(w, h, len(f), csz, crc, flags)
        res.append(dict(sent=len(payload), len_out=len(payload), payload=payload, hdr=hdr, crc=crc, pkt=orc.crc32c(hdr + payload),
                        off=off, flags=flags))
        off += (len(payload) + 15) // 16 * 16
    return res, off


def check(frames, dims, out, capacity, what="", piece=W.PIECE):
    """zpack_support.check against the wide restatement: offsets, sent lengths, checksums, headers as the reference's
    receiver checks them, packet checksums, payloads byte for byte and decoded back (subset decoder, libzstd), and no store
    outside the frames"""
    exp, total = expect(frames, dims, piece)
    n = len(frames)
    assert int(out["off"][n]) == total, (what, int(out["off"][n]), total)
    written = np.zeros(len(out["dst"]), dtype=bool)
    for i, (f, e) in enumerate(zip(frames, exp)):
        tag = f"{what} frame {i}"
        assert int(out["off"][i]) == e["off"], tag
        assert int(out["len_out"][i]) == e["len_out"], (tag, int(out["len_out"][i]), e["len_out"])
        assert int(out["crc"][i]) == e["crc"], tag
        hdr = out["hdr"][24 * i:24 * i + 24].tobytes()
        assert hdr == e["hdr"], (tag, hdr.hex(), e["hdr"].hex())
        assert int(out["pkt"][i]) == e["pkt"], tag
        if isinstance(f, int):
            continue
        w_, h_, orig, csz, cks, flags = struct.unpack(">6I", hdr)
        assert orig == len(f) and cks == orc.crc32c(f) and flags == e["flags"]
        assert (csz == e["sent"] and flags == Z.FLAG_COMPRESSED) or (csz == 0 and flags == 0 and e["sent"] == len(f))
        room = (e["sent"] + 15) // 16 * 16
        if e["off"] + room > capacity:
            continue
        got = out["dst"][e["off"]:e["off"] + e["sent"]].tobytes()
        assert got == e["payload"], (tag, "payload differs at", next(k for k in range(len(got)) if got[k] != e["payload"][k]))
        if flags:
            assert W.decode(got, piece) == f, tag
            if Z.libzstd() is not None:
                assert Z.zstd_decompress(got, len(f)) == f, tag
            written[e["off"]:e["off"] + e["sent"]] = True
        else:
            written[e["off"]:e["off"] + room] = True
    assert (out["dst"][~written] == FILL).all(), f"{what}: a store outside the frames ({np.flatnonzero((out['dst'] != FILL) & ~written)[:4]})"


# ---- the emulator ------------------------------------------------------------------------------------------------------
_emu = {}


def emulator(piece=W.PIECE):
    """the emulator library of the wide kernels; another piece size gives a second library built with that ACHIP_ZPACK_PIECE"""
    if piece not in _emu:
        drv = os.path.join(ZS.EMU_DIR, "zwide_emu_driver.cpp")
        srcs = [drv, os.path.join(ZS.EMU_DIR, "hip_emu.h"), os.path.join(ZS.EMU_DIR, "gfx950_ops.hpp")] + \
               [os.path.join(ZS.CSRC, f) for f in ("zpack_kernels.hpp", "zpack.h", "crc_math.hpp", "render_kernels.hpp")]
        so = os.path.join(ZS.OUT_DIR, "libzwide_emu.so" if piece == W.PIECE else "libzwide_emu_%d.so" % piece)
        define = [] if piece == W.PIECE else ["-DACHIP_ZPACK_PIECE=%du" % piece]
        if not (os.path.exists(so) and all(os.path.getmtime(s) <= os.path.getmtime(so) for s in srcs)):
            os.makedirs(ZS.OUT_DIR, exist_ok=True)
            tmp = so + ".%d.tmp" % os.getpid()
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I" + ZS.EMU_DIR, "-I" + ZS.CSRC, "-I" + ZS.INC] + define +
                                  [drv, "-o", tmp])
            os.replace(tmp, so)
        L = C.CDLL(so)
        vp = C.c_void_p
        L.emu_zwide_scratch_bytes.restype = C.c_size_t
        L.emu_zwide_scratch_bytes.argtypes = [C.c_uint32, C.c_int]
        L.emu_zwide.restype = None
        L.emu_zwide.argtypes = [vp, C.c_uint64, vp, C.c_uint32, C.c_int, vp, vp, vp, vp, vp, C.c_uint64, vp, vp, vp]
        L.emu_zwide_piece.restype = C.c_uint32
        L.emu_zwide_rec_words.restype = C.c_uint32
        assert L.emu_zwide_piece() == piece and L.emu_zwide_rec_words() == REC_WORDS
        _emu[piece] = L
    return _emu[piece]


def emu_run(frames, dims, capacity=None, tail=256, piece=W.PIECE, stride=None):
    """the four kernels in their wide form over the frames -> (out dict for check() and the scratch records, capacity)"""
    L = emulator(piece)
    n = len(frames)
    slab0, stride, ln, mx = ZS.slab_of(frames, stride)
    slab = ZS._aligned(len(slab0) + 16, FILL)
    slab[:len(slab0)] = slab0
    _, total = expect(frames, dims, piece)
    cap = total if capacity is None else capacity
    dst = ZS._aligned(max(cap, total) + tail, FILL)
    off = np.full(n + 1, 0xEEEEEEEE, dtype=np.uint64)
    len_out = np.full(n, 0xEEEEEEEE, dtype=np.uint32)
    crc = np.full(n, 0xEEEEEEEE, dtype=np.uint32)
    pkt = np.full(n, 0xEEEEEEEE, dtype=np.uint32)
    hdr = ZS._aligned(24 * n, FILL)
    d = np.array(dims, dtype=np.uint32).reshape(n, 2)
    scratch = np.full(L.emu_zwide_scratch_bytes(mx, n) // 4, 0xEEEEEEEE, dtype=np.uint32)
    L.emu_zwide(slab.ctypes.data, stride, ln.ctypes.data, mx, n, d.ctypes.data, crc.ctypes.data, hdr.ctypes.data, pkt.ctypes.data,
                dst.ctypes.data, cap, off.ctypes.data, len_out.ctypes.data, scratch.ctypes.data)
    return dict(dst=dst, off=off, len_out=len_out, crc=crc, hdr=hdr, pkt=pkt, scratch=scratch, pieces=max(1, -(-mx // piece))), cap


# ---- the wide scratch records (csrc/zpack.h) -----------------------------------------------------------------------------
REC_WORDS, ZR_KIND, ZR_MAXBITS, ZR_TABLE, ZWR_TREELEN, ZWR_TREE = 320, 0, 8, 16, 272, 276


def device_record(out, i, p=0):
    """-> (block type, 256 words code | length << 16, maxBits, tree bytes of the FSE form) measure left for piece p of frame i"""
    rec = out["scratch"][(i * out["pieces"] + p) * REC_WORDS:][:REC_WORDS]
    tree = rec[ZWR_TREE:ZWR_TREE + 32].tobytes()[:int(rec[ZWR_TREELEN])] if int(rec[ZR_KIND]) == 2 else b""
    return int(rec[ZR_KIND]), [int(x) for x in rec[ZR_TABLE:ZR_TABLE + 256]], int(rec[ZR_MAXBITS]), tree


def check_records(frames, out, piece=W.PIECE):
    """every coded piece's table and tree in the scratch records against the restatement's"""
    coded = 0
    for i, f in enumerate(frames):
        if isinstance(f, int):
            continue
        for p in range(max(1, -(-len(f) // piece))):
            part = f[p * piece:(p + 1) * piece]
            kind, table, dev_bits, tree = device_record(out, i, p)
            t, info = [], {}
            body = W.huf_block_body(part, t, info)
            assert (kind == 2) == (body is not None), (i, p, kind)
            if body is None:
                continue
            coded += 1
            codes, max_bits = Z.canonical_codes(t[0])
            assert dev_bits == max_bits and table == [c | (d << 16) if d else 0 for c, d in zip(codes, t[0])], (i, p)
            if info["form"] == "fse":
                hl = 2 + ((body[0] >> 2) & 3)
                assert tree == body[hl:hl + 1 + body[hl]], (i, p, tree.hex())
    return coded
