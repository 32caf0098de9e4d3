"""zhuf wire pass test support: the cases the restatement, the emulated and the GPU tests share, the four kernels under the
CPU emulator (tests/hipemu/zpack_emu_driver.cpp), and the check of a call's outputs against the restatement.  TESTS ONLY."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import orc
import zhuf_ref as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ascii-chat_amd", "csrc")
INC = os.path.join(ROOT, "include")
EMU_DIR = os.path.join(ROOT, "tests", "hipemu")
OUT_DIR = os.path.join(EMU_DIR, "_build")
LIB = os.path.join(ROOT, "ascii-chat_amd", "libasciichat_hip.so")
FILL = 0xEE   # the destination, the headers and the slab behind every frame before the pass
ERR = 0xFFFFFFF1  # a render error code in place of a length


# ---- inputs ------------------------------------------------------------------------------------------------------------
def skewed(n, seed, spread=0.5, base=0x30, top=0x50):
    """n bytes below 0x80 with a geometric histogram"""
    r = np.random.default_rng(seed)
    return bytes(np.minimum(r.geometric(spread, n) - 1 + base, top).astype(np.uint8))


def uniform7(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 128, n, dtype=np.uint8))


def fibonacci():
    """20 symbols with Fibonacci counts, shuffled: unlimited Huffman depth 19"""
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    a = np.concatenate([np.full(c, s + 1, dtype=np.uint8) for s, c in enumerate(fib)])
    np.random.default_rng(5).shuffle(a)
    return bytes(a)


def ansi_truecolor(w, h, seed):
    """a synthetic truecolor-foreground frame: ESC[38;2;R;G;Bm + glyph per cell"""
    r = np.random.default_rng(seed)
    pal = orc.PALETTE_STANDARD
    rows = []
    for _ in range(h):
        rows.append("".join("\x1b[38;2;%d;%d;%dm%s" % (*r.integers(0, 256, 3), pal[int(r.integers(0, len(pal)))]) for _ in range(w)))
    return ("\x1b[0m\n".join(rows) + "\x1b[0m").encode()


def small_cases():
    """name -> frame bytes (or an error code): what the emulated and the GPU batch run"""
    every = bytes(range(129)) * 6 + skewed(3000, 11)
    out = {
        "error code": ERR,
        "empty": b"",
        "1 byte": b"x",
        "5 bytes": skewed(5, 1),
        "1024 skewed (as it is: the size floor)": skewed(1024, 2),
        "1025 skewed": skewed(1025, 3),
        "1026 skewed": skewed(1026, 4),
        "1027 skewed": skewed(1027, 5),
        "1028 skewed": skewed(1028, 6),
        "one byte value (RLE)": b"a" * 2000,
        "two byte values": bytes(np.random.default_rng(7).integers(0, 2, 3000, dtype=np.uint8) * 5 + 0x41),
        "fibonacci counts (limiter and repair)": fibonacci(),
        "all 129 symbols": every,
        "0x81 present (raw)": skewed(2000, 8) + b"\x81" + skewed(100, 9),
        "S = 128": skewed(2500, 10) + b"\x80" * 3,
        "uniform below 0x80 (as it is: the ratio)": uniform7(2000, 12),
        "another error code": 0xFFFFFFFF,
        "truecolor 20x6": ansi_truecolor(20, 6, 13),
        "17 bytes": skewed(17, 14),
    }
    return out


# ---- expectation -------------------------------------------------------------------------------------------------------
_wire = {}


def wire_of(frame, piece=Z.PIECE):
    """zhuf_ref.wire(frame), computed once per distinct frame (and piece size)"""
    if (frame, piece) not in _wire:
        _wire[frame, piece] = Z.wire(frame, piece)
    return _wire[frame, piece]


def expect(frames, dims, piece=Z.PIECE):
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


def check(frames, dims, out, capacity, what="", piece=Z.PIECE):
    """out: dict(dst, off, len_out, crc, hdr, pkt) of numpy arrays (dst at least `capacity` bytes, FILL before the call)"""
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
        # what parsing.c / protocol.c check of a received frame
        w_, h_, orig, csz, cks, flags = struct.unpack(">6I", hdr)
        assert orig == len(f) and cks == orc.crc32c(f) and flags == e["flags"]
        assert (csz == e["sent"] and flags == Z.FLAG_COMPRESSED) or (csz == 0 and flags == 0 and e["sent"] == len(f))
        room = (e["sent"] + 15) // 16 * 16
        if e["off"] + room > capacity:  # does not fit: not copied
            continue
        got = out["dst"][e["off"]:e["off"] + e["sent"]].tobytes()
        assert got == e["payload"], (tag, "payload differs at", next(k for k in range(len(got)) if got[k] != e["payload"][k]))
        if flags:
            assert Z.decode(got, piece) == f, tag
            if Z.libzstd() is not None:
                assert Z.zstd_decompress(got, len(f)) == f, tag
            written[e["off"]:e["off"] + e["sent"]] = True  # a zhuf frame is stored to the byte
        else:
            written[e["off"]:e["off"] + room] = True  # a frame sent as it is travels in whole groups
    assert (out["dst"][~written] == FILL).all(), f"{what}: a store outside the frames ({np.flatnonzero((out['dst'] != FILL) & ~written)[:4]})"


def slab_of(frames, stride=None):
    """-> (slab bytes with FILL behind every frame, stride, lengths, max_len)"""
    mx = max([len(f) for f in frames if not isinstance(f, int)] + [16])
    if stride is None:
        stride = (mx + 15) // 16 * 16
    slab = np.full(len(frames) * stride, FILL, dtype=np.uint8)
    for i, f in enumerate(frames):
        if not isinstance(f, int):
            slab[i * stride:i * stride + len(f)] = np.frombuffer(f, dtype=np.uint8)
    ln = np.array([f if isinstance(f, int) else len(f) for f in frames], dtype=np.uint32)
    return slab, stride, ln, mx


def dims_of(n):
    return [(80 + i, 24 + 2 * i) for i in range(n)]


# ---- the emulator ------------------------------------------------------------------------------------------------------
_emu = {}


def emulator(piece=Z.PIECE):
    """the emulator library; a piece size other than the product's gives a second library built with that ACHIP_ZPACK_PIECE"""
    if piece not in _emu:
        drv = os.path.join(EMU_DIR, "zpack_emu_driver.cpp")
        srcs = [drv, os.path.join(EMU_DIR, "hip_emu.h"), os.path.join(EMU_DIR, "gfx950_ops.hpp")] + \
               [os.path.join(CSRC, f) for f in ("zpack_kernels.hpp", "zpack.h", "crc_math.hpp", "render_kernels.hpp")]
        so = os.path.join(OUT_DIR, "libzpack_emu.so" if piece == Z.PIECE else "libzpack_emu_%d.so" % piece)
        define = [] if piece == Z.PIECE else ["-DACHIP_ZPACK_PIECE=%du" % piece]
        if not (os.path.exists(so) and all(os.path.getmtime(s) <= os.path.getmtime(so) for s in srcs)):
            os.makedirs(OUT_DIR, exist_ok=True)
            tmp = so + ".%d.tmp" % os.getpid()
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I" + EMU_DIR, "-I" + CSRC, "-I" + INC] + define + [drv, "-o", tmp])
            os.replace(tmp, so)
        L = C.CDLL(so)
        vp = C.c_void_p
        L.emu_zpack_scratch_bytes.restype = C.c_size_t
        L.emu_zpack_scratch_bytes.argtypes = [C.c_uint32, C.c_int]
        L.emu_zpack.restype = None
        L.emu_zpack.argtypes = [vp, C.c_uint64, vp, C.c_uint32, C.c_int, vp, vp, vp, vp, vp, C.c_uint64, vp, vp, vp]
        L.emu_zpack_piece.restype = C.c_uint32
        assert L.emu_zpack_piece() == piece
        _emu[piece] = L
    return _emu[piece]


def _aligned(nbytes, fill):
    raw = np.full(nbytes + 16, fill, dtype=np.uint8)
    o = (-raw.ctypes.data) % 16
    return raw[o:o + nbytes]


def emu_run(frames, dims, capacity=None, tail=256, piece=Z.PIECE, stride=None):
    """the four kernels over the frames -> (out dict for check() and the scratch records, capacity)"""
    L = emulator(piece)
    n = len(frames)
    slab0, stride, ln, mx = slab_of(frames, stride)
    slab = _aligned(len(slab0) + 16, FILL)
    slab[:len(slab0)] = slab0
    _, total = expect(frames, dims, piece)
    cap = total if capacity is None else capacity
    dst = _aligned(max(cap, total) + tail, FILL)
    off = np.full(n + 1, 0xEEEEEEEE, dtype=np.uint64)
    len_out = np.full(n, 0xEEEEEEEE, dtype=np.uint32)
    crc = np.full(n, 0xEEEEEEEE, dtype=np.uint32)
    pkt = np.full(n, 0xEEEEEEEE, dtype=np.uint32)
    hdr = _aligned(24 * n, FILL)
    d = np.array(dims, dtype=np.uint32).reshape(n, 2)
    scratch = np.full(L.emu_zpack_scratch_bytes(mx, n) // 4, 0xEEEEEEEE, dtype=np.uint32)
    L.emu_zpack(slab.ctypes.data, stride, ln.ctypes.data, mx, n, d.ctypes.data, crc.ctypes.data, hdr.ctypes.data, pkt.ctypes.data,
                dst.ctypes.data, cap, off.ctypes.data, len_out.ctypes.data, scratch.ctypes.data)
    return dict(dst=dst, off=off, len_out=len_out, crc=crc, hdr=hdr, pkt=pkt, scratch=scratch, pieces=max(1, -(-mx // piece))), cap


# ---- the scratch records (csrc/zpack.h) --------------------------------------------------------------------------------
REC_WORDS, ZR_KIND, ZR_N, ZR_MAXBITS, ZR_TABLE = 160, 0, 1, 8, 16


def device_table(out, i, p=0):
    """-> (129 words code | length << 16, maxBits) that measure left for piece p of frame i"""
    rec = out["scratch"][(i * out["pieces"] + p) * REC_WORDS:][:REC_WORDS]
    return [int(x) for x in rec[ZR_TABLE:ZR_TABLE + 129]], int(rec[ZR_MAXBITS])
