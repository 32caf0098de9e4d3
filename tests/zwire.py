"""The three compressed wire forms (asciichat_hip_frame_packets_zpacked, ..._wide, ..._seq) described once for their tests: a
record per form, and everything that does not depend on the form -- the expectation from the form's restatement, the check
of a call's outputs against it, the kernels under the CPU emulator (tests/hipemu/zwire_emu_driver.cpp), the buffers of a call
on the GPU, and what the product library refuses before it needs a device.  The inputs and the case tables live in
zpack_support.py, zwide_support.py and zseq_cases.py, which bind these functions to their form; this module imports none of
them (their tables take seconds to build).  TESTS ONLY."""
import collections
import ctypes as C
import os
import struct

import numpy as np

import emubuild
import orc
import zhuf_ref as Z
import zseq_ref as S
import zwide_ref as W

LIB = os.path.join(emubuild.ROOT, "ascii-chat_amd", "libasciichat_hip.so")
FILL = 0xEE   # the destination, the headers and the slab behind every frame before the pass
ERR = 0xFFFFFFF1  # a render error code in place of a length
WIDE_REC_WORDS = 320  # ACHIP_ZPACK_WIDE_REC_WORDS (csrc/zpack.h); emulator() holds it against the header


# ---- the forms ---------------------------------------------------------------------------------------------------------
def _narrow_sizes(scratch):
    narrow = scratch[""]
    assert narrow(0, 4) == 0 and narrow(100, 0) == 0
    one = narrow(131072, 1)
    assert one > 0 and narrow(131073, 1) > one
    assert narrow(36864, 256) == 256 * narrow(36864, 1)


def _wide_sizes(scratch):
    wide = scratch["_wide"]
    assert wide(0, 4) == 0 and wide(100, 0) == 0 and wide(0xFFFFFFF0, 1) == 0
    assert wide(131072, 1) == 4 * (WIDE_REC_WORDS + 8) and wide(131073, 1) == 4 * (2 * WIDE_REC_WORDS + 8)
    assert wide(36864, 256) == 256 * wide(36864, 1) > scratch[""](36864, 256)


def _seq_sizes(scratch):
    seq = scratch["_seq"]
    assert seq(0, 4) == 0 and seq(100, 0) == 0 and seq(0xFFFFFFF0, 1) == 0
    # 64 bytes per block and 32 per frame of records, a slot of min(8192, max_len) bytes (rounded to 16) per block
    assert seq(100, 1) == 64 + 32 + 112 and seq(8192, 1) == 64 + 32 + 8192 and seq(8193, 1) == 2 * (64 + 8192) + 32
    assert seq(36864, 256) == 256 * seq(36864, 1) == 256 * (5 * (64 + 8192) + 32)


# ref: the restatement (wire, decode, PIECE); suffix: of the C entries and the binding's names; index: the emulator driver's
# `form`; piece_macro: what a second emulator library is built with to shrink the form's piece; sizes: the scratch sizes
# check_refusals holds the library to
Form = collections.namedtuple("Form", "ref suffix index piece_macro sizes")
NARROW = Form(Z, "", 0, "ACHIP_ZPACK_PIECE", _narrow_sizes)
WIDE = Form(W, "_wide", 1, "ACHIP_ZPACK_PIECE", _wide_sizes)
SEQ = Form(S, "_seq", 2, "ACHIP_ZSEQ_PIECE", _seq_sizes)
FORMS = (NARROW, WIDE, SEQ)


# ---- expectation -------------------------------------------------------------------------------------------------------
_wire = {}


def wire_of(form, frame, piece=None):
    """the restatement's wire(frame), computed once per form, distinct frame and piece size"""
    key = (form.index, frame, piece or form.ref.PIECE)
    if key not in _wire:
        _wire[key] = form.ref.wire(frame, key[2])
    return _wire[key]


def expect(form, frames, dims, piece=None):
    """-> per frame dict(sent, len_out, payload, hdr, crc, pkt, off, flags), total"""
    res, off = [], 0
    for f, (w, h) in zip(frames, dims):
        if isinstance(f, int):
            res.append(dict(sent=0, len_out=f, payload=b"", hdr=bytes(24), crc=0, pkt=0, off=off, flags=0))
            continue
        payload, csz, flags = wire_of(form, f, piece)
        crc = orc.crc32c(f)
        hdr = Z.packet_header(w, h, len(f), csz, crc, flags)
        res.append(dict(sent=len(payload), len_out=len(payload), payload=payload, hdr=hdr, crc=crc, pkt=orc.crc32c(hdr + payload),
                        off=off, flags=flags))
        off += (len(payload) + 15) // 16 * 16
    return res, off


def check(form, frames, dims, out, capacity, what="", piece=None):
    """out: dict(dst, off, len_out, crc, hdr, pkt) of numpy arrays (dst at least `capacity` bytes, FILL before the call).
    Offsets, sent lengths, checksums, headers byte for byte and as the reference's receiver (parsing.c / protocol.c) reads
    them, packet checksums (0 for an error code), payloads byte for byte and decoded back (the restatement's decoder, libzstd
    where it loads), and no store outside the frames."""
    piece = piece or form.ref.PIECE
    exp, total = expect(form, frames, dims, piece)
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
        if e["off"] + room > capacity:  # does not fit: not copied
            continue
        got = out["dst"][e["off"]:e["off"] + e["sent"]].tobytes()
        assert got == e["payload"], (tag, "payload differs at", next(k for k in range(len(got)) if got[k] != e["payload"][k]))
        if flags:
            assert form.ref.decode(got, piece) == f, tag
            if Z.libzstd() is not None:
                assert Z.zstd_decompress(got, len(f)) == f, tag
            written[e["off"]:e["off"] + e["sent"]] = True  # a compressed frame is stored to the byte
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


def emulator(form, piece=None):
    """the emulator library of the three forms; a piece size other than the product's gives a second library built with
    that value of the form's piece macro"""
    pieces = {f.piece_macro: f.ref.PIECE for f in FORMS}
    pieces[form.piece_macro] = piece or form.ref.PIECE
    key = (pieces["ACHIP_ZPACK_PIECE"], pieces["ACHIP_ZSEQ_PIECE"])
    if key not in _emu:
        so = emubuild.shared_library("libzwire_emu_%d_%d.so" % key, "zwire_emu_driver.cpp",
                                     ("zseq_kernels.hpp", "zpack_kernels.hpp", "zpack.h", "crc_math.hpp", "render_kernels.hpp"),
                                     ["%s=%du" % kv for kv in sorted(pieces.items())])
        L = C.CDLL(so)
        vp = C.c_void_p
        L.emu_zwire_scratch_bytes.restype = C.c_size_t
        L.emu_zwire_scratch_bytes.argtypes = [C.c_int, C.c_uint32, C.c_int]
        L.emu_zwire.restype = None
        L.emu_zwire.argtypes = [C.c_int, vp, C.c_uint64, vp, C.c_uint32, C.c_int, vp, vp, vp, vp, vp, C.c_uint64, vp, vp, vp]
        L.emu_zwire_piece.restype = C.c_uint32
        L.emu_zwire_piece.argtypes = [C.c_int]
        L.emu_zwide_rec_words.restype = C.c_uint32
        L.emu_zseq_tables.restype = C.POINTER(C.c_uint32)
        assert L.emu_zwide_rec_words() == WIDE_REC_WORDS
        assert all(L.emu_zwire_piece(f.index) == pieces[f.piece_macro] for f in FORMS)
        _emu[key] = L
    return _emu[key]


def _aligned(nbytes, fill):
    raw = np.full(nbytes + 16, fill, dtype=np.uint8)
    o = (-raw.ctypes.data) % 16
    return raw[o:o + nbytes]


def emu_run(form, frames, dims, capacity=None, tail=256, piece=None, stride=None):
    """the form's four kernels over the frames -> (out dict for check() with the scratch records, capacity)"""
    piece = piece or form.ref.PIECE
    L = emulator(form, piece)
    n = len(frames)
    slab0, stride, ln, mx = slab_of(frames, stride)
    slab = _aligned(len(slab0) + 16, FILL)
    slab[:len(slab0)] = slab0
    _, total = expect(form, frames, dims, piece)
    cap = total if capacity is None else capacity
    dst = _aligned(max(cap, total) + tail, FILL)
    off = np.full(n + 1, 0xEEEEEEEE, dtype=np.uint64)
    len_out = np.full(n, 0xEEEEEEEE, dtype=np.uint32)
    crc = np.full(n, 0xEEEEEEEE, dtype=np.uint32)
    pkt = np.full(n, 0xEEEEEEEE, dtype=np.uint32)
    hdr = _aligned(24 * n, FILL)
    d = np.array(dims, dtype=np.uint32).reshape(n, 2)
    scratch = _aligned((L.emu_zwire_scratch_bytes(form.index, mx, n) + 7) // 8 * 8, 0xEE).view(np.uint32)
    L.emu_zwire(form.index, slab.ctypes.data, stride, ln.ctypes.data, mx, n, d.ctypes.data, crc.ctypes.data, hdr.ctypes.data, pkt.ctypes.data,
                dst.ctypes.data, cap, off.ctypes.data, len_out.ctypes.data, scratch.ctypes.data)
    return dict(dst=dst, off=off, len_out=len_out, crc=crc, hdr=hdr, pkt=pkt, scratch=scratch, pieces=max(1, -(-mx // piece))), cap


# ---- a call on the GPU -------------------------------------------------------------------------------------------------
class Call:
    """the buffers of one call of a form through the binding; dst in device memory or in mapped host memory"""

    def __init__(self, form, pkg, frames, dims, capacity=None, host=False, tail=256, stride=None):
        import torch
        self.form, self.pkg, self.frames, self.dims, self.n = form, pkg, frames, dims, len(frames)
        slab, self.stride, ln, self.mx = slab_of(frames, stride)
        self.slab = torch.from_numpy(np.concatenate([slab, np.full(16, FILL, dtype=np.uint8)])).cuda()
        self.len = torch.from_numpy(ln.view(np.int32)).cuda()
        self.len_before = ln
        _, total = expect(form, frames, dims)
        self.cap = total if capacity is None else capacity
        self.nbytes = max(self.cap, total) + tail
        self.host = pkg.HostBuffer(self.nbytes) if host else None
        if host:
            self.host.view()[:] = FILL
            self.dst_ptr = self.host.dev
        else:
            self.dst = torch.full((self.nbytes,), FILL, dtype=torch.uint8, device="cuda")
            self.dst_ptr = self.dst.data_ptr()
        n = self.n
        self.off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        self.len_out = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        self.crc = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        self.pkt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        self.hdr = torch.full((24 * n,), FILL, dtype=torch.uint8, device="cuda")
        self.d = torch.from_numpy(np.array(dims, dtype=np.uint32).reshape(n, 2).view(np.int32)).cuda()
        self.sbytes = getattr(pkg, "zpack%s_scratch_bytes" % form.suffix)(self.mx, n)
        self.scratch = torch.full((self.sbytes // 8 + 1,), -1, dtype=torch.int64, device="cuda")

    def launch(self, stream):
        fn = getattr(self.pkg, "frame_packets_zpacked" + self.form.suffix)
        fn(self.slab.data_ptr(), self.stride, self.len.data_ptr(), self.mx, self.n, self.d.data_ptr(), self.crc.data_ptr(), self.hdr.data_ptr(),
           self.pkt.data_ptr(), self.dst_ptr, self.cap, self.off.data_ptr(), self.len_out.data_ptr(), self.scratch.data_ptr(), self.sbytes, stream)

    def out(self):
        dst = self.host.view().copy() if self.host else self.dst.cpu().numpy()
        return dict(dst=dst, off=self.off.cpu().numpy().view(np.uint64), len_out=self.len_out.cpu().numpy().view(np.uint32),
                    crc=self.crc.cpu().numpy().view(np.uint32), hdr=self.hdr.cpu().numpy(), pkt=self.pkt.cpu().numpy().view(np.uint32),
                    scratch=self.scratch.cpu().numpy().view(np.uint32), pieces=max(1, -(-self.mx // self.form.ref.PIECE)))

    def check(self, what):
        """-> out(), checked; the call is over"""
        out = self.out()
        check(self.form, self.frames, self.dims, out, self.cap, what)
        assert np.array_equal(self.len.cpu().numpy().view(np.uint32), self.len_before), "len_dev keeps the original lengths"
        assert (out["dst"][self.cap:] == FILL).all(), "a store at or behind dst + capacity"
        if self.host:
            self.host.close()
        return out


# ---- what the library decides before it needs a device -----------------------------------------------------------------
def check_refusals(form):
    """the form's scratch sizes (the library's and the emulator's agree), every bad argument refused as INVALID_PARAM, and a
    good call that gets as far as needing a device"""
    L = C.CDLL(LIB)
    vp, sz, u32, ci = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int
    scratch = {}
    for f in FORMS:
        scratch[f.suffix] = getattr(L, "asciichat_hip_zpack%s_scratch_bytes" % f.suffix)
        scratch[f.suffix].restype = sz
        scratch[f.suffix].argtypes = [u32, ci]
    frame_packets = getattr(L, "asciichat_hip_frame_packets_zpacked" + form.suffix)
    frame_packets.restype = ci
    frame_packets.argtypes = [vp, sz, vp, u32, ci, vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, vp]
    plan_render_packets = getattr(L, "asciichat_hip_plan_render_packets_zpacked" + form.suffix)
    plan_render_packets.restype = ci
    plan_render_packets.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, vp]
    L.asciichat_hip_device_count.restype = ci
    NO_DEVICE, INVALID = 200, 86
    form.sizes(scratch)
    for mx, n in ((1024, 2), (70000, 3)):
        assert scratch[form.suffix](mx, n) == emulator(form).emu_zwire_scratch_bytes(form.index, mx, n)
    buf = np.zeros(8192 + 64, dtype=np.uint8)
    a = buf.ctypes.data + (-buf.ctypes.data) % 16
    need = scratch[form.suffix](1024, 2)

    def call(base=a, stride=1024, ln=a, mx=1024, n=2, crc=a, hdr=a, dst=a, off=a, lo=a, scratch=a, sbytes=need):
        return frame_packets(base, stride, ln, mx, n, a, crc, hdr, a, dst, 4096, off, lo, scratch, sbytes, None)

    smaller = [dict(sbytes=s) for s in sorted({fn(1024, 2) for fn in scratch.values()}) if s < need]  # another form's scratch
    for bad in [dict(base=None), dict(base=a + 1), dict(stride=1000), dict(ln=None), dict(mx=0), dict(mx=0xFFFFFFF0), dict(n=0),
                dict(crc=None), dict(hdr=None), dict(dst=None), dict(dst=a + 8), dict(off=a + 4), dict(lo=a + 2), dict(scratch=None),
                dict(scratch=a + 4), dict(sbytes=need - 1), dict(stride=512)] + smaller:
        assert call(**bad) == INVALID, bad
    assert plan_render_packets(None, a, 1024, a, a, a, a, a, a, 4096, a, a, a, need, None) == INVALID
    if L.asciichat_hip_device_count() == 0:
        assert call() == NO_DEVICE
