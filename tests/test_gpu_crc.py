"""The stand-alone checksum wire pass on the GPU through the C ABI, at its group, round and span boundaries: every family of
tests/crc_cases.py through asciichat_hip_frame_packets (with and without dims, headers only), asciichat_hip_crc32c (length
words and a fixed length), the one-launch form of achip_launch_crc32c on the caller's arrival counters, the COPY forms
(asciichat_hip_frame_packets_packed), achip_launch_crc32c_at over their output and asciichat_hip_packets_from_crc -- every
element of every output array against the bitwise oracle (tests/crc_ref.py), outputs prefilled with sentinels.

The launcher is steered through max_len and n alone; each batch first asserts with achip_crc_parts that it takes the path its
family is named for, so a change of the cost model fails here instead of moving the cases to another kernel.  The real DPP
reductions, readlane, agent-scope atomics and LDS table images are checked only here: under the emulator they are stand-ins."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crc_cases as CC  # noqa: E402
import crc_ref as R  # noqa: E402
import orc  # noqa: E402

vp, u32, u64, ci, sz = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_size_t


@pytest.fixture(scope="module")
def gpu():
    if os.environ.get("ASCIICHAT_HIP_CRC_FRAME_MAX") or os.environ.get("ASCIICHAT_HIP_CRC_SMALL_SPANS"):
        pytest.skip("ASCIICHAT_HIP_CRC_FRAME_MAX / ASCIICHAT_HIP_CRC_SMALL_SPANS is set: the launcher's choice is overridden")
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from __graft_entry__ import load_package

    p = load_package()
    L = p.lib()
    assert torch.cuda.is_available() and L.asciichat_hip_device_count() > 0
    torch.cuda.set_device(0)
    L.achip_crc_parts.restype = ci
    L.achip_crc_parts.argtypes = [u32, ci]
    L.achip_launch_crc32c.restype = ci
    L.achip_launch_crc32c.argtypes = [vp, u64, vp, u32, u32, ci, vp, vp, vp, vp, vp, vp, vp]
    L.achip_launch_crc32c_at.restype = ci
    L.achip_launch_crc32c_at.argtypes = [vp, vp, vp, u32, ci, vp, vp, vp, vp, vp, vp, vp]
    return p


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


class _Call:
    """the device side of one batch: slab, length words, dims, and output arrays prefilled with sentinels"""

    def __init__(self, gpu, b, slack_seed=0):
        self.L, self.b = gpu.lib(), b
        assert self.L.achip_crc_parts(b.max_len, b.n) == b.parts, (b, "the launcher takes another path than the family names")
        self.slab_host = b.slab(slack_seed)
        self.slab, self.len, self.dims = _dev(self.slab_host), _dev(b.len_words()), _dev(b.dim_words())
        assert self.slab.data_ptr() % 16 == 0
        self.fresh()

    def fresh(self):
        n = self.b.n
        self.crc = _dev(np.full(n, R.SENTINEL_WORD, dtype=np.uint32))
        self.pkt = _dev(np.full(n, R.SENTINEL_WORD, dtype=np.uint32))
        self.hdr = _dev(np.full(24 * n, R.SENTINEL_BYTE, dtype=np.uint8))

    def outputs(self, hdr=True, pkt=True):
        import torch
        torch.cuda.synchronize()
        return (_host(self.crc, np.uint32), self.hdr.cpu().numpy() if hdr else None, _host(self.pkt, np.uint32) if pkt else None)

    def check(self, what, hdr=True, pkt=True, with_dims=True):
        out = self.outputs(hdr, pkt)
        R.check_outputs(self.b.expect(), self.b.lens, *out, with_dims=with_dims, what=f"{self.b.name} {what}")
        if not hdr:
            assert (self.hdr.cpu().numpy() == R.SENTINEL_BYTE).all()
        if not pkt:
            assert (_host(self.pkt, np.uint32) == R.SENTINEL_WORD).all()
        return out

    def frame_packets(self, with_dims=True, pkt=True):
        self.fresh()
        b = self.b
        rc = self.L.asciichat_hip_frame_packets(self.slab.data_ptr(), b.stride, self.len.data_ptr(), b.max_len, b.n,
                                                self.dims.data_ptr() if with_dims else None, self.crc.data_ptr(),
                                                self.hdr.data_ptr(), self.pkt.data_ptr() if pkt else None, _stream())
        assert rc == 0, (b, rc)
        return self.check("frame_packets" + ("" if with_dims else ", no dims") + ("" if pkt else ", headers only"), pkt=pkt,
                          with_dims=with_dims)

    def crc32c(self):
        self.fresh()
        b = self.b
        rc = self.L.asciichat_hip_crc32c(self.slab.data_ptr(), b.stride, self.len.data_ptr(), 0, b.max_len, b.n, self.crc.data_ptr(),
                                         _stream())
        assert rc == 0, (b, rc)
        return self.check("crc32c", hdr=False, pkt=False)

    def crc32c_fixed(self, fixed):
        self.fresh()
        b = self.b
        assert fixed <= b.max_len
        rc = self.L.asciichat_hip_crc32c(self.slab.data_ptr(), b.stride, None, fixed, b.max_len, b.n, self.crc.data_ptr(), _stream())
        assert rc == 0, (b, rc)
        s = self.slab_host
        want = np.array([orc.crc32c(s[i * b.stride:i * b.stride + fixed].tobytes()) for i in range(b.n)], dtype=np.uint32)
        assert np.array_equal(self.outputs(False, False)[0], want), (b, fixed)

    def all_variants(self):
        self.frame_packets()
        self.frame_packets(with_dims=False)
        self.frame_packets(pkt=False)
        self.crc32c()


# ---- the one-workgroup kernel ------------------------------------------------------------------------------------------------
def test_frame_tails_and_slack_independence(gpu):
    """(a): 207 lengths; the same outputs with every slack byte regenerated (bytes behind the end count as zeros, and so do
    the zero groups in front)"""
    b = CC.frame_tails()
    c = _Call(gpu, b)
    first = c.frame_packets()
    c.frame_packets(with_dims=False)
    c.frame_packets(pkt=False)
    c.crc32c()
    again = _Call(gpu, b, slack_seed=1)
    assert not np.array_equal(again.slab_host, c.slab_host)
    assert all(np.array_equal(x, y) for x, y in zip(first, again.frame_packets()))


def test_frame_content(gpu):
    """(b)"""
    _Call(gpu, CC.frame_content()).all_variants()


def test_error_codes_and_empty_frames(gpu):
    """(c): CRC 0, zero dimensions, length 0 and packet CRC 0 behind an error code, wherever it stands in the batch"""
    for b in CC.error_and_empty():
        _Call(gpu, b).all_variants()


def test_long_frames_in_one_workgroup(gpu):
    """(d)"""
    _Call(gpu, CC.long_frames()).all_variants()


# ---- spans -------------------------------------------------------------------------------------------------------------------
def test_span_edges_and_slack_independence(gpu):
    """(e)"""
    for b in CC.span_edges():
        c = _Call(gpu, b)
        c.frame_packets()
        c.crc32c()
    b = CC.span_edges()[5]
    c = _Call(gpu, b)
    first = c.frame_packets()
    c.frame_packets(with_dims=False)
    c.frame_packets(pkt=False)
    again = _Call(gpu, b, slack_seed=1)
    assert not np.array_equal(again.slab_host, c.slab_host)
    assert all(np.array_equal(x, y) for x, y in zip(first, again.frame_packets()))


def test_span_batches(gpu):
    """(f): 63, 64, 65, 128 and 129 registers a frame"""
    for b in CC.span_batches():
        _Call(gpu, b).frame_packets()
    _Call(gpu, CC.span_batches()[2]).all_variants()


def test_wide_spans(gpu):
    """(g)"""
    _Call(gpu, CC.wide_spans()).all_variants()


def test_len_bits(gpu):
    """(h): 1029 spans of 16 KB for the lone frame, 258 of 64 KB with a short frame next to it"""
    for b in CC.len_bits():
        c = _Call(gpu, b)
        c.frame_packets()
        c.crc32c()


def test_a_fixed_length_without_length_words(gpu):
    """len_dev == NULL once per path: every slot's first fixed_len bytes, slack and all"""
    for b, fixed in ((CC.error_and_empty()[0], 19999), (CC.long_frames(), 196601), (CC.span_edges()[0], 180229),
                     (CC.wide_spans(), 65537)):
        _Call(gpu, b).crc32c_fixed(fixed)


def _launch_direct(c, partial, counters):
    c.fresh()
    b = c.b
    rc = c.L.achip_launch_crc32c(c.slab.data_ptr(), b.stride, c.len.data_ptr(), 0, b.max_len, b.n, partial.data_ptr(),
                                 counters.data_ptr() if counters is not None else None, c.dims.data_ptr(), c.crc.data_ptr(),
                                 c.hdr.data_ptr(), c.pkt.data_ptr(), _stream())
    assert rc == 0, (b, rc)
    return c.check("achip_launch_crc32c" + (" on counters" if counters is not None else ""))


def test_one_launch_form_on_the_callers_counters(gpu):
    """the last span of a frame to arrive finishes it and re-arms the counter: results as the two-launch call's, counters
    zero afterwards, and a second launch on them with other data right too.  At 65 and 129 registers (n * parts > 128)
    the launcher drops the counters: results only."""
    e, f, g = CC.span_edges(), CC.span_batches(), CC.span_batches_swapped()
    for first, second in ((e[5], e[9]), (e[10], e[0]), (f[0], g[0]), (f[1], g[1]), (f[3], f[4])):
        assert first.n == second.n and first.parts == second.parts and first.n * first.parts <= 128
        partial = _dev(np.full(first.n * first.parts, R.SENTINEL_WORD, dtype=np.uint32))
        counters = _dev(np.zeros(first.n, dtype=np.uint32))
        for b in (first, second):
            c = _Call(gpu, b)
            two = c.frame_packets()
            one = _launch_direct(c, partial, counters)
            assert all(np.array_equal(x, y) for x, y in zip(one, two)), b
            assert not _host(counters, np.uint32).any(), (b, _host(counters, np.uint32))
    for b in (f[2], f[6]):
        assert b.n * b.parts > 128
        partial = _dev(np.full(b.n * b.parts, R.SENTINEL_WORD, dtype=np.uint32))
        counters = _dev(np.zeros(b.n, dtype=np.uint32))
        _launch_direct(_Call(gpu, b), partial, counters)


# ---- (j) ---------------------------------------------------------------------------------------------------------------------
def _packed(gpu, b):
    import torch
    c = _Call(gpu, b)
    plain = c.frame_packets()
    off_ref, _ = b.packed()
    total = off_ref[b.n]
    for name, cap in CC.pack_capacities(b):
        c.fresh()
        dst = torch.full((total + 64,), R.SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
        off = _dev(np.full(b.n + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64))
        lo = _dev(np.full(b.n, R.SENTINEL_WORD, dtype=np.uint32))
        rc = c.L.asciichat_hip_frame_packets_packed(c.slab.data_ptr(), b.stride, c.len.data_ptr(), b.max_len, b.n, c.dims.data_ptr(),
                                                    c.crc.data_ptr(), c.hdr.data_ptr(), c.pkt.data_ptr(), dst.data_ptr(), cap,
                                                    off.data_ptr(), lo.data_ptr(), _stream())
        assert rc == 0, (b, name, rc)
        what = f"packed, capacity {name} = {cap}"
        got = c.check(what)
        assert all(np.array_equal(x, y) for x, y in zip(got, plain)), (b, what)
        R.check_packed(c.slab_host, b.stride, b.lens, cap, _host(off, np.uint64), _host(lo, np.uint32), dst.cpu().numpy(),
                       what=f"{b.name} {what}")
        if name != "total":
            continue
        # the frames where the COPY form left them: achip_launch_crc32c_at on its offsets, garbage ones behind error codes
        at = np.array(off_ref[:b.n], dtype=np.uint64)
        for i, l in enumerate(b.lens):
            if l >= R.ERR_FROM:
                at[i] = (total // 2) | 7
        at_dev = _dev(at)
        partial = _dev(np.full(b.n * b.parts, R.SENTINEL_WORD, dtype=np.uint32))
        c.fresh()
        rc = c.L.achip_launch_crc32c_at(dst.data_ptr(), at_dev.data_ptr(), c.len.data_ptr(), b.max_len, b.n, partial.data_ptr(), None,
                                        c.dims.data_ptr(), c.crc.data_ptr(), c.hdr.data_ptr(), c.pkt.data_ptr(), _stream())
        assert rc == 0, (b, rc)
        got = c.check("at the packed offsets")
        assert all(np.array_equal(x, y) for x, y in zip(got, plain)), (b, "at")


def test_pack_edges_in_one_workgroup(gpu):
    for b in (CC.frame_tails(2),) + CC.error_and_empty():
        _packed(gpu, b)


def test_pack_edges_in_spans(gpu):
    for b in CC.span_edges():
        _packed(gpu, b)


def test_pack_offsets_of_more_frames_than_threads(gpu):
    """1100 frames: the offset prefix walks the 1024 threads of a workgroup more than once"""
    _packed(gpu, CC.short_pack_batch())


# ---- (i) ---------------------------------------------------------------------------------------------------------------------
def test_packets_from_known_checksums(gpu):
    """crc_packets_kernel beyond one block and at lengths of 2^24 and above: headers byte for byte, packet CRCs against
    crc_ref.packet_crc_from_frame_crc"""
    import torch
    L = gpu.lib()
    for case in CC.packets_only():
        n, lens, crcs, dims = case
        for d in (dims, None):
            want_hdr, want_pkt = CC.packets_expect(case if d is not None else (n, lens, crcs, np.zeros_like(dims)))
            hdr = _dev(np.full(24 * n, R.SENTINEL_BYTE, dtype=np.uint8))
            pkt = _dev(np.full(n, R.SENTINEL_WORD, dtype=np.uint32))
            ln, cr = _dev(lens), _dev(crcs)
            dd = _dev(d) if d is not None else None
            rc = L.asciichat_hip_packets_from_crc(ln.data_ptr(), cr.data_ptr(), n, dd.data_ptr() if dd is not None else None,
                                                  hdr.data_ptr(), pkt.data_ptr(), _stream())
            assert rc == 0
            torch.cuda.synchronize()
            assert np.array_equal(hdr.cpu().numpy(), want_hdr), n
            got = _host(pkt, np.uint32)
            assert np.array_equal(got, want_pkt), (n, np.flatnonzero(got != want_pkt)[:4])
