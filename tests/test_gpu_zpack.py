"""The zhuf wire pass on the GPU through the C ABI: the batch of tests/zpack_support.py against the restatement byte for byte
(destination in device memory and in mapped host memory), every sent frame decoded back by tests/zhuf_ref.py's decoder and by
libzstd where it loads, headers as the reference's receiver checks them, two calls back to back on one stream, frames of two
and three pieces, plan_render_packets_zpacked over real renders, and every family of tests/zpack_cases.py -- the pass at
its block, stream and batch boundaries -- at the real piece size, a few batches per test.  Out of scope: offsets above 4 GB
(ZF_OFF_HI), which would have to move more than 4 GB, and lengths above max_len, which the caller promises."""
import functools
import os
import struct
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orc  # noqa: E402
import zhuf_ref as Z  # noqa: E402
import zpack_cases as ZC  # noqa: E402
import zpack_support as ZS  # noqa: E402
import zwire as ZW  # noqa: E402

CASES = ZS.small_cases()


@pytest.fixture(scope="module")
def pkg():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from __graft_entry__ import load_package

    p = load_package()
    assert torch.cuda.is_available() and p.lib().asciichat_hip_device_count() > 0
    return p


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


_Call = functools.partial(ZW.Call, ZW.NARROW)


@pytest.mark.parametrize("host", [False, True], ids=["device", "mapped host"])
def test_mixed_batch_equals_the_restatement(pkg, host):
    import torch
    frames = list(CASES.values())
    c = _Call(pkg, frames, ZS.dims_of(len(frames)), host=host)
    c.launch(_stream())
    torch.cuda.synchronize()
    c.check("mixed")


def test_tight_capacity(pkg):
    import torch
    frames = [CASES[k] for k in ("1025 skewed", "error code", "one byte value (RLE)", "1024 skewed (as it is: the size floor)",
                                 "two byte values", "5 bytes")]
    dims = ZS.dims_of(len(frames))
    _, total = ZS.expect(frames, dims)
    for short in (1, 17, 700):
        c = _Call(pkg, frames, dims, capacity=total - short)
        c.launch(_stream())
        torch.cuda.synchronize()
        c.check(f"capacity -{short}")


def test_two_calls_back_to_back_on_one_stream(pkg):
    """no host wait in between: each call has its own scratch and outputs, both complete"""
    import torch
    a = [CASES[k] for k in ("truecolor 20x6", "fibonacci counts (limiter and repair)", "error code", "all 129 symbols")]
    b = [CASES[k] for k in ("two byte values", "S = 128", "empty", "uniform below 0x80 (as it is: the ratio)", "1027 skewed")]
    ca, cb = _Call(pkg, a, ZS.dims_of(len(a))), _Call(pkg, b, ZS.dims_of(len(b)))
    s = _stream()
    ca.launch(s)
    cb.launch(s)
    torch.cuda.synchronize()
    ca.check("first call")
    cb.check("second call")


@pytest.mark.parametrize("n", [131073, 262145])
def test_large_pieces_once_each(pkg, n):
    """two and three pieces, the last one a single byte; next to it a frame whose second block is raw inside a zhuf frame"""
    import torch
    frames = [ZS.skewed(n, 20 + n % 7)]
    if n == 131073:
        frames.append(ZS.skewed(131072, 21) + ZS.uniform7(100, 22))
    c = _Call(pkg, frames, ZS.dims_of(len(frames)))
    c.launch(_stream())
    torch.cuda.synchronize()
    c.check(f"{n} bytes")


def test_a_full_size_truecolor_frame_in_256_copies(pkg):
    """80x24 truecolor cells (about 11 KB a frame, 256 workgroups in flight): one expectation, shared"""
    import torch
    f = ZS.ansi_truecolor(80, 24, 30)
    assert ZS.wire_of(f)[2] == Z.FLAG_COMPRESSED
    c = _Call(pkg, [f] * 256, [(80, 24)] * 256)
    c.launch(_stream())
    torch.cuda.synchronize()
    c.check("256 equal frames")


def _source(w, h, seed):
    img = orc.frame_smooth(w, h)
    img[h // 4:h // 2, w // 4:w // 2] = orc.frame_hash_noise(w // 2 - w // 4, h // 2 - h // 4, seed)
    return img


@pytest.mark.parametrize("mode,caps,n", [(1, (3, 0), 12), (5, (3, 2), 4)], ids=["truecolor fg x12", "half-block x4"])
def test_plan_render_packets_zpacked(pkg, mode, caps, n):
    """12 frames of 160x90 -> 80x24 truecolor compress (sent < original is all that is asked of the ratio); 4 half-block
    frames hold bytes above 0x80 and go out as they are, flags 0.  Either way the payload decodes to the oracle's frame."""
    import torch
    cl, rm = caps
    imgs = [_source(160, 90, 40 + i) for i in range(n)]
    dev = torch.from_numpy(np.stack(imgs)).cuda()
    fs = [pkg.frame_setup(dev.data_ptr() + i * 160 * 90 * 3, 160, 90, 80, 24, rm, False, False, False) for i in range(n)]
    plan = pkg.Plan(mode, orc.PALETTE_STANDARD, fs)
    stride = plan.stride
    slab = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    cap = n * stride
    host = pkg.HostBuffer(cap)
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    len_out = torch.zeros(n, dtype=torch.int32, device="cuda")
    crc = torch.zeros(n, dtype=torch.int32, device="cuda")
    pkt = torch.zeros(n, dtype=torch.int32, device="cuda")
    hdr = torch.zeros(24 * n, dtype=torch.uint8, device="cuda")
    d = torch.from_numpy(np.array([(80, 24)] * n, dtype=np.uint32).view(np.int32)).cuda()
    sbytes = pkg.zpack_scratch_bytes(stride, n)
    scratch = torch.zeros(sbytes // 8 + 1, dtype=torch.int64, device="cuda")
    plan.render_packets_zpacked(slab.data_ptr(), stride, ln.data_ptr(), d.data_ptr(), crc.data_ptr(), hdr.data_ptr(), pkt.data_ptr(),
                                host.dev, cap, off.data_ptr(), len_out.data_ptr(), scratch.data_ptr(), sbytes, _stream())
    torch.cuda.synchronize()
    dst = host.view().copy()
    offs, sent, orig = off.cpu().numpy(), len_out.cpu().numpy().view(np.uint32), ln.cpu().numpy().view(np.uint32)
    hdrs, pkts = hdr.cpu().numpy(), pkt.cpu().numpy().view(np.uint32)
    at = 0
    for i in range(n):
        exp = orc.convert_with_caps(imgs[i], 80, 24, cl, rm, False, False, False)
        assert int(orig[i]) == len(exp) and int(offs[i]) == at
        payload = dst[at:at + int(sent[i])].tobytes()
        w_, h_, osz, csz, cks, flags = struct.unpack(">6I", hdrs[24 * i:24 * i + 24].tobytes())
        assert (w_, h_, osz, cks) == (80, 24, len(exp), orc.crc32c(exp))
        assert int(pkts[i]) == orc.crc32c(hdrs[24 * i:24 * i + 24].tobytes() + payload)
        if mode == 1:
            assert int(sent[i]) < len(exp) and flags == Z.FLAG_COMPRESSED and csz == int(sent[i])
            assert payload == ZS.wire_of(exp)[0] and Z.decode(payload) == exp
            if Z.libzstd() is not None:
                assert Z.zstd_decompress(payload, len(exp)) == exp
        else:
            assert flags == 0 and csz == 0 and payload == exp
        at += (int(sent[i]) + 15) // 16 * 16
    assert int(offs[n]) == at
    plan.close()
    host.close()


# ---- the boundaries of tests/zpack_cases.py ----------------------------------------------------------------------------
def _once(pkg, frames, what, **kw):
    import torch
    c = _Call(pkg, frames, ZS.dims_of(len(frames)), **kw)
    c.launch(_stream())
    torch.cuda.synchronize()
    return c.check(what)


def test_tail_lengths_gains_and_symbols_behind_a_full_piece(pkg):
    """(a), (b), (c): one batch of carrier + tail frames, the carrier's block coded and decoded once"""
    named = ZC.tail_lengths(Z.PIECE) + ZC.tail_lengths_long() + ZC.tail_gain(Z.PIECE) + ZC.tail_symbols(Z.PIECE)
    _once(pkg, [f for _, f in named], "tails")


@pytest.mark.parametrize("host", [False, True], ids=["device", "mapped host"])
def test_tail_blocks_at_every_phase(pkg, host):
    """(d): a Huffman block at each of the 16 phases of a group, raw and RLE blocks at 0 / 1 / 8 / 15, three pieces"""
    _once(pkg, [f for _, f in ZC.tail_phases(Z.PIECE)], "phases", host=host)


def test_ratio_stream_cuts_and_lane_shares(pkg):
    """(e), (f), (g) in one batch of 235 frames"""
    named = ZC.ratio_frames() + ZC.stream_cut_frames() + ZC.chunk_step_frames()
    _once(pkg, [f for _, f in named], "whole frames")


def test_histogram_frames_and_the_table_in_the_scratch_records(pkg):
    """(h): the payloads, and the table the measure kernel left"""
    hists = ZC.histograms()
    rec = _once(pkg, [f for _, _, f in hists], "histograms")
    for i, (name, hist, _) in enumerate(hists):
        lens = Z.code_lengths(hist)
        codes, max_bits = Z.canonical_codes(lens)
        table, dev_bits = ZS.device_table(rec, i)
        assert dev_bits == max_bits, (name, dev_bits, max_bits)
        assert table == [c | (d << 16) if d else 0 for c, d in zip(codes, lens)], name


@pytest.mark.parametrize("host", [False, True], ids=["device", "mapped host"])
def test_more_frames_than_threads_of_the_plan(pkg, host):
    """(i): 257 and 600 short frames, then 600 with a capacity that ends inside a frame of index >= 256"""
    for n in (257, 600):
        _once(pkg, ZC.short_batch(n), f"{n} frames", host=host)
    frames = ZC.short_batch(600)
    i, tight = ZC.capacity_inside(frames, ZS.dims_of(600), 256, ZS.expect)
    assert i >= 256
    _once(pkg, frames, f"600 frames, capacity inside frame {i}", host=host, capacity=tight)


@pytest.mark.parametrize("host", [False, True], ids=["device", "mapped host"])
def test_short_frames_among_frames_of_whole_pieces(pkg, host):
    """(i): an empty frame, an error code and 5 bytes in front of frames of 1, 2 and 3 pieces; capacities that end inside
    the first and the second block of the first frame of several pieces; a stride 48 bytes wider; one piece alone"""
    frames = ZC.piece_batch(Z.PIECE)
    dims = ZS.dims_of(len(frames))
    _once(pkg, frames, "whole pieces", host=host)
    for tight in ZC.piece_batch_capacities(frames, dims, ZS.expect, Z.PIECE):
        _once(pkg, frames, f"capacity {tight}", host=host, capacity=tight)
    _once(pkg, frames, "stride + 48", host=host, stride=ZS.slab_of(frames)[1] + 48)
    _once(pkg, [frames[3]], "one piece alone", host=host)
