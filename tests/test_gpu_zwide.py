"""The wide zhuf form on the GPU through the C ABI: the batch of tests/zwide_support.py against the restatement
(tests/zwide_ref.py) byte for byte, destination in device memory and in mapped host memory, every sent frame decoded back by
the subset decoder and by libzstd where it loads, headers as the reference's receiver checks them; tight capacities, two
calls back to back on one stream, 257 small frames, a half-block frame of two full pieces and six bytes, the narrow and the
wide call over the narrow form's cases, and plan_render_packets_zpacked_wide over real renders."""
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
import zpack_support as ZS  # noqa: E402
import zwide_ref as W  # noqa: E402
import zwide_support as WS  # noqa: E402
import zwire as ZW  # noqa: E402

CASES = WS.wide_cases()


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


_Call = functools.partial(ZW.Call, ZW.WIDE)


@pytest.mark.parametrize("host", [False, True], ids=["device", "mapped host"])
def test_mixed_batch_equals_the_restatement(pkg, host):
    import torch
    frames = list(CASES.values())
    c = _Call(pkg, frames, ZS.dims_of(len(frames)), host=host)
    c.launch(_stream())
    torch.cuda.synchronize()
    out = c.check("mixed")
    assert WS.check_records(frames, out) >= 20  # the tables and the trees measure left


def test_tight_capacity(pkg):
    import torch
    frames = [CASES[k] for k in ("top 129 (odd count of weights)", "error code", "one byte value above 0x80 (RLE)",
                                 "half blocks below the size floor (as it is)", "half-block truecolor 20x6", "empty")]
    dims = ZS.dims_of(len(frames))
    _, total = WS.expect(frames, dims)
    for short in (1, 17, 700):
        c = _Call(pkg, frames, dims, capacity=total - short)
        c.launch(_stream())
        torch.cuda.synchronize()
        c.check(f"capacity -{short}")


def test_two_calls_back_to_back_on_one_stream(pkg):
    """no host wait in between: each call has its own scratch and outputs, both complete"""
    import torch
    a = [CASES[k] for k in ("half-block truecolor 20x6", "top 255", "error code", "all 256 symbols skewed")]
    b = [CASES[k] for k in ("two symbols, one above 0x80", "top 128 (direct form)", "empty", "uniform bytes (raw by size)", "csize 1024")]
    ca, cb = _Call(pkg, a, ZS.dims_of(len(a))), _Call(pkg, b, ZS.dims_of(len(b)))
    s = _stream()
    ca.launch(s)
    cb.launch(s)
    torch.cuda.synchronize()
    ca.check("first call")
    cb.check("second call")


def test_more_frames_than_threads_of_the_plan(pkg):
    """257 small frames, coded and not, with error codes and empty frames among them"""
    import torch
    pool = [CASES[k] for k in ("utf-8 palette truecolor 20x6", "error code", "zero run of 3 weight values", "empty",
                               "half blocks below the size floor (as it is)", "top 130 (even count)", "one byte value above 0x80 (RLE)")]
    frames = [pool[i % len(pool)] for i in range(257)]
    c = _Call(pkg, frames, ZS.dims_of(257))
    c.launch(_stream())
    torch.cuda.synchronize()
    c.check("257 frames")


def test_a_half_block_frame_of_two_full_pieces_and_six_bytes(pkg):
    """the real piece size: three blocks, the last one raw (six bytes), checksums combined over the pieces"""
    import torch
    cell = WS.halfblock_truecolor(40, 12, 21)
    f = (cell * (2 * W.PIECE // len(cell) + 1))[:2 * W.PIECE] + WS.HALF * 2
    assert len(f) == 2 * W.PIECE + 6 and [k for k, _, _ in Z.blocks(W.encode(f))] == [2, 2, 0] and WS.wire_of(f)[2] == Z.FLAG_COMPRESSED
    c = _Call(pkg, [f], [(400, 120)])
    c.launch(_stream())
    torch.cuda.synchronize()
    c.check("two pieces + 6")


def test_narrow_and_wide_calls_agree_on_the_narrow_cases(pkg):
    """zpack_support.small_cases() without its one frame that holds a byte above 0x80: identical outputs"""
    import torch
    frames = [f for f in ZS.small_cases().values() if isinstance(f, int) or not f or max(f) <= 0x80]
    dims = ZS.dims_of(len(frames))
    cn, cw = ZW.Call(ZW.NARROW, pkg, frames, dims), _Call(pkg, frames, dims)
    cn.launch(_stream())
    cw.launch(_stream())
    torch.cuda.synchronize()
    n, w = cn.check("narrow call"), cw.out()
    for k in ("dst", "off", "len_out", "crc", "hdr", "pkt"):
        assert np.array_equal(n[k], w[k]), k


def _source(w, h, seed):
    img = orc.frame_smooth(w, h)
    img[h // 4:h // 2, w // 4:w // 2] = orc.frame_hash_noise(w // 2 - w // 4, h // 2 - h // 4, seed)
    return img


@pytest.mark.parametrize("mode,rm,palette,sizes", [(5, 2, orc.PALETTE_STANDARD, [(20, 6), (20, 6)]), (5, 2, orc.PALETTE_STANDARD, [(80, 24)]),
                                                   (1, 0, orc.PALETTE_BLOCKS, [(20, 6)])],
                         ids=["half blocks 20x6 x2", "half blocks 80x24", "BLOCKS palette 20x6"])
def test_plan_render_packets_zpacked_wide(pkg, mode, rm, palette, sizes):
    """real renders from 32x16 sources: every payload is the restatement's, decodes (subset decoder, libzstd) to the bytes a
    plain plan_render leaves, and travels compressed; headers as the reference's receiver checks them"""
    import torch
    n = len(sizes)
    imgs = [_source(32, 16, 60 + i) for i in range(n)]
    dev = torch.from_numpy(np.stack(imgs)).cuda()
    fs = [pkg.frame_setup(dev.data_ptr() + i * 32 * 16 * 3, 32, 16, w, h, rm, False, False, False) for i, (w, h) in enumerate(sizes)]
    plan = pkg.Plan(mode, palette, fs)
    stride = plan.stride
    plain = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    plain_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    plan.render(plain.data_ptr(), stride, plain_len.data_ptr(), _stream())
    slab = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    cap = n * stride
    host = pkg.HostBuffer(cap)
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    len_out = torch.zeros(n, dtype=torch.int32, device="cuda")
    crc = torch.zeros(n, dtype=torch.int32, device="cuda")
    pkt = torch.zeros(n, dtype=torch.int32, device="cuda")
    hdr = torch.zeros(24 * n, dtype=torch.uint8, device="cuda")
    d = torch.from_numpy(np.array(sizes, dtype=np.uint32).view(np.int32)).cuda()
    sbytes = pkg.zpack_wide_scratch_bytes(stride, n)
    scratch = torch.zeros(sbytes // 8 + 1, dtype=torch.int64, device="cuda")
    plan.render_packets_zpacked_wide(slab.data_ptr(), stride, ln.data_ptr(), d.data_ptr(), crc.data_ptr(), hdr.data_ptr(), pkt.data_ptr(),
                                     host.dev, cap, off.data_ptr(), len_out.data_ptr(), scratch.data_ptr(), sbytes, _stream())
    torch.cuda.synchronize()
    dst = host.view().copy()
    offs, sent, orig = off.cpu().numpy(), len_out.cpu().numpy().view(np.uint32), ln.cpu().numpy().view(np.uint32)
    hdrs, pkts = hdr.cpu().numpy(), pkt.cpu().numpy().view(np.uint32)
    plain_host, plain_lens = plain.cpu().numpy(), plain_len.cpu().numpy().view(np.uint32)
    at = 0
    for i, (w, h) in enumerate(sizes):
        exp = plain_host[i * stride:i * stride + int(plain_lens[i])].tobytes()
        assert max(exp) > 0x80 and len(exp) > 1024
        assert int(orig[i]) == len(exp) and int(offs[i]) == at
        payload = dst[at:at + int(sent[i])].tobytes()
        w_, h_, osz, csz, cks, flags = struct.unpack(">6I", hdrs[24 * i:24 * i + 24].tobytes())
        assert (w_, h_, osz, cks) == (w, h, len(exp), orc.crc32c(exp))
        assert int(pkts[i]) == orc.crc32c(hdrs[24 * i:24 * i + 24].tobytes() + payload)
        assert payload == WS.wire_of(exp)[0]
        assert flags == Z.FLAG_COMPRESSED and csz == int(sent[i]) and 5 * csz < 4 * len(exp)
        assert W.decode(payload) == exp
        if Z.libzstd() is not None:
            assert Z.zstd_decompress(payload, len(exp)) == exp
        at += (int(sent[i]) + 15) // 16 * 16
    assert int(offs[n]) == at
    plan.close()
    host.close()
