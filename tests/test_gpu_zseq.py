"""The zseq wire form on the GPU through the C ABI: the boundary families of tests/zseq_cases.py in one mixed batch against the
restatement (tests/zseq_ref.py) byte for byte, destination in device memory and in mapped host memory, every sent frame decoded
back by the subset decoder and by libzstd where it loads, headers as the reference's receiver checks them; tight capacities,
two calls back to back on one stream, a stride wider than the longest frame, 257 small frames, and
plan_render_packets_zpacked_seq over real renders."""
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
import zseq_cases as SC  # noqa: E402
import zseq_ref as S  # noqa: E402
import zwire as ZW  # noqa: E402

CASES = SC.cases()


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


_Call = functools.partial(ZW.Call, ZW.SEQ)


@pytest.mark.parametrize("host", [False, True], ids=["device", "mapped host"])
def test_mixed_batch_equals_the_restatement(pkg, host):
    import torch
    frames = list(CASES.values())
    c = _Call(pkg, frames, ZS.dims_of(len(frames)), host=host)
    c.launch(_stream())
    torch.cuda.synchronize()
    c.check("mixed")


def test_tight_capacity(pkg):
    """capacities that end in the last frame, in a frame sent as it is and inside a block of a frame of three"""
    import torch
    frames = [CASES[k] for k in ("exactly 3 blocks", "error code", "one byte value (RLE)", "1024 bytes (as it is: the size floor)",
                                 "half-block truecolor 20x6", "empty", "127 sequences")]
    dims = ZS.dims_of(len(frames))
    exp, total = SC.expect(frames, dims)
    second = Z.blocks(exp[0]["payload"])[1][2]
    for cap in (total - 1, total - 17, total - 700, exp[3]["off"] + 512, second + 40):
        c = _Call(pkg, frames, dims, capacity=cap)
        c.launch(_stream())
        torch.cuda.synchronize()
        c.check(f"capacity {cap}")


def test_two_calls_back_to_back_on_one_stream(pkg):
    """no host wait in between: each call has its own scratch and outputs, both complete"""
    import torch
    a = [CASES[k] for k in ("half-block truecolor 20x6", "a match back over the block cut", "error code", "128 sequences")]
    b = [CASES[k] for k in ("a block without literals", "match of 300", "empty", "uniform bytes (as it is)", "4096 literals")]
    ca, cb = _Call(pkg, a, ZS.dims_of(len(a))), _Call(pkg, b, ZS.dims_of(len(b)))
    s = _stream()
    ca.launch(s)
    cb.launch(s)
    torch.cuda.synchronize()
    ca.check("first call")
    cb.check("second call")


def test_a_stride_wider_than_the_longest_frame(pkg):
    import torch
    frames = [CASES[k] for k in ("exactly 2 blocks", "period 64", "empty", "a match cut to 4 by the block's end, no tail literals")]
    c = _Call(pkg, frames, ZS.dims_of(len(frames)), stride=3 * S.PIECE + 48)
    c.launch(_stream())
    torch.cuda.synchronize()
    c.check("wide stride")


def test_more_frames_than_threads_of_the_plan(pkg):
    """257 small frames, coded and not, with error codes and empty frames among them"""
    import torch
    pool = [CASES[k] for k in ("utf-8 palette truecolor 20x6 (FSE tree)", "error code", "a match at position 6 of the frame", "empty",
                               "1024 bytes (as it is: the size floor)", "truecolor 20x6 (direct tree)", "one byte value (RLE)")]
    frames = [pool[i % len(pool)] for i in range(257)]
    c = _Call(pkg, frames, ZS.dims_of(257))
    c.launch(_stream())
    torch.cuda.synchronize()
    c.check("257 frames")


def _source(w, h, seed):
    img = orc.frame_smooth(w, h)
    img[h // 4:h // 2, w // 4:w // 2] = orc.frame_hash_noise(w // 2 - w // 4, h // 2 - h // 4, seed)
    return img


@pytest.mark.parametrize("mode,rm,palette,sizes", [(1, 0, orc.PALETTE_STANDARD, [(20, 6), (80, 24)]), (5, 2, orc.PALETTE_STANDARD, [(20, 6), (80, 24)]),
                                                   (2, 0, orc.PALETTE_STANDARD, [(80, 24)]), (0, 0, orc.PALETTE_STANDARD, [(80, 24)]),
                                                   (0, 0, orc.PALETTE_BLOCKS, [(80, 24)]), (1, 0, orc.PALETTE_BLOCKS, [(20, 6)])],
                         ids=["truecolor fg", "half-block truecolor", "ANSI-256", "mono", "mono BLOCKS palette", "truecolor BLOCKS palette"])
def test_plan_render_packets_zpacked_seq(pkg, mode, rm, palette, sizes):
    """real renders from 32x16 sources: every payload is the restatement's and, where it travels compressed, decodes (subset
    decoder, libzstd) to the bytes a plain plan_render leaves; headers as the reference's receiver checks them"""
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
    sbytes = pkg.zpack_seq_scratch_bytes(stride, n)
    scratch = torch.zeros(sbytes // 8 + 1, dtype=torch.int64, device="cuda")
    plan.render_packets_zpacked_seq(slab.data_ptr(), stride, ln.data_ptr(), d.data_ptr(), crc.data_ptr(), hdr.data_ptr(), pkt.data_ptr(),
                                    host.dev, cap, off.data_ptr(), len_out.data_ptr(), scratch.data_ptr(), sbytes, _stream())
    torch.cuda.synchronize()
    dst = host.view().copy()
    offs, sent, orig = off.cpu().numpy(), len_out.cpu().numpy().view(np.uint32), ln.cpu().numpy().view(np.uint32)
    hdrs, pkts = hdr.cpu().numpy(), pkt.cpu().numpy().view(np.uint32)
    plain_host, plain_lens = plain.cpu().numpy(), plain_len.cpu().numpy().view(np.uint32)
    at, compressed = 0, 0
    for i, (w, h) in enumerate(sizes):
        exp = plain_host[i * stride:i * stride + int(plain_lens[i])].tobytes()
        assert int(orig[i]) == len(exp) and int(offs[i]) == at
        payload = dst[at:at + int(sent[i])].tobytes()
        w_, h_, osz, csz, cks, flags = struct.unpack(">6I", hdrs[24 * i:24 * i + 24].tobytes())
        assert (w_, h_, osz, cks) == (w, h, len(exp), orc.crc32c(exp))
        assert int(pkts[i]) == orc.crc32c(hdrs[24 * i:24 * i + 24].tobytes() + payload)
        want, want_csz, want_flags = S.wire(exp)
        assert payload == want and (csz, flags) == (want_csz, want_flags)
        if flags:
            compressed += 1
            assert csz == int(sent[i]) and 5 * csz < 4 * len(exp)
            assert S.decode(payload) == exp
            if Z.libzstd() is not None:
                assert Z.zstd_decompress(payload, len(exp)) == exp
        else:
            assert payload == exp
        at += (int(sent[i]) + 15) // 16 * 16
    assert int(offs[n]) == at
    assert compressed > 0 or mode == 0, "a colour render above the size floor travels compressed"
    plan.close()
    host.close()
