"""The zhuf wire pass without a GPU: its four kernels under the CPU emulator against the restatement (tests/zhuf_ref.py) and
the oracle's CRC -- destination, offsets, sent lengths, headers, checksums and packet checksums byte for byte, nothing stored
outside the frames -- and what the product library decides before it needs a device."""
import pytest

import zhuf_ref as Z
import zpack_support as ZS
import zwire as ZW

CASES = ZS.small_cases()


@pytest.fixture(scope="module")
def mixed():
    frames = list(CASES.values())
    dims = ZS.dims_of(len(frames))
    out, cap = ZS.emu_run(frames, dims)
    return frames, dims, out, cap


def test_mixed_batch_equals_the_restatement(mixed):
    frames, dims, out, cap = mixed
    ZS.check(frames, dims, out, cap, "mixed")


def test_the_batch_takes_every_path(mixed):
    """the cases are what they claim: frames sent as they are and as zhuf frames, and RLE, raw and Huffman blocks among them"""
    frames, _, _, _ = mixed
    kinds = set()
    for name, f in CASES.items():
        if isinstance(f, int):
            continue
        payload, csz, flags = ZS.wire_of(f)
        z = Z.encode(f)
        kinds.add(("zhuf" if flags else "as is", (z[9] >> 1) & 3))
        if "as it is" in name or "raw" in name or len(f) <= 1024:
            assert flags == 0, name
        else:
            assert flags == Z.FLAG_COMPRESSED and csz == len(payload) < len(f), name
    assert {("zhuf", 1), ("zhuf", 2), ("as is", 0), ("as is", 2)} <= kinds


@pytest.mark.parametrize("short", [1, 16, 17, 700])
def test_tight_capacity(short):
    """a destination that ends inside / right behind a frame: that frame and the ones behind it stay out, nothing is stored
    at or behind the capacity, every result that does not live in dst is complete"""
    frames = [CASES[k] for k in ("1025 skewed", "error code", "one byte value (RLE)", "1024 skewed (as it is: the size floor)",
                                 "two byte values", "5 bytes")]
    dims = ZS.dims_of(len(frames))
    _, total = ZS.expect(frames, dims)
    out, cap = ZS.emu_run(frames, dims, capacity=total - short)
    ZS.check(frames, dims, out, cap, f"capacity -{short}")
    assert (out["dst"][cap:] == ZS.FILL).all()


def test_one_frame_alone_and_a_batch_of_equal_frames():
    f = CASES["truecolor 20x6"]
    out, cap = ZS.emu_run([f], [(20, 6)])
    ZS.check([f], [(20, 6)], out, cap, "alone")
    out, cap = ZS.emu_run([f] * 5, [(20, 6)] * 5)
    ZS.check([f] * 5, [(20, 6)] * 5, out, cap, "five equal")


def test_library_refuses_before_it_needs_a_device_and_needs_one_after():
    ZW.check_refusals(ZW.NARROW)



def test_frames_of_two_and_three_pieces():
    """131 073 bytes (the last piece one byte: an RLE block), 131 072 + 100 uniform bytes (a raw block inside a zhuf frame) and
    262 145 bytes: blocks behind the first start at three phases of a 16-byte group (every phase: test_zpack_boundaries.py),
    checksums combined over the pieces"""
    frames = [ZS.skewed(131073, 20), ZS.skewed(131072, 21) + ZS.uniform7(100, 22), ZS.skewed(262145, 23, spread=0.3)]
    for f in frames[:2]:
        assert ZS.wire_of(f)[2] == Z.FLAG_COMPRESSED
    dims = ZS.dims_of(3)
    out, cap = ZS.emu_run(frames, dims)
    ZS.check(frames, dims, out, cap, "pieces")
