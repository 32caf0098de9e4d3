"""The shared checker of the three compressed wire forms (tests/zwire.py: check) still bites: per form one small emulated batch
-- a frame sent compressed, one sent as it is, an error code, an empty frame -- passes as the kernels leave it and fails with
any one field of it corrupted."""
import copy

import pytest

import zhuf_ref as Z
import zpack_support as ZS
import zseq_cases as SC
import zwide_support as WS
import zwire as ZW

CODED, AS_IS, ERROR, EMPTY = range(4)
FRAMES = {ZW.NARROW: ZS.skewed(1500, 1), ZW.WIDE: WS.skewed_high(1503, 2, top=0xE2, symbols=40), ZW.SEQ: SC.text(1500, 3)}
_runs = {}


def _run(form):
    """-> (frames, dims, out, capacity, expectation) of the form's batch, emulated once"""
    if form not in _runs:
        frames = [FRAMES[form], SC.rnd(1100, 5), ZW.ERR, b""]
        dims = ZW.dims_of(len(frames))
        exp, total = ZW.expect(form, frames, dims)
        assert exp[CODED]["flags"] == Z.FLAG_COMPRESSED and exp[CODED]["sent"] % 16 != 0, "a compressed frame with padding behind it"
        assert exp[AS_IS]["flags"] == 0 and exp[AS_IS]["sent"] == 1100
        out, cap = ZW.emu_run(form, frames, dims)
        assert cap == total and len(out["dst"]) > total
        _runs[form] = frames, dims, out, cap, exp
    return _runs[form]


def _payload(i, k):
    def fault(out, exp, total):
        out["dst"][exp[i]["off"] + k] ^= 1  # (uint8)
    return fault


def _word(key, i):
    def fault(out, exp, total):
        out[key][i] = int(out[key][i]) ^ 1
    return fault


def _padding(out, exp, total):
    out["dst"][exp[CODED]["off"] + exp[CODED]["sent"]] = 0


def _behind(out, exp, total):
    out["dst"][total + 3] = 0


FAULTS = {"a payload byte of the compressed frame": _payload(CODED, 40), "a byte of the frame sent as it is": _payload(AS_IS, 1099),
          "a header byte": _word("hdr", 24 * AS_IS + 5), "pkt of the compressed frame": _word("pkt", CODED),
          "pkt of the error code": _word("pkt", ERROR), "crc": _word("crc", CODED), "crc of the empty frame": _word("crc", EMPTY),
          "off of a frame": _word("off", AS_IS), "off of the error code": _word("off", ERROR), "the total": _word("off", 4),
          "len_out": _word("len_out", AS_IS), "len_out of the error code": _word("len_out", ERROR),
          "padding between two frames": _padding, "a byte behind the last frame": _behind}
FORM_IDS = ["narrow", "wide", "seq"]


@pytest.mark.parametrize("form", ZW.FORMS, ids=FORM_IDS)
def test_the_batch_passes_as_the_kernels_leave_it(form):
    frames, dims, out, cap, _ = _run(form)
    ZW.check(form, frames, dims, out, cap, "clean")


@pytest.mark.parametrize("fault", FAULTS, ids=[f.replace(" ", "_") for f in FAULTS])
@pytest.mark.parametrize("form", ZW.FORMS, ids=FORM_IDS)
def test_one_corrupted_field_fails_the_check(form, fault):
    frames, dims, out, cap, exp = _run(form)
    bad = copy.deepcopy(out)
    FAULTS[fault](bad, exp, cap)
    with pytest.raises(AssertionError):
        ZW.check(form, frames, dims, bad, cap, fault)
