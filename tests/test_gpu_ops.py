"""The product's gfx950_ops.hpp on the device, op by op: the probe kernels of tests/opsprobe/ through libachip_opsprobe.so (built by
ascii-chat_amd/Makefile with the product's flags) on the shared cases of ops_cases.py against the restatements of ops_ref.py -- the
same kernels, cases and reference test_ops_emulated.py holds the emulator's twin to.  One test per family; no launch is larger
than 64 workgroups of 256 threads, and no probe thread waits for another workgroup."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ops_cases as OC  # noqa: E402

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ascii-chat_amd", "libachip_opsprobe.so")


class DeviceBackend:
    """buffers as torch tensors on the current device, launches on the current torch stream"""

    class _Placed:
        def __init__(self, data):
            import torch
            self.t = torch.from_numpy(np.array(data, dtype=np.uint8, order="C")).cuda()
            self.addr = self.t.data_ptr()

        def read(self):
            return self.t.cpu().numpy()

    def __init__(self):
        import torch
        self.stream = torch.cuda.current_stream().cuda_stream

    def place(self, data):
        return self._Placed(data)

    def sync(self):
        import torch
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def probe():
    import torch
    assert torch.cuda.is_available(), "the machine-ops probe needs a GPU"
    torch.cuda.set_device(0)
    assert os.path.exists(LIB), "libachip_opsprobe.so is built with the product libraries (make -C ascii-chat_amd): it is missing"
    return OC.declare(C.CDLL(LIB))


def test_lane_arithmetic(probe):
    OC.run_lane_arith(probe, DeviceBackend())


def test_lane_arithmetic_with_compile_time_arguments(probe):
    OC.run_lane_const(probe, DeviceBackend())


def test_wave_operations(probe):
    OC.run_wave(probe, DeviceBackend())


def test_lds_byte_stores(probe):
    OC.run_lds_bytes(probe, DeviceBackend())


def test_lds_ors(probe):
    OC.run_lds_or(probe, DeviceBackend())


def test_global_memory_unaligned_and_non_temporal(probe):
    OC.run_gmem(probe, DeviceBackend())


def test_scoped_atomics(probe):
    OC.run_atomics(probe, DeviceBackend())


def test_arrival_hand_off_between_64_workgroups(probe):
    OC.run_arrival(probe, DeviceBackend())


def test_a_grid_beyond_64_workgroups_is_refused(probe):
    assert probe.opsprobe_wave(OC.MAX_GRID + 1, *[None] * 10) == -1
