"""What zpack_timing.py, zpack_wide_timing.py and zseq_timing.py share (imported, not run): the PCIe-rate probe, a batch of real
renders with four sets of output buffers over it, the launchers of the packed form and of a compressed form on those buffers,
the two timing loops, and the verdict
    t_form + sent_bytes / pcie_rate  <  t_packed + original_bytes / pcie_rate.
"""
import statistics
import time

import numpy as np

DISTINCT = 16  # source images; a batch cycles through them


def entropy_ratio(data):
    counts = np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=256).astype(np.float64)
    p = counts[counts > 0] / len(data)
    return float(-(p * np.log2(p)).sum() / 8.0)


def smooth_with_noise(orc, sw, sh):
    """DISTINCT source images: S-smooth with a third-size patch of noise, shifted from image to image"""
    rng = np.random.default_rng(1)
    imgs = []
    for k in range(DISTINCT):
        img = orc.frame_smooth(sw, sh).copy()
        x0, y0 = int(rng.integers(0, sw // 2)), int(rng.integers(0, sh // 2))
        img[y0:y0 + sh // 3, x0:x0 + sw // 3] = orc.frame_hash_noise(sw // 3, sh // 3, 100 + k)
        img = np.roll(img, 37 * k, axis=1)
        imgs.append(np.ascontiguousarray(img))
    return imgs


def pcie_rate():
    """bytes per second a device -> pinned host copy reaches (64 MB, median of 10)"""
    import torch
    big = torch.zeros(64 << 20, dtype=torch.uint8, device="cuda")
    pinned = torch.zeros(64 << 20, dtype=torch.uint8).pin_memory()
    ts = []
    for _ in range(10):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pinned.copy_(big, non_blocking=True)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return (64 << 20) / statistics.median(ts)


def pays(t_form, sent, t_packed, original, rate):
    """-> (us of the compressed form with its bytes over PCIe, us of the packed form with its, 'YES' where the first is less)"""
    lhs, rhs = t_form + sent / rate * 1e6, t_packed + original / rate * 1e6
    return lhs, rhs, "YES" if lhs < rhs else "NO"


class Batch:
    """n frames of out_w x out_h rendered once from imgs (n cycles through them) into a slab, and four sets of output buffers
    (destination in mapped host memory) for the wire forms over that slab"""

    def __init__(self, pkg, orc_palette, imgs, mode, rm, out_w, out_h, n, reps, streams, exact_capacity=True):
        import torch
        self.torch, self.pkg, self.n, self.reps, self.streams = torch, pkg, n, reps, streams
        sh, sw = imgs[0].shape[:2]
        self.dev = torch.from_numpy(np.stack(imgs)).cuda()
        fs = [pkg.frame_setup(self.dev.data_ptr() + (i % len(imgs)) * sw * sh * 3, sw, sh, out_w, out_h, rm, False, False, False) for i in range(n)]
        self.plan = pkg.Plan(mode, orc_palette, fs)
        self.stride = stride = self.plan.stride
        self.slab = torch.zeros(n * stride + 16, dtype=torch.uint8, device="cuda")
        self.ln = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.plan.render(self.slab.data_ptr(), stride, self.ln.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        self.lens = self.ln.cpu().numpy().view(np.uint32)
        self.original = int(self.lens.sum())
        # what the frames take at their exact lengths, or a whole slab
        self.cap = int(((self.lens.astype(np.int64) + 15) // 16 * 16).sum()) + 4096 if exact_capacity else n * stride
        self.d = torch.from_numpy(np.array([(out_w, out_h)] * n, dtype=np.uint32).view(np.int32)).cuda()
        self.bufs = []

    def buffers(self, sbytes):
        """the four sets, each with a scratch of sbytes"""
        torch, n = self.torch, self.n
        self.sbytes = sbytes
        self.bufs = [dict(host=self.pkg.HostBuffer(self.cap), off=torch.zeros(n + 1, dtype=torch.int64, device="cuda"),
                          lo=torch.zeros(n, dtype=torch.int32, device="cuda"), crc=torch.zeros(n, dtype=torch.int32, device="cuda"),
                          pkt=torch.zeros(n, dtype=torch.int32, device="cuda"), hdr=torch.zeros(24 * n, dtype=torch.uint8, device="cuda"),
                          scratch=torch.zeros(sbytes // 8 + 1, dtype=torch.int64, device="cuda")) for _ in range(4)]

    def frames(self, count):
        """the first `count` rendered frames as bytes"""
        host_slab = self.slab.cpu().numpy()
        return [host_slab[i * self.stride:i * self.stride + int(self.lens[i])].tobytes() for i in range(min(self.n, count))]

    def packed(self, b, s):
        rc = self.pkg.lib().asciichat_hip_frame_packets_packed(self.slab.data_ptr(), self.stride, self.ln.data_ptr(), self.stride, self.n,
                                                               self.d.data_ptr(), b["crc"].data_ptr(), b["hdr"].data_ptr(), b["pkt"].data_ptr(),
                                                               b["host"].dev, self.cap, b["off"].data_ptr(), b["lo"].data_ptr(), s)
        assert rc == 0, self.pkg.last_error()

    def form(self, fn):
        """fn: pkg.frame_packets_zpacked or one of its forms -> its launcher over a set of buffers"""
        def run(b, s):
            fn(self.slab.data_ptr(), self.stride, self.ln.data_ptr(), self.stride, self.n, self.d.data_ptr(), b["crc"].data_ptr(),
               b["hdr"].data_ptr(), b["pkt"].data_ptr(), b["host"].dev, self.cap, b["off"].data_ptr(), b["lo"].data_ptr(),
               b["scratch"].data_ptr(), self.sbytes, s)
        return run

    def one_at_a_time(self, fn):
        """-> (median, min, max) us between HIP events around one launch"""
        torch = self.torch
        s = torch.cuda.current_stream().cuda_stream
        ts = []
        for r in range(self.reps + 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(self.bufs[0], s)
            b.record()
            torch.cuda.synchronize()
            if r >= 3:
                ts.append(a.elapsed_time(b) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    def four_in_flight(self, fn):
        """-> median wall clock us per launch, 16 launches over the four streams"""
        ts = []
        for r in range(self.reps // 3 + 2):
            self.torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(4):
                for b, st in zip(self.bufs, self.streams):
                    fn(b, st.cuda_stream)
            self.torch.cuda.synchronize()
            if r >= 2:
                ts.append((time.perf_counter() - t0) * 1e6 / 16)
        return statistics.median(ts)

    def sent(self, run):
        """one more launch on the first set -> (sent lengths, offsets, the destination's bytes)"""
        run(self.bufs[0], self.torch.cuda.current_stream().cuda_stream)
        self.torch.cuda.synchronize()
        return self.bufs[0]["lo"].cpu().numpy().view(np.uint32), self.bufs[0]["off"].cpu().numpy(), self.bufs[0]["host"].view()

    def close(self):
        for b in self.bufs:
            b["host"].close()
        self.plan.close()
        self.bufs, self.dev, self.slab = [], None, None
