"""Support of the packed RGB source tests: test sources laid out in one buffer each (the base at a chosen misalignment, the
stride padded with noise, alpha bytes noise), the kernels of libasciichat_pix.so under the CPU emulator
(tests/hipemu/pix_emu_driver.cpp), pix.c itself over the mock HIP runtime, guard-filled destinations, and the one case table the
emulated and the GPU tests share; expectations from tests/pix_ref.py.  TESTS ONLY."""
import ctypes as C
import os

import numpy as np

import emubuild
import pix_ref as PR
from achip_ctypes import Frame

FILL = 0xA5
RGB, RGBA, BGR, BGRA = PR.RGB, PR.RGBA, PR.BGR, PR.BGRA
FORMATS, NAMES, BPP = PR.FORMATS, PR.NAMES, PR.BPP
FLIP_X, FLIP_Y = PR.FLIP_X, PR.FLIP_Y
INVALID, NOT_SUPPORTED = 86, 30
MAX_SIDE, MAX_STRIDE, BOX_W, BOX_H, BOX_OUT = 8192, 1 << 24, 3840, 2160, 16384
HEADERS = ("pix_kernels.hpp", "pix.h", "pix_math.h", "asciichat_pix.h", "achip_desc.h", "achip_types.h")
RUNS = (4, 16)  # the pixels of a lane's run in whole_kernel: both are kept working, one ships (pix.h)


class CSource(C.Structure):  # asciichat_pix_source_t
    _fields_ = [("pixels", C.c_void_p), ("stride", C.c_int32), ("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


_emu = {}


def emulator(run=None):
    """the driver built at the shipped run of whole_kernel (None), or at `run` pixels"""
    if run not in _emu:
        drv = os.path.join(emubuild.EMU_DIR, "pix_emu_driver.cpp")
        assert os.path.exists(drv), "tests/hipemu/pix_emu_driver.cpp is missing: the emulator driver of libasciichat_pix.so"
        if run is None:
            L = C.CDLL(emubuild.shared_library("libpix_emu.so", "pix_emu_driver.cpp", HEADERS))
        else:
            L = C.CDLL(emubuild.shared_library(f"libpix_emu_run{run}.so", "pix_emu_driver.cpp", HEADERS, defines=(f"PIX_WHOLE_PIXELS={run}",)))
        vp, ci, u32 = C.c_void_p, C.c_int, C.c_uint32
        L.emu_pix_whole_pixels.restype = ci
        L.emu_pix_whole_pixels.argtypes = []
        L.emu_pix_bounds.restype = None
        L.emu_pix_bounds.argtypes = [u32, u32, u32, C.POINTER(u32), C.POINTER(u32)]
        L.emu_pix_source_check.restype = ci
        L.emu_pix_source_check.argtypes = [C.POINTER(CSource), C.POINTER(C.c_char_p)]
        L.emu_pix_set_check.restype = ci
        L.emu_pix_set_check.argtypes = [vp, vp, ci, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(C.c_char_p)]
        L.emu_pix_run.restype = ci
        L.emu_pix_run.argtypes = [vp, vp, ci, ci, vp, C.c_uint64, ci, ci]
        L.emu_pix_run_whole.restype = ci
        L.emu_pix_run_whole.argtypes = [vp, ci, ci, vp, C.c_uint64, ci]
        L.emu_pix_convert.restype = ci
        L.emu_pix_convert.argtypes = [C.POINTER(CSource), vp, ci]
        L.emu_pix_downscale.restype = ci
        L.emu_pix_downscale.argtypes = [C.POINTER(CSource), vp, ci, ci, ci, ci]
        assert L.emu_pix_whole_pixels() == (run or L.emu_pix_whole_pixels()) and L.emu_pix_whole_pixels() in RUNS
        _emu[run] = L
    return _emu[run]


# ---- test sources ---------------------------------------------------------------------------------------------------------------
class Src:
    """A source in ONE buffer (`image`, whose byte 0 belongs at a 16-byte boundary): pixel (0, 0) `off` bytes behind a 16-byte
    boundary, rows `stride` apart (0: tight), every other byte -- in front, between the rows, behind, and every alpha byte --
    noise of its own.  pixels: None for noise, or an (h, w, 3) array of the RGB24 values the source is to hold."""

    def __init__(self, fmt, w, h, seed, stride=0, off=0, pixels=None, alpha=None):
        rng = np.random.default_rng(seed)
        bpp = BPP[fmt]
        self.format, self.width, self.height, self.given, self.off = fmt, w, h, stride, off
        self.stride = stride or bpp * w
        assert self.stride >= bpp * w and 0 <= off < 16
        self.at = 64 + off
        self.extent = (h - 1) * self.stride + bpp * w
        image = rng.integers(0, 256, self.at + self.extent + 64, dtype=np.uint8)
        if pixels is not None:
            for y in range(h):
                row = image[self.at + y * self.stride:self.at + y * self.stride + bpp * w].reshape(w, bpp)
                row[:, list(PR.ORDER[fmt])] = pixels[y]
                if alpha is not None and bpp == 4:
                    row[:, 3] = alpha
        image.setflags(write=False)
        self.image = image
        self._whole = None

    def whole(self):
        if self._whole is None:
            self._whole = PR.whole(self.image[self.at:], self.format, self.width, self.height, self.stride)
            self._whole.setflags(write=False)
        return self._whole

    def c_source(self, base, cls=CSource):
        """the structure over a copy of `image` at address base (a multiple of 16)"""
        assert base % 16 == 0
        s = cls()
        s.format, s.width, s.height, s.pixels, s.stride = self.format, self.width, self.height, base + self.at, self.given
        return s


def ramp(fmt, channel, seed):
    """256 x 1: `channel` runs 0..255, the other two channels and alpha are held at distinct constants -- a swapped or leaked
    channel shows in every byte"""
    const = [0x11, 0x22, 0x33]
    px = np.empty((1, 256, 3), dtype=np.uint8)
    px[0, :] = const
    px[0, :, channel] = np.arange(256)
    return Src(fmt, 256, 1, seed, pixels=px, alpha=0x44)


def host_copy(src):
    """-> (array to keep alive, the 16-aligned address of its copy of src.image)"""
    buf = np.empty(src.image.size + 16, dtype=np.uint8)
    start = (-buf.ctypes.data) % 16
    buf[start:start + src.image.size] = src.image
    return buf, buf.ctypes.data + start


def place_on_host(srcs, cls=CSource):
    """-> (arrays to keep alive, [source structures over 16-aligned host copies])"""
    keep = [host_copy(s) for s in srcs]
    return keep, [s.c_source(k[1], cls) for s, k in zip(srcs, keep)]


def frame(src, out_w, out_h, flips=0, x_ratio=None, y_ratio=None, pad_left=0, pad_top=0, ops=0, cls=Frame):
    """the descriptor achip_frame_setup makes for a src.width x src.height source and an out_w x out_h target: the reference's
    ratios ((s << 16) / d) + 1 (image.c:282-283); src stays NULL and src_stride odd -- set() reads neither"""
    f = cls()
    f.src_w, f.src_h, f.out_w, f.out_h, f.pad_left, f.pad_top = src.width, src.height, out_w, out_h, pad_left, pad_top
    f.x_ratio = (src.width << 16) // out_w + 1 if x_ratio is None else x_ratio
    f.y_ratio = (src.height << 16) // out_h + 1 if y_ratio is None else y_ratio
    f.src_stride = -7
    f.ops = flips | ops
    return f


# ---- the cases ------------------------------------------------------------------------------------------------------------------
class Case:
    """items: [(Src, out_w, out_h, flips)]; the handle holds max_frames.  The same items serve the sampled pass (kind "run") and
    the box pass (kind "box")"""

    def __init__(self, items, max_frames=None, pitch_extra=0):
        self.items = [(i[0], i[1], i[2], i[3] if len(i) > 3 else 0) for i in items]
        self.max_frames = max_frames or len(items)
        self.pitch_extra = pitch_extra
        self._expected = {}

    def frames(self, cls=Frame):
        return [frame(s, ow, oh, fl, cls=cls) for s, ow, oh, fl in self.items]

    def expected(self, kind):
        if kind not in self._expected:
            if kind == "run":
                e = [PR.sample(i[0].whole(), f) for i, f in zip(self.items, self.frames())]
            else:
                e = [PR.box(s.whole(), ow, oh, bool(fl & FLIP_X), bool(fl & FLIP_Y)) for s, ow, oh, fl in self.items]
            for a in e:
                a.setflags(write=False)
            self._expected[kind] = e
        return self._expected[kind]

    def pitch(self):
        return (max(3 * i[1] * i[2] for i in self.items) + 127) // 128 * 128 + self.pitch_extra

    def sources(self):
        return [i[0] for i in self.items]


class WholeCase:
    """one source through convert: the destination `dst_off` bytes behind a 16-byte boundary, rows rgb_stride apart (0: tight)"""

    def __init__(self, src, dst_off=0, rgb_stride=0):
        self.src, self.dst_off, self.rgb_stride = src, dst_off, rgb_stride

    def row_stride(self):
        return self.rgb_stride or 3 * self.src.width


def _stride(fmt, w, kind):
    """a padded stride above bpp * w that is a multiple of 16 ("16"), of 4 but not of 16 ("4"), or odd ("1")"""
    s = (BPP[fmt] * w + 16) // 16 * 16
    return {"16": s, "4": s + 4, "1": s + 1}[kind]


# (base offset, stride kind): base offsets 0..15 crossed with strides that are and are not multiples of 16, and 0..3 crossed with
# strides that are and are not multiples of 4 -- offset 0 with a stride of 16s is the aligned path of each kernel, base and
# stride multiples of 4 the dword path, everything else the byte path
ALIGNMENTS = [(off, kind) for off in range(16) for kind in ("16", "4")] + [(off, "1") for off in range(4)]
MIXED = "mixed batch: four formats, four sizes, 8 of 12 frames, a pitch with extra bytes"
_cases = None


def cases():
    """{name: Case}: every case is run by the sampled pass and by the box pass"""
    global _cases
    if _cases is not None:
        return _cases
    c = {}
    for fmt in FORMATS:
        n = NAMES[fmt]
        c[f"{n} 1x1 -> 1x1"] = Case([(Src(fmt, 1, 1, 10 + fmt), 1, 1)])
        c[f"{n} 3x2 -> 3x2 narrower than a run"] = Case([(Src(fmt, 3, 2, 20 + fmt), 3, 2)])
        for w in (4, 5, 6, 7):
            c[f"{n} {w}x2 -> 3x2 width 4k+{w % 4}"] = Case([(Src(fmt, w, 2, 30 + fmt + 4 * w), 3, 2)])
        c[f"{n} 17x3 -> 5x3 a whole run and an edge"] = Case([(Src(fmt, 17, 3, 60 + fmt), 5, 3)])
        for off, kind in ALIGNMENTS:
            c[f"{n} 20x3 -> 7x2 base +{off} stride {kind}"] = Case([(Src(fmt, 20, 3, 70 + fmt, stride=_stride(fmt, 20, kind), off=off), 7, 2)])
        for fl in range(4):
            c[f"{n} 30x17 -> 7x4 flips {fl}"] = Case([(Src(fmt, 30, 17, 100 + fmt), 7, 4, fl)])
        c[f"{n} 6x4 -> 6x4 identity"] = Case([(Src(fmt, 6, 4, 110 + fmt), 6, 4)])
        c[f"{n} 5x3 -> 11x7 upscale"] = Case([(Src(fmt, 5, 3, 120 + fmt), 11, 7)])
        c[f"{n} 64x36 -> 1x1"] = Case([(Src(fmt, 64, 36, 130 + fmt), 1, 1)])
        c[f"{n} 64x48 -> 37x29 two workgroups of samples"] = Case([(Src(fmt, 64, 48, 140 + fmt), 37, 29)])
        c[f"{n} 1031x3 -> 7x2 a second group per lane"] = Case([(Src(fmt, 1031, 3, 150 + fmt), 7, 2)])
        c[f"{n} 3840x2 -> 80x1 the widest stage"] = Case([(Src(fmt, 3840, 2, 160 + fmt), 80, 1)])
        for ch in range(3):
            c[f"{n} ramp in channel {ch} 256x1 -> 256x1"] = Case([(ramp(fmt, ch, 170 + fmt), 256, 1)])
            c[f"{n} ramp in channel {ch} 256x1 -> 64x1"] = Case([(ramp(fmt, ch, 170 + fmt), 64, 1)])
    sizes = [((16, 8), (5, 3)), ((30, 17), (7, 4)), ((64, 48), (9, 5)), ((6, 4), (1, 1))]
    items = []
    for i in range(8):
        fmt = FORMATS[(i + i // 4) % 4]
        (w, h), (ow, oh) = sizes[(i * 3) % 4]
        items.append((Src(fmt, w, h, 300 + i, stride=BPP[fmt] * w + (0, 3, 4, 16)[i % 4], off=(0, 5, 4, 2)[i % 4]), ow, oh, i % 4))
    c[MIXED] = Case(items, max_frames=12, pitch_extra=48)
    _cases = c
    return c


_whole_cases = None


def whole_cases():
    """{format: {name: WholeCase}} for convert: 1x1, 3x2, every w % 4, a whole run of 16 and its edges, more lanes than a
    workgroup's 64 at either run, every destination offset 0..3 with tight and explicit rows, every source alignment, the ramps"""
    global _whole_cases
    if _whole_cases is not None:
        return _whole_cases
    out = {}
    for fmt in FORMATS:
        c, k = {}, 0
        for w, h in ((1, 1), (3, 2), (4, 2), (5, 2), (6, 2), (7, 2), (16, 2), (17, 3), (40, 3), (30, 17), (300, 2), (1100, 2)):
            pad = (k // 4) % 2
            c[f"{w}x{h} dst +{k % 4} {'padded' if pad else 'tight'}"] = WholeCase(Src(fmt, w, h, 200 + 40 * fmt + k), k % 4, 3 * w + 5 if pad else 0)
            k += 1
        for off in range(4):
            for stride in (0, 3 * 18 + 1, 3 * 18 + 4):  # tight; padded so that the rows' alignments differ; padded and alike
                c[f"18x4 dst +{off} rgb_stride {stride}"] = WholeCase(Src(fmt, 18, 4, 300 + fmt), off, stride)
        # 32 pixels a row: a run of 16 leaves as three 16-byte stores where the row is a multiple of 16 (rows of 96 bytes: all are)
        for off in (0, 4, 16 - 3):
            c[f"32x3 dst +{off} rows of 96 bytes"] = WholeCase(Src(fmt, 32, 3, 310 + fmt, stride=_stride(fmt, 32, "16")), off, 0)
        for off, kind in ALIGNMENTS:
            c[f"36x3 source base +{off} stride {kind}"] = WholeCase(Src(fmt, 36, 3, 320 + fmt, stride=_stride(fmt, 36, kind), off=off), off % 4, 0)
        for ch in range(3):
            c[f"ramp in channel {ch}"] = WholeCase(ramp(fmt, ch, 330 + fmt), ch, 0)
        out[fmt] = c
    _whole_cases = out
    return out


def whole_batch():
    """sources of every format and several sizes for one run_whole"""
    return cases()[MIXED].sources() + [Src(RGB, 17, 3, 400), Src(BGRA, 36, 4, 401, stride=157, off=1), Src(RGBA, 1, 1, 402), Src(BGR, 40, 2, 403, off=8)]


# ---- destinations ---------------------------------------------------------------------------------------------------------------
def image_buffer(case, base=None):
    """-> (guard-filled buffer, byte index of image 0: a 16-byte boundary of the address the bytes will live at, pitch)"""
    pitch = case.pitch()
    buf = np.full(64 + 16 + len(case.items) * pitch + 256, FILL, dtype=np.uint8)
    start = 64 + (-((buf.ctypes.data if base is None else base) + 64)) % 16
    return buf, start, pitch


def check_images(name, case, kind, buf, start, pitch):
    """every image the restatement's, every other byte -- in front, between, behind -- still the guard"""
    assert (buf[:start] == FILL).all(), f"{name}: a store in front of the first image"
    for i, want in enumerate(case.expected(kind)):
        nb = want.size
        got = buf[start + i * pitch:start + i * pitch + nb]
        if not np.array_equal(got, want.reshape(-1)):
            k = int(np.argmax(got != want.reshape(-1)))
            raise AssertionError(f"{name} ({kind}) frame {i}: byte {k} (pixel {k // 3} of {nb // 3}) is {int(got[k])}, restatement {int(want.reshape(-1)[k])}")
        assert (buf[start + i * pitch + nb:start + (i + 1) * pitch] == FILL).all(), f"{name} ({kind}) frame {i}: a store beyond the image"
    assert (buf[start + len(case.items) * pitch:] == FILL).all(), f"{name}: a store past the last image"


def whole_buffer(case, base=None):
    """-> (guard-filled buffer, byte index of the image, bytes the image spans)"""
    span = (case.src.height - 1) * case.row_stride() + 3 * case.src.width
    buf = np.full(64 + 16 + 16 + span + 128, FILL, dtype=np.uint8)
    start = 64 + (-((buf.ctypes.data if base is None else base) + 64)) % 16 + case.dst_off
    return buf, start, span


def check_whole(name, src, buf, start, row_stride, end=None):
    """the image of src at buf[start:], rows row_stride apart; everything else up to `end` still the guard"""
    want = src.whole()
    h, w = want.shape[:2]
    assert (buf[:start] == FILL).all(), f"{name}: a store in front of the image"
    for y in range(h):
        row = buf[start + y * row_stride:start + y * row_stride + 3 * w]
        if not np.array_equal(row, want[y].reshape(-1)):
            k = int(np.argmax(row != want[y].reshape(-1)))
            raise AssertionError(f"{name}: row {y} byte {k} (pixel {k // 3}) is {int(row[k])}, restatement {int(want[y].reshape(-1)[k])}")
        stop = start + (y + 1) * row_stride if y + 1 < h else (buf.size if end is None else end)
        assert (buf[start + y * row_stride + 3 * w:stop] == FILL).all(), f"{name}: a store behind the {3 * w} bytes of row {y}"


def batch_buffer(srcs, base=None, extra=48):
    """run_whole's destination for srcs: -> (guard-filled buffer, start, pitch)"""
    pitch = (max(3 * s.width * s.height for s in srcs) + 127) // 128 * 128 + extra
    buf = np.full(64 + 16 + len(srcs) * pitch + 128, FILL, dtype=np.uint8)
    start = 64 + (-((buf.ctypes.data if base is None else base) + 64)) % 16 + 3  # (any alignment)
    return buf, start, pitch


def check_batch(name, srcs, buf, start, pitch):
    assert (buf[:start] == FILL).all(), f"{name}: a store in front of the first image"
    for i, s in enumerate(srcs):
        nb = 3 * s.width * s.height
        got = buf[start + i * pitch:start + i * pitch + nb]
        assert np.array_equal(got, s.whole().reshape(-1)), f"{name}: image {i} ({NAMES[s.format]} {s.width}x{s.height}) differs at byte {int(np.argmax(got != s.whole().reshape(-1)))}"
        assert (buf[start + i * pitch + nb:start + (i + 1) * pitch] == FILL).all(), f"{name}: a store beyond image {i}"
    assert (buf[start + len(srcs) * pitch:] == FILL).all(), f"{name}: a store past the last image"


# ---- the kernels under the emulator ---------------------------------------------------------------------------------------------
def emu_run(case, kind, host=False):
    """-> (buffer, start, pitch) of the sampled pass ("run") or the box pass ("box") under the emulator (host: the host walk of
    pix.h in the kernel's place)"""
    keep, sources = place_on_host(case.sources())
    n = len(case.items)
    srcs = (CSource * n)(*sources)
    frames = (Frame * n)(*case.frames())
    buf, start, pitch = image_buffer(case)
    rc = emulator().emu_pix_run(C.cast(srcs, C.c_void_p), C.cast(frames, C.c_void_p), n, case.max_frames, buf.ctypes.data + start, pitch,
                                int(kind == "box"), int(host))
    assert rc == 0, f"refused ({rc})"
    return buf, start, pitch


def emu_convert(case, run=None):
    keep, addr = host_copy(case.src)
    buf, start, _ = whole_buffer(case)
    s = case.src.c_source(addr)
    rc = emulator(run).emu_pix_convert(C.byref(s), buf.ctypes.data + start, case.rgb_stride)
    assert rc == 0, f"refused ({rc})"
    return buf, start


def emu_run_whole(srcs, run=None, host=False, max_frames=None):
    keep, sources = place_on_host(srcs)
    arr = (CSource * len(srcs))(*sources)
    buf, start, pitch = batch_buffer(srcs)
    rc = emulator(run).emu_pix_run_whole(C.cast(arr, C.c_void_p), len(srcs), max_frames or len(srcs), buf.ctypes.data + start, pitch, int(host))
    assert rc == 0, f"refused ({rc})"
    return buf, start, pitch


# ---- the host side (pix.c) through its C interface: the real library on a GPU, or the mock build without one --------------------
EXPORTS = ("device_count", "last_error", "convert", "downscale", "create", "set", "image_pitch", "run", "run_box", "render_frames", "whole_pitch",
           "run_whole", "destroy")


def bind(L):
    vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
    for name, res, args in (("device_count", ci, []), ("last_error", C.c_char_p, []), ("convert", ci, [vp, vp, ci, vp]),
                            ("downscale", ci, [vp, vp, ci, ci, ci, ci, vp]), ("create", ci, [C.POINTER(vp), ci]), ("set", ci, [vp, vp, vp, ci, vp]),
                            ("image_pitch", sz, [vp]), ("run", ci, [vp, vp, sz, vp]), ("run_box", ci, [vp, vp, sz, vp]),
                            ("render_frames", ci, [vp, vp, sz, vp]), ("whole_pitch", sz, [vp]), ("run_whole", ci, [vp, vp, sz, vp]),
                            ("destroy", None, [vp])):
        fn = getattr(L, "asciichat_pix_" + name)
        fn.restype, fn.argtypes = res, args
    return L


_mock = None


def mock_library():
    """pix.c as it stands over the mock HIP runtime (tests/mockhip/mock_hip.c: device memory is host memory), its launchers the
    emulator's (pix_emu_driver.cpp): the handle's own code without a GPU"""
    global _mock
    if _mock is None:
        import subprocess
        import mockgpu
        so = os.path.join(emubuild.OUT_DIR, "libpix_mock.so")
        srcs = [os.path.join(emubuild.CSRC, "pix.c"), os.path.join(mockgpu.MOCK, "mock_hip.c"), os.path.join(emubuild.EMU_DIR, "pix_emu_driver.cpp")]
        for s in srcs:
            assert os.path.exists(s), f"{s} is missing"
        deps = srcs + [emubuild._header(h) for h in ("hip_emu.h", "gfx950_ops.hpp") + HEADERS]
        if not (os.path.exists(so) and all(os.path.getmtime(d) <= os.path.getmtime(so) for d in deps)):
            os.makedirs(emubuild.OUT_DIR, exist_ok=True)
            tag = ".%d" % os.getpid()
            objs = []
            for src in srcs[:2]:
                objs.append(os.path.join(emubuild.OUT_DIR, "pix_" + os.path.basename(src) + tag + ".o"))
                subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fPIC", "-pthread", "-I" + emubuild.INC, "-I" + emubuild.CSRC, "-I" + mockgpu.HIP_INC,
                                       "-c", src, "-o", objs[-1]])
            # -Bsymbolic: the hip* calls bind to the mock runtime inside this library whatever else the process has loaded
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wl,-Bsymbolic", *["-I" + d for d in emubuild.INCLUDE], srcs[2], *objs,
                                   "-o", so + tag, "-lpthread"])
            os.replace(so + tag, so)
            for o in objs:
                os.remove(o)
        _mock = bind(C.CDLL(so))
    return _mock


class Handle:
    """asciichat_pix_* of a bound library, return codes as they come"""

    def __init__(self, L, max_frames, stream=0):
        self.L, self.h, self.stream = L, C.c_void_p(), stream
        rc = L.asciichat_pix_create(C.byref(self.h), max_frames)
        assert rc == 0, (rc, self.error())

    def error(self):
        return self.L.asciichat_pix_last_error().decode()

    def set(self, sources, frames, n=None):
        """sources, frames: lists of structures (or None for a NULL array)"""
        self._keep = (None if sources is None else (type(sources[0]) * len(sources))(*sources),
                      None if frames is None else (type(frames[0]) * len(frames))(*frames))
        count = n if n is not None else len(sources)
        return self.L.asciichat_pix_set(self.h, *[C.cast(a, C.c_void_p) if a is not None else None for a in self._keep], count, self.stream)

    def pitch(self):
        return int(self.L.asciichat_pix_image_pitch(self.h))

    def whole_pitch(self):
        return int(self.L.asciichat_pix_whole_pitch(self.h))

    def run(self, images, pitch, kind="run"):
        return (self.L.asciichat_pix_run_box if kind == "box" else self.L.asciichat_pix_run)(self.h, images, pitch, self.stream)

    def run_whole(self, rgb, pitch):
        return self.L.asciichat_pix_run_whole(self.h, rgb, pitch, self.stream)

    def render_frames(self, images, pitch, n, cls=Frame):
        out = (cls * n)()
        rc = self.L.asciichat_pix_render_frames(self.h, images, pitch, C.cast(out, C.c_void_p))
        return rc, [out[i] for i in range(n)]

    def close(self):
        if self.h:
            self.L.asciichat_pix_destroy(self.h)
            self.h = C.c_void_p()


def changed(obj, **kw):
    c = type(obj).from_buffer_copy(bytes(obj))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def check_render_frames(given, out, images, pitch):
    """what asciichat_hip_box_render_frames documents, field for field"""
    for i, (f, d) in enumerate(zip(given, out)):
        assert d.src == images + i * pitch and d.comp is None, i
        assert (d.src_w, d.src_h, d.out_w, d.out_h) == (f.out_w, f.out_h, f.out_w, f.out_h), i
        assert (d.x_ratio, d.y_ratio, d.src_stride) == (65537, 65537, 3 * f.out_w), i
        assert (d.pad_left, d.pad_top) == (f.pad_left, f.pad_top) and d.ops == f.ops & ~(FLIP_X | FLIP_Y), i


def refusal_case():
    """two frames: a padded BGRA source and an RGB one, flipped"""
    return Case([(Src(BGRA, 16, 8, 950, stride=16 * 4 + 12, off=4), 5, 3), (Src(RGB, 18, 6, 951), 4, 2, 3)], max_frames=2)


def check_refusals(L, place, new_images, stream=0, synchronize=lambda: None):
    """Every refusal of include/asciichat_pix.h at its limit -- the last accepted value passes, the first refused is refused with
    its code --, that a refused call launches nothing and leaves the handle as it was, and that the handle still works.
    place(srcs) -> (keep, [sources at addresses L's kernels can read]); new_images(case) -> (address of image 0, pitch,
    read: () -> (buffer, start))"""
    case = refusal_case()
    keep, sources = place(case.sources())
    frames = case.frames(Frame)
    images, pitch, read = new_images(case)
    # create
    for bad in (0, -1, 65536):
        h = C.c_void_p(1)
        assert L.asciichat_pix_create(C.byref(h), bad) == INVALID and not h.value and str(bad) in L.asciichat_pix_last_error().decode()
    assert L.asciichat_pix_create(None, 2) == INVALID
    for good in (1, 65535):
        Handle(L, good).close()
    # a handle that is not one of this library's
    junk = np.zeros(512, dtype=np.uint8)
    for address in (junk.ctypes.data, None):
        hh = Handle.__new__(Handle)
        hh.L, hh.h, hh.stream = L, C.c_void_p(address), stream
        assert hh.set(sources, frames) == INVALID and hh.run(images, pitch) == INVALID and hh.run(images, pitch, "box") == INVALID
        assert hh.run_whole(images, 1 << 20) == INVALID and hh.render_frames(images, pitch, 2)[0] == INVALID
        assert hh.pitch() == 0 and hh.whole_pitch() == 0 and "not a handle" in hh.error()

    g = Handle(L, 2, stream)
    try:
        # before any set
        assert g.run(images, pitch) == INVALID and "no descriptors" in g.error() and g.run(images, pitch, "box") == INVALID
        assert g.run_whole(images, 1 << 20) == INVALID and "no sources" in g.error()
        assert g.render_frames(images, pitch, 2)[0] == INVALID and g.pitch() == 0 and g.whole_pitch() == 0

        def code(srcs=sources, frs=frames, n=None, named=None):
            rc = g.set(srcs, frs, n)
            assert rc in (0, INVALID, NOT_SUPPORTED), (rc, g.error())
            if rc and named:
                assert named in g.error(), g.error()
            return rc

        def with_source(i, **kw):
            return [changed(s, **kw) if k == i else s for k, s in enumerate(sources)]

        def with_frame(i, **kw):
            return [changed(f, **kw) if k == i else f for k, f in enumerate(frames)]

        def sized(i, w, h, **kw):
            """source and descriptor i at w x h (the pixels are not read: the set is refused, or replaced before any run)"""
            return dict(srcs=with_source(i, width=w, height=h, **kw), frs=with_frame(i, src_w=w, src_h=h))

        assert code() == 0
        # the arrays and their number
        assert code(srcs=None, n=2) == INVALID
        assert code(n=0) == INVALID and code(n=-1) == INVALID and code(n=1) == 0 and code(n=2) == 0
        assert code(srcs=sources + sources[:1], frs=frames + frames[:1]) == INVALID and "max_frames" in g.error()
        # width and height: 1..8192
        for w, h, want in ((0, 8, INVALID), (8193, 8, INVALID), (16, 0, INVALID), (16, 8193, INVALID), (-1, 8, INVALID), (1, 1, 0), (8192, 1, 0), (1, 8192, 0)):
            assert code(**sized(1, w, h, stride=0), named="frame 1") == want, (w, h)
        # the stride: bpp * w - 1 refused, bpp * w taken, 2^24 - 1 taken, 2^24 and a negative one refused, 0 tight
        for i, bpp, w in ((0, 4, 16), (1, 3, 18)):
            for stride, want in ((bpp * w - 1, INVALID), (bpp * w, 0), (0, 0), (MAX_STRIDE - 1, 0), (MAX_STRIDE, INVALID), (-1, INVALID), (-bpp * w, INVALID)):
                assert code(srcs=with_source(i, stride=stride), named=f"frame {i}") == want, (i, stride)
        # the format: 0..3; the pixels
        for fmt, want in ((-1, INVALID), (4, INVALID), (RGBA, 0)):  # (RGBA over 18 x 6 tight: 72 bytes a row)
            assert code(srcs=with_source(1, format=fmt), named="frame 1") == want, fmt
        assert code(srcs=with_source(0, format=RGB)) == 0  # (BGRA's stride of 76 holds RGB's 48)
        assert code(srcs=with_source(1, pixels=None), named="frame 1") == INVALID and "no pixels" in g.error()
        # the descriptor's size is the source's
        for kw in (dict(src_w=15), dict(src_w=17), dict(src_h=7), dict(src_h=9)):
            assert code(frs=with_frame(0, **kw), named="frame 0") == INVALID, kw
        # the image's size and the ratios (achip_frame_ratios_ok)
        for kw in (dict(out_w=0), dict(out_h=0), dict(out_w=-1), dict(out_w=1 << 15, out_h=1 << 15, x_ratio=1, y_ratio=1)):
            assert code(frs=with_frame(1, **kw), named="frame 1") == INVALID, kw
        assert code(frs=with_frame(1, out_w=5, x_ratio=(1 << 30) - 1)) == 0 and code(frs=with_frame(1, out_w=5, x_ratio=1 << 30), named="2^32") == INVALID
        assert code(frs=with_frame(1, out_h=3, y_ratio=1 << 31), named="2^32") == INVALID
        # comp: refused as unsupported, nothing else is
        assert code(frs=with_frame(1, comp=1), named="frame 1") == NOT_SUPPORTED
        # src and src_stride are not read; paddings, tints and the other bits of ops pass through
        assert code(frs=with_frame(0, src=1, src_stride=-9, pad_left=3, pad_top=2, ops=3 | 4 | 0x112233 << 8)) == 0

        # a refused set leaves the set before: its pitches, its descriptors, its sources
        assert code() == 0
        before = g.pitch(), g.whole_pitch(), [bytes(f) for f in g.render_frames(images, pitch, 2)[1]]
        assert before[:2] == (128, 384)
        assert code(frs=with_frame(0, out_w=0)) == INVALID and code(frs=with_frame(1, comp=1)) == NOT_SUPPORTED and code(n=0) == INVALID
        assert code(**sized(0, 8193, 8)) == INVALID and code(srcs=with_source(0, stride=63)) == INVALID and code(srcs=with_source(1, format=4)) == INVALID
        assert (g.pitch(), g.whole_pitch(), [bytes(f) for f in g.render_frames(images, pitch, 2)[1]]) == before
        # the images' place
        for kind in ("run", "box"):
            assert g.run(None, pitch, kind) == INVALID and g.run(images + 8, pitch, kind) == INVALID and g.run(images, pitch + 8, kind) == INVALID
            assert g.run(images, 32, kind) == INVALID and "below" in g.error()  # below the largest image's 45 bytes
        assert g.render_frames(None, pitch, 2)[0] == INVALID and g.render_frames(images, 32, 2)[0] == INVALID
        assert L.asciichat_pix_render_frames(g.h, images, pitch, None) == INVALID and "no descriptors to write" in g.error()
        assert g.run_whole(None, 384) == INVALID and g.run_whole(images, 383) == INVALID and "384" in g.error()
        # convert and downscale
        one = sources[0]
        conv = lambda s, dst, st: L.asciichat_pix_convert(C.byref(s) if s is not None else None, dst, st, stream)  # noqa: E731
        assert conv(None, images, 0) == INVALID and conv(one, None, 0) == INVALID
        assert conv(one, images, 47) == INVALID and conv(one, images, MAX_STRIDE) == INVALID and conv(one, images, -48) == INVALID
        assert conv(changed(one, width=0), images, 0) == INVALID and conv(changed(one, stride=63), images, 0) == INVALID
        down = lambda s, dst, w, h: L.asciichat_pix_downscale(C.byref(s) if s is not None else None, dst, w, h, 0, 0, stream)  # noqa: E731
        assert down(None, images, 5, 3) == INVALID and down(one, None, 5, 3) == INVALID
        assert down(one, images, 0, 3) == INVALID and down(one, images, 5, BOX_OUT + 1) == INVALID
        assert down(changed(one, width=BOX_W + 1, stride=0), images, 5, 3) == INVALID and "3840" in L.asciichat_pix_last_error().decode()
        assert down(changed(one, height=BOX_H + 1), images, 5, 3) == INVALID and down(changed(one, format=4), images, 5, 3) == INVALID
        # run without descriptors: the set is taken, run_whole serves it, run / run_box / render_frames refuse
        assert code(frs=None, n=2) == 0 and g.pitch() == 0 and g.whole_pitch() == 384
        assert g.run(images, pitch) == INVALID and "no descriptors" in g.error() and g.run(images, pitch, "box") == INVALID
        assert g.render_frames(images, pitch, 2)[0] == INVALID
        assert code() == 0
        synchronize()
        buf, start = read()
        assert (buf == FILL).all(), "a refused call launched something"
        # and the handle still works, with the set it was left with
        for kind in ("run", "box"):
            assert g.run(images, pitch, kind) == 0
            synchronize()
            buf, start = read()
            check_images("after the refusals", case, kind, buf, start, pitch)
        rc, out = g.render_frames(images, pitch, 2)
        assert rc == 0
        check_render_frames(frames, out, images, pitch)
    finally:
        g.close()
    return keep


def check_too_large_for_the_box(L, place, new_images, stream=0, synchronize=lambda: None):
    """3841 x 1: refused by run_box with ERR_NOT_SUPPORTED, decided at set; accepted by run and run_whole"""
    wide = Case([(Src(BGRA, BOX_W + 1, 1, 960), 9, 1), (Src(RGB, 12, 2, 961), 9, 1)], max_frames=2)
    keep, sources = place(wide.sources())
    images, pitch, read = new_images(wide)
    g = Handle(L, 2, stream)
    try:
        assert g.set(sources, wide.frames()) == 0
        assert g.run(images, pitch, "box") == NOT_SUPPORTED and "3840" in g.error()
        synchronize()
        assert (read()[0] == FILL).all(), "a refused run_box launched something"
        assert g.run(images, pitch) == 0
        synchronize()
        buf, start = read()
        check_images("3841x1", wide, "run", buf, start, pitch)
        return g, keep, wide  # (the caller runs run_whole into a destination of its own, then closes)
    except BaseException:
        g.close()
        raise
