"""Support of the YUV source tests: test sources laid out in one buffer each (planes at chosen misalignments, strides padded
with noise), the kernels of libasciichat_yuv.so under the CPU emulator (tests/hipemu/yuv_emu_driver.cpp), guard-filled
destinations, and the one case table the emulated and the GPU tests share.  TESTS ONLY."""
import ctypes as C

import numpy as np

import emubuild
import yuv_ref as YR
from achip_ctypes import Frame

FILL = 0xA5
I420, NV12, YUYV, UYVY = YR.I420, YR.NV12, YR.YUYV, YR.UYVY
FORMATS = (I420, NV12, YUYV, UYVY)
PLANAR = (I420, NV12)


class CSource(C.Structure):  # asciichat_yuv_source_t
    _fields_ = [("plane", C.c_void_p * 3), ("stride", C.c_int32 * 3), ("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


_emu = None


def emulator():
    global _emu
    if _emu is None:
        L = C.CDLL(emubuild.shared_library("libyuv_emu.so", "yuv_emu_driver.cpp",
                                           ("yuv_kernels.hpp", "yuv.h", "yuv_math.h", "asciichat_yuv.h", "achip_desc.h", "achip_types.h")))
        vp, ci = C.c_void_p, C.c_int
        L.emu_yuv_rgb.restype = C.c_uint32
        L.emu_yuv_rgb.argtypes = [C.c_uint32] * 3
        L.emu_yuv_rgb_all.restype = None
        L.emu_yuv_rgb_all.argtypes = [vp]
        L.emu_yuv_source_check.restype = ci
        L.emu_yuv_source_check.argtypes = [C.POINTER(CSource), C.POINTER(C.c_char_p)]
        L.emu_yuv_frames_check.restype = ci
        L.emu_yuv_frames_check.argtypes = [vp, vp, ci, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(C.c_char_p)]
        L.emu_yuv_host_pixel.restype = C.c_uint32
        L.emu_yuv_host_pixel.argtypes = [C.POINTER(CSource), ci, ci]
        L.emu_yuv_run.restype = ci
        L.emu_yuv_run.argtypes = [vp, vp, ci, ci, vp, C.c_uint64]
        L.emu_yuv_run_whole.restype = ci
        L.emu_yuv_run_whole.argtypes = [vp, ci, ci, vp, C.c_uint64]
        L.emu_yuv_convert.restype = ci
        L.emu_yuv_convert.argtypes = [C.POINTER(CSource), vp, ci]
        _emu = L
    return _emu


# ---- test sources ---------------------------------------------------------------------------------------------------------------
class Src:
    """A source of noise samples in ONE buffer (`image`, whose byte 0 belongs at a 16-byte boundary): plane k starts offs[k]
    bytes behind a 16-byte boundary, rows strides[k] apart (0: tight), the bytes between rows and planes noise of their own.
    given: the strides as the caller states them (0 kept); ref: the yuv_ref.Source over the same bytes."""

    def __init__(self, fmt, w, h, seed, strides=(0, 0, 0), offs=(0, 0, 0), extremes=False):
        rng = np.random.default_rng(seed)
        cw, ch = YR.chroma_size(w, h)
        Y = rng.integers(0, 256, (h, w), dtype=np.uint8)
        cshape = (h, w // 2) if fmt in YR.PACKED else (ch, cw)
        U = rng.integers(0, 256, cshape, dtype=np.uint8)
        V = rng.integers(0, 256, cshape, dtype=np.uint8)
        if extremes:  # the ends of every range occur
            Y.reshape(-1)[:2] = (0, 255)
            U.reshape(-1)[:1] = 0
            V.reshape(-1)[:1] = 255
        planes, resolved = YR.pack(fmt, Y, U, V, strides, fill=rng)
        self.format, self.width, self.height = fmt, w, h
        self.given = tuple(strides[k] if k < len(planes) else 0 for k in range(3))
        self.at, pos = [], 64
        for k, p in enumerate(planes):
            pos = (pos + 15) // 16 * 16 + offs[k]
            self.at.append(pos)
            pos += p.size + 5
        self.image = rng.integers(0, 256, pos + 64, dtype=np.uint8)
        for a, p in zip(self.at, planes):
            self.image[a:a + p.size] = p
        self.image.setflags(write=False)
        self.ref = YR.Source(fmt, w, h, [self.image[a:] for a in self.at], resolved)
        self._whole = None

    def whole(self):
        if self._whole is None:
            self._whole = YR.convert_whole(self.ref)
            self._whole.setflags(write=False)
        return self._whole

    def c_source(self, base, cls=CSource):
        """the structure over a copy of `image` at address base (a multiple of 16)"""
        assert base % 16 == 0
        s = cls()
        s.format, s.width, s.height = self.format, self.width, self.height
        for k in range(3):
            s.plane[k] = base + self.at[k] if k < len(self.at) else None
            s.stride[k] = self.given[k]
        return s


def host_copy(src):
    """-> (array to keep alive, the 16-aligned address of its copy of src.image)"""
    buf = np.empty(src.image.size + 16, dtype=np.uint8)
    start = (-buf.ctypes.data) % 16
    buf[start:start + src.image.size] = src.image
    return buf, buf.ctypes.data + start


def frame(src, out_w, out_h, flips=0, x_ratio=None, y_ratio=None, pad_left=0, pad_top=0, ops=0, cls=Frame):
    """the descriptor achip_frame_setup makes for a src.width x src.height source and an out_w x out_h target: the reference's
    ratios ((s << 16) / d) + 1 (image.c:282-283); src is left NULL -- set() does not read it"""
    f = cls()
    f.src_w, f.src_h, f.out_w, f.out_h, f.pad_left, f.pad_top = src.width, src.height, out_w, out_h, pad_left, pad_top
    f.x_ratio = (src.width << 16) // out_w + 1 if x_ratio is None else x_ratio
    f.y_ratio = (src.height << 16) // out_h + 1 if y_ratio is None else y_ratio
    f.ops = flips | ops
    return f


# ---- the sampled pass: cases --------------------------------------------------------------------------------------------------------
class SampleCase:
    """items: [(Src, out_w, out_h, flips, ratios or None)]; the handle holds max_frames"""

    def __init__(self, items, max_frames=None, pitch_extra=0):
        self.items = [(i[0], i[1], i[2], i[3] if len(i) > 3 else 0, i[4] if len(i) > 4 else None) for i in items]
        self.max_frames = max_frames or len(items)
        self.pitch_extra = pitch_extra
        self._expected = None

    def frames(self, cls=Frame):
        return [frame(s, ow, oh, fl, *(r or (None, None)), cls=cls) for s, ow, oh, fl, r in self.items]

    def expected(self):
        if self._expected is None:
            self._expected = [YR.sample(i[0].ref, f) for i, f in zip(self.items, self.frames())]
            for e in self._expected:
                e.setflags(write=False)
        return self._expected

    def pitch(self):
        return (max(3 * i[1] * i[2] for i in self.items) + 127) // 128 * 128 + self.pitch_extra


_SIZES = [(16, 8), (7, 5), (2, 2), (300, 2), (64, 48), (4, 2), (30, 17)]


def _mixed(count, seed):
    """formats and sizes mixed per frame"""
    items = []
    for i in range(count):
        fmt = FORMATS[(i + i // 4) % 4]
        w, h = _SIZES[(i * 3 + seed) % len(_SIZES)]
        if fmt in YR.PACKED and w % 2:
            w += 1
        ow, oh = [(5, 3), (9, 5), (1, 1), (13, 4), (6, 8)][i % 5]
        items.append((Src(fmt, w, h, 1000 * seed + i, offs=(i % 4, (i + 1) % 4, (i + 2) % 4)), ow, oh, i % 4))
    return items


_sample_cases = None


def sample_cases():
    global _sample_cases
    if _sample_cases is not None:
        return _sample_cases
    c = {}
    for fmt in FORMATS:
        n = YR.NAMES[fmt]
        c[f"{n} 16x8 -> 5x3: a tail of bytes"] = SampleCase([(Src(fmt, 16, 8, 10 + fmt, extremes=True), 5, 3)])
        c[f"{n} 2x2 -> 1x1"] = SampleCase([(Src(fmt, 2, 2, 20 + fmt), 1, 1)])
        c[f"{n} upscale 4x2 -> 9x5"] = SampleCase([(Src(fmt, 4, 2, 30 + fmt), 9, 5)])
        # ratios near twice the sizes': the second half of the columns and rows reaches the min clamp
        c[f"{n} 4x2 -> 9x5 into the clamp"] = SampleCase([(Src(fmt, 4, 2, 40 + fmt), 9, 5, 0, (2 * 29128, 2 * 26215))])
        for fl, what in ((1, "flip x"), (2, "flip y"), (3, "both flips")):
            c[f"{n} 16x8 -> 5x3 {what}"] = SampleCase([(Src(fmt, 16, 8, 50 + fmt), 5, 3, fl)])
        c[f"{n} half-block: 16x8 -> 5x6"] = SampleCase([(Src(fmt, 16, 8, 60 + fmt), 5, 6)])
    # padded strides, the chroma strides different from the luma stride; plane bases off their alignment
    c["I420 strides 24 / 13 / 11"] = SampleCase([(Src(I420, 16, 8, 70, strides=(24, 13, 11), offs=(1, 3, 2)), 5, 3)])
    c["NV12 strides 19 / 22"] = SampleCase([(Src(NV12, 16, 8, 71, strides=(19, 22, 0), offs=(3, 1, 0)), 5, 3)])
    c["YUYV stride 37"] = SampleCase([(Src(YUYV, 16, 8, 72, strides=(37, 0, 0), offs=(1, 0, 0)), 5, 3)])
    c["UYVY stride 40"] = SampleCase([(Src(UYVY, 16, 8, 73, strides=(40, 0, 0), offs=(2, 0, 0)), 5, 3)])
    for fmt in PLANAR:  # odd in both axes: the last chroma column and row stand for one pixel column and row
        c[f"{YR.NAMES[fmt]} 7x5 -> 7x5 and -> 4x3"] = SampleCase([(Src(fmt, 7, 5, 80 + fmt), 7, 5), (Src(fmt, 7, 5, 82 + fmt), 4, 3, 3)])
    for fmt in YR.PACKED:  # every sx: the odd and the even pixel of each pair
        c[f"{YR.NAMES[fmt]} 8x2 -> 8x2: both pixels of a pair"] = SampleCase([(Src(fmt, 8, 2, 90 + fmt), 8, 2)])
    c["I420 300x2 -> 300x2"] = SampleCase([(Src(I420, 300, 2, 100), 300, 2)])
    c["UYVY 300x2 -> 299x2: lanes straddle the rows"] = SampleCase([(Src(UYVY, 300, 2, 101), 299, 2)])
    c["NV12 64x48 -> 37x29: two workgroups, one pixel in the last lane"] = SampleCase([(Src(NV12, 64, 48, 102), 37, 29)])
    c["batch of 40 in a handle of 64"] = SampleCase(_mixed(40, 1), max_frames=64, pitch_extra=48)
    c["33 of 40 frames set"] = SampleCase(_mixed(33, 2), max_frames=40)
    c["NV12 1920x1080 -> 80x24"] = SampleCase([(Src(NV12, 1920, 1080, 103), 80, 24)])
    _sample_cases = c
    return c


def image_buffer(case, base=None):
    """-> (guard-filled buffer, byte index of image 0: a 16-byte boundary of the address the bytes will live at, pitch)"""
    pitch = case.pitch()
    buf = np.full(64 + 16 + len(case.items) * pitch + 256, FILL, dtype=np.uint8)
    start = 64 + (-((buf.ctypes.data if base is None else base) + 64)) % 16
    return buf, start, pitch


def check_images(name, case, buf, start, pitch):
    assert (buf[:start] == FILL).all(), f"{name}: a store in front of the first image"
    for i, want in enumerate(case.expected()):
        nb = want.size
        got = buf[start + i * pitch:start + i * pitch + nb]
        if not np.array_equal(got, want.reshape(-1)):
            k = int(np.argmax(got != want.reshape(-1)))
            raise AssertionError(f"{name} frame {i}: byte {k} (pixel {k // 3} of {nb // 3}) is {int(got[k])}, restatement {int(want.reshape(-1)[k])}")
        assert (buf[start + i * pitch + nb:start + (i + 1) * pitch] == FILL).all(), f"{name} frame {i}: a store beyond the image"
    assert (buf[start + len(case.items) * pitch:] == FILL).all(), f"{name}: a store past the last image"


def emu_run(case):
    """-> (buffer, start, pitch) of the sampled pass under the emulator"""
    keep = [host_copy(i[0]) for i in case.items]
    n = len(case.items)
    srcs = (CSource * n)(*[i[0].c_source(k[1]) for i, k in zip(case.items, keep)])
    frames = (Frame * n)(*case.frames())
    buf, start, pitch = image_buffer(case)
    rc = emulator().emu_yuv_run(C.cast(srcs, C.c_void_p), C.cast(frames, C.c_void_p), n, case.max_frames, buf.ctypes.data + start, pitch)
    assert rc == 0, f"refused ({rc})"
    return buf, start, pitch


# ---- whole conversion: cases ----------------------------------------------------------------------------------------------------
class WholeCase:
    """one source through convert: the destination `dst_off` bytes behind a 16-byte boundary, rows rgb_stride apart (0: tight)"""

    def __init__(self, src, dst_off=0, rgb_stride=0):
        self.src, self.dst_off, self.rgb_stride = src, dst_off, rgb_stride

    def row_stride(self):
        return self.rgb_stride or 3 * self.src.width


_whole_cases = None


def whole_cases():
    """{format: {name: WholeCase}}: widths 2, 6, 14, 16, 18 (15 too for the planar formats) x heights 2, 4 (3 too), every
    destination alignment 0..3 with tight and padded rows, source bases and strides that are no multiples of 4"""
    global _whole_cases
    if _whole_cases is not None:
        return _whole_cases
    out = {}
    for fmt in FORMATS:
        c, k = {}, 0
        widths = (2, 6, 14, 15, 16, 18) if fmt in PLANAR else (2, 6, 14, 16, 18)
        heights = (2, 3, 4) if fmt in PLANAR else (2, 4)
        for w in widths:
            for h in heights:
                pad = (k // 4) % 2
                c[f"{w}x{h} dst +{k % 4} {'padded' if pad else 'tight'}"] = WholeCase(Src(fmt, w, h, 200 + 40 * fmt + k, extremes=True), k % 4,
                                                                                         3 * w + 5 if pad else 0)
                k += 1
        w, h = (15, 3) if fmt in PLANAR else (14, 4)
        for off in range(4):
            for stride in (0, 3 * 18 + 1, 3 * 18 + 4):  # tight; padded so that the rows' alignments differ; padded and alike
                c[f"18x4 dst +{off} rgb_stride {stride}"] = WholeCase(Src(fmt, 18, 4, 300 + fmt), off, stride)
            c[f"{w}x{h} dst +{off} tight"] = WholeCase(Src(fmt, w, h, 310 + fmt), off, 0)
        # source bases and strides that are no multiples of 4 (and of 2): the unaligned loads
        tight = [YR.row_bytes(fmt, p, 18) for p in range(YR.planes_of(fmt))] + [0, 0]
        for j, offs in enumerate(((1, 3, 2), (2, 1, 3), (0, 0, 0))):
            strides = tuple(t + (1, 3, 2)[(j + p) % 3] if t else 0 for p, t in enumerate(tight[:3]))
            c[f"18x4 source bases +{offs} strides {strides}"] = WholeCase(Src(fmt, 18, 4, 320 + fmt + j, strides=strides, offs=offs), j, 0)
        out[fmt] = c
    _whole_cases = out
    return out


def whole_buffer(case, base=None):
    """-> (guard-filled buffer, byte index of the image, bytes the image spans)"""
    span = (case.src.height - 1) * case.row_stride() + 3 * case.src.width
    buf = np.full(64 + 16 + 4 + span + 128, FILL, dtype=np.uint8)
    start = 64 + (-((buf.ctypes.data if base is None else base) + 64)) % 16 + case.dst_off
    return buf, start, span


def check_whole(name, src, buf, start, row_stride):
    """the image of src at buf[start:], rows row_stride apart; everything else still the guard"""
    want = src.whole()
    h, w = want.shape[:2]
    assert (buf[:start] == FILL).all(), f"{name}: a store in front of the image"
    for y in range(h):
        row = buf[start + y * row_stride:start + y * row_stride + 3 * w]
        if not np.array_equal(row, want[y].reshape(-1)):
            k = int(np.argmax(row != want[y].reshape(-1)))
            raise AssertionError(f"{name}: row {y} byte {k} (pixel {k // 3}) is {int(row[k])}, restatement {int(want[y].reshape(-1)[k])}")
        end = start + (y + 1) * row_stride if y + 1 < h else buf.size
        assert (buf[start + y * row_stride + 3 * w:end] == FILL).all(), f"{name}: a store behind the {3 * w} bytes of row {y}"


def emu_convert(case):
    keep, addr = host_copy(case.src)
    buf, start, _ = whole_buffer(case)
    s = case.src.c_source(addr)
    rc = emulator().emu_yuv_convert(C.byref(s), buf.ctypes.data + start, case.rgb_stride)
    assert rc == 0, f"refused ({rc})"
    return buf, start


def whole_batch():
    """sources of every format and several sizes for one run_whole"""
    return [i[0] for i in _mixed(12, 3)] + [Src(I420, 15, 3, 400), Src(UYVY, 18, 4, 401, strides=(39, 0, 0), offs=(1, 0, 0))]
