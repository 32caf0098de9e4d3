"""Support of the fused YUV box-average tests: the kernel of libasciichat_yuvbox.so under the CPU emulator
(tests/hipemu/yuvbox_emu_driver.cpp), yuvbox.c itself over the mock HIP runtime, and the one case table the emulated and the GPU
tests share -- sources from yuv_support.Src (planes at chosen misalignments, strides padded with noise), guard-filled
destinations, expectations from tests/yuvbox_ref.py.  TESTS ONLY."""
import ctypes as C
import os

import numpy as np

import emubuild
import yuv_ref as YR
import yuv_support as YS
import yuvbox_ref as BR
from achip_ctypes import Frame

FILL = YS.FILL
I420, NV12, YUYV, UYVY = YS.I420, YS.NV12, YS.YUYV, YS.UYVY
FORMATS, PLANAR, PACKED = YS.FORMATS, YS.PLANAR, YR.PACKED
FLIP_X, FLIP_Y = YR.FLIP_X, YR.FLIP_Y
CSource = YS.CSource
INVALID, NOT_SUPPORTED = 86, 30
MAX_W, MAX_H, MAX_OUT = 3840, 2160, 16384
HEADERS = ("yuvbox_kernels.hpp", "yuvbox.h", "yuv_math.h", "asciichat_yuvbox.h", "asciichat_yuv.h", "achip_desc.h", "achip_types.h")

_emu = None


def emulator():
    global _emu
    if _emu is None:
        drv = os.path.join(emubuild.EMU_DIR, "yuvbox_emu_driver.cpp")
        assert os.path.exists(drv), "tests/hipemu/yuvbox_emu_driver.cpp is missing: the emulator driver of libasciichat_yuvbox.so"
        L = C.CDLL(emubuild.shared_library("libyuvbox_emu.so", "yuvbox_emu_driver.cpp", HEADERS))
        vp, ci = C.c_void_p, C.c_int
        L.emu_yuvbox_set_check.restype = ci
        L.emu_yuvbox_set_check.argtypes = [vp, vp, ci, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(C.c_char_p)]
        L.emu_yuvbox_run.restype = ci
        L.emu_yuvbox_run.argtypes = [vp, vp, ci, ci, vp, C.c_uint64, ci]
        L.emu_yuvbox_downscale.restype = ci
        L.emu_yuvbox_downscale.argtypes = [C.POINTER(CSource), vp, ci, ci, ci, ci]
        _emu = L
    return _emu


# ---- test sources ---------------------------------------------------------------------------------------------------------------
class Flat(YS.Src):
    """a yuv_support.Src whose every sample is (y, u, v): laid out like any other, its bytes between rows and planes noise"""

    def __init__(self, fmt, w, h, yuv, seed, strides=(0, 0, 0), offs=(0, 0, 0)):
        YS.Src.__init__(self, fmt, w, h, seed, strides, offs)
        cw, ch = YR.chroma_size(w, h)
        cshape = (h, w // 2) if fmt in PACKED else (ch, cw)
        planes, _ = YR.pack(fmt, np.full((h, w), yuv[0], np.uint8), np.full(cshape, yuv[1], np.uint8), np.full(cshape, yuv[2], np.uint8), strides)
        image = self.image.copy()
        for k, (a, p) in enumerate(zip(self.at, planes)):
            rows, row, stride = YR.plane_rows(fmt, k, h), YR.row_bytes(fmt, k, w), self.ref.strides[k]
            for r in range(rows):  # (the samples only: the padding keeps its noise)
                image[a + r * stride:a + r * stride + row] = p[r * stride:r * stride + row]
        image.setflags(write=False)
        self.image = image
        self.ref = YR.Source(fmt, w, h, [image[a:] for a in self.at], self.ref.strides)


WHITE = (255, 128, 128)  # 298 * 239 + 128 >> 8 = 278: every channel saturates


class Case:
    """items: [(Src, out_w, out_h, flips)]; the handle holds max_frames.  (items, pitch() and expected() as yuv_support's
    image_buffer and check_images read them)"""

    def __init__(self, items, max_frames=None, pitch_extra=0):
        self.items = [(i[0], i[1], i[2], i[3] if len(i) > 3 else 0) for i in items]
        self.max_frames = max_frames or len(items)
        self.pitch_extra = pitch_extra
        self._expected = None

    def frames(self, cls=Frame):
        """the descriptors achip_frame_setup makes; src stays NULL and src_stride odd: set() reads neither, nor the ratios"""
        out = []
        for s, ow, oh, fl in self.items:
            f = YS.frame(s, ow, oh, fl, cls=cls)
            f.src_stride = -7
            out.append(f)
        return out

    def expected(self):
        if self._expected is None:
            self._expected = [BR.image(s.ref, ow, oh, bool(fl & FLIP_X), bool(fl & FLIP_Y)) for s, ow, oh, fl in self.items]
            for e in self._expected:
                e.setflags(write=False)
        return self._expected

    def pitch(self):
        return (max(3 * i[1] * i[2] for i in self.items) + 127) // 128 * 128 + self.pitch_extra


def _padded(fmt, w, pad):
    """strides of every plane `pad` bytes above tight"""
    return tuple(YR.row_bytes(fmt, k, w) + pad if k < YR.planes_of(fmt) else 0 for k in range(3))


MIXED = "mixed batch: four formats, four sizes, 8 of 12 frames, a pitch with extra bytes"
DEEP_WHITE = "8x600 -> 2x2 saturating white: 300 rows a box"
_cases = None


def cases():
    global _cases
    if _cases is not None:
        return _cases
    c = {}
    for fmt in FORMATS:
        n = YR.NAMES[fmt]
        c[f"{n} 2x2 -> 1x1"] = Case([(YS.Src(fmt, 2, 2, 10 + fmt), 1, 1)])
        c[f"{n} 16x8 -> 5x3 the extremes of Y, U and V"] = Case([(YS.Src(fmt, 16, 8, 20 + fmt, extremes=True), 5, 3)])
        # columns [0,2) [2,5) [5,7) [7,10): two edges split a chroma pair; rows [0,1) [1,3) [3,4) [4,6): boxes share chroma rows
        c[f"{n} 10x6 -> 4x4 box edges inside chroma blocks"] = Case([(YS.Src(fmt, 10, 6, 30 + fmt), 4, 4)])
        c[f"{n} 6x4 -> 6x4 identity"] = Case([(YS.Src(fmt, 6, 4, 40 + fmt, extremes=True), 6, 4)])
        for fl in range(4):
            c[f"{n} 18x7 -> 5x3 flips {fl}"] = Case([(YS.Src(fmt, 18, 7, 50 + fmt), 5, 3, fl)])
        for off in range(4):  # every plane `off` bytes behind a 16-byte boundary, strides padded by a multiple of 4: off 0 aligned
            c[f"{n} 20x6 -> 5x3 planes +{off} strides +4"] = Case([(YS.Src(fmt, 20, 6, 60 + fmt, strides=_padded(fmt, 20, 4), offs=(off,) * 3), 5, 3)])
        c[f"{n} 20x6 -> 5x3 planes +0 strides +1"] = Case([(YS.Src(fmt, 20, 6, 70 + fmt, strides=_padded(fmt, 20, 1)), 5, 3)])
        c[f"{n} {DEEP_WHITE}"] = Case([(Flat(fmt, 8, 600, WHITE, 80 + fmt), 2, 2)])
        c[f"{n} 4x2160 -> 1x1"] = Case([(YS.Src(fmt, 4, 2160, 90 + fmt), 1, 1)])
        c[f"{n} 3840x2 -> 80x1 the widest stage"] = Case([(YS.Src(fmt, 3840, 2, 100 + fmt), 80, 1)])
        c[f"{n} 3840x2 -> 1x1 the widest stage"] = Case([(YS.Src(fmt, 3840, 2, 110 + fmt), 1, 1)])
    for fmt in PLANAR:
        n = YR.NAMES[fmt]
        c[f"{n} 5x3 -> 2x2 odd width and height"] = Case([(YS.Src(fmt, 5, 3, 120 + fmt), 2, 2)])
        c[f"{n} 7x5 -> 3x2 odd width and height"] = Case([(YS.Src(fmt, 7, 5, 130 + fmt, extremes=True), 3, 2)])
        c[f"{n} 1x1 -> 1x1"] = Case([(YS.Src(fmt, 1, 1, 140 + fmt), 1, 1)])
        c[f"{n} 1x5 -> 1x2"] = Case([(YS.Src(fmt, 1, 5, 150 + fmt), 1, 2)])
        c[f"{n} 5x1 -> 3x1"] = Case([(YS.Src(fmt, 5, 1, 160 + fmt), 3, 1)])
        for w in (9, 10, 11):
            c[f"{n} {w}x4 -> 3x2 width 4k+{w % 4}"] = Case([(YS.Src(fmt, w, 4, 170 + fmt + w), 3, 2)])
        c[f"{n} 3x2 -> 7x5 upscale"] = Case([(YS.Src(fmt, 3, 2, 190 + fmt), 7, 5)])
        c[f"{n} 1031x3 -> 7x2 a second group per lane"] = Case([(YS.Src(fmt, 1031, 3, 200 + fmt), 7, 2)])
    for fmt in PACKED:
        n = YR.NAMES[fmt]
        c[f"{n} 2x5 -> 1x2"] = Case([(YS.Src(fmt, 2, 5, 150 + fmt), 1, 2)])
        c[f"{n} 6x1 -> 2x1"] = Case([(YS.Src(fmt, 6, 1, 160 + fmt), 2, 1)])
        c[f"{n} 4x2 -> 9x5 upscale"] = Case([(YS.Src(fmt, 4, 2, 190 + fmt), 9, 5)])
        c[f"{n} 1030x2 -> 5x1 a second group per lane"] = Case([(YS.Src(fmt, 1030, 2, 200 + fmt), 5, 1)])
    sizes = [((16, 8), (5, 3)), ((30, 17), (7, 4)), ((64, 48), (9, 5)), ((6, 4), (1, 1))]
    items = []
    for i in range(8):
        fmt = FORMATS[(i + i // 4) % 4]
        (w, h), (ow, oh) = sizes[(i * 3) % 4]
        items.append((YS.Src(fmt, w, h, 300 + i, offs=(i % 4, (i + 1) % 4, (i + 2) % 4)), ow, oh, i % 4))
    c[MIXED] = Case(items, max_frames=12, pitch_extra=48)
    _cases = c
    return c


# ---- the kernel under the emulator -----------------------------------------------------------------------------------------------
def place_on_host(srcs, cls=CSource):
    """-> (arrays to keep alive, [source structures over 16-aligned host copies])"""
    keep = [YS.host_copy(s) for s in srcs]
    return keep, [s.c_source(k[1], cls) for s, k in zip(srcs, keep)]


def emu_run(case, host=False):
    """-> (buffer, start, pitch) of the pass under the emulator (host: the host walk of yuvbox.h in the kernel's place)"""
    keep, sources = place_on_host([i[0] for i in case.items])
    n = len(case.items)
    srcs = (CSource * n)(*sources)
    frames = (Frame * n)(*case.frames())
    buf, start, pitch = YS.image_buffer(case)
    rc = emulator().emu_yuvbox_run(C.cast(srcs, C.c_void_p), C.cast(frames, C.c_void_p), n, case.max_frames, buf.ctypes.data + start, pitch, int(host))
    assert rc == 0, f"refused ({rc})"
    return buf, start, pitch


check_images = YS.check_images  # every image the restatement's, every other byte -- in front, between, behind -- still the guard


# ---- the host side (yuvbox.c) through its C interface: the real library on a GPU, or the mock build without one -----------------
def bind(L):
    vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
    for name, res, args in (("device_count", ci, []), ("last_error", C.c_char_p, []), ("create", ci, [C.POINTER(vp), ci]),
                            ("set", ci, [vp, vp, vp, ci, vp]), ("image_pitch", sz, [vp]), ("run", ci, [vp, vp, sz, vp]),
                            ("render_frames", ci, [vp, vp, sz, vp]), ("downscale", ci, [vp, vp, ci, ci, ci, ci, vp]), ("destroy", None, [vp])):
        fn = getattr(L, "asciichat_yuvbox_" + name)
        fn.restype, fn.argtypes = res, args
    return L


_mock = None


def mock_library():
    """yuvbox.c as it stands over the mock HIP runtime (tests/mockhip/mock_hip.c: device memory is host memory), its launcher the
    emulator's (yuvbox_emu_driver.cpp): the handle's own code without a GPU"""
    global _mock
    if _mock is None:
        import subprocess
        import mockgpu
        so = os.path.join(emubuild.OUT_DIR, "libyuvbox_mock.so")
        srcs = [os.path.join(emubuild.CSRC, "yuvbox.c"), os.path.join(mockgpu.MOCK, "mock_hip.c"), os.path.join(emubuild.EMU_DIR, "yuvbox_emu_driver.cpp")]
        for s in srcs:
            assert os.path.exists(s), f"{s} is missing"
        deps = srcs + [emubuild._header(h) for h in ("hip_emu.h", "gfx950_ops.hpp") + HEADERS]
        if not (os.path.exists(so) and all(os.path.getmtime(d) <= os.path.getmtime(so) for d in deps)):
            os.makedirs(emubuild.OUT_DIR, exist_ok=True)
            tag = ".%d" % os.getpid()
            objs = []
            for src in srcs[:2]:
                objs.append(os.path.join(emubuild.OUT_DIR, os.path.basename(src) + tag + ".o"))
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
    """asciichat_yuvbox_* of a bound library, return codes as they come"""

    def __init__(self, L, max_frames, stream=0):
        self.L, self.h, self.stream = L, C.c_void_p(), stream
        rc = L.asciichat_yuvbox_create(C.byref(self.h), max_frames)
        assert rc == 0, (rc, self.error())

    def error(self):
        return self.L.asciichat_yuvbox_last_error().decode()

    def set(self, sources, frames, n=None):
        """sources, frames: lists of structures (or None for a NULL array)"""
        self._keep = (None if sources is None else (type(sources[0]) * len(sources))(*sources),
                      None if frames is None else (type(frames[0]) * len(frames))(*frames))
        count = n if n is not None else len(sources)
        return self.L.asciichat_yuvbox_set(self.h, *[C.cast(a, C.c_void_p) if a is not None else None for a in self._keep], count, self.stream)

    def pitch(self):
        return int(self.L.asciichat_yuvbox_image_pitch(self.h))

    def run(self, images, pitch):
        return self.L.asciichat_yuvbox_run(self.h, images, pitch, self.stream)

    def render_frames(self, images, pitch, n, cls=Frame):
        out = (cls * n)()
        rc = self.L.asciichat_yuvbox_render_frames(self.h, images, pitch, C.cast(out, C.c_void_p))
        return rc, [out[i] for i in range(n)]

    def close(self):
        if self.h:
            self.L.asciichat_yuvbox_destroy(self.h)
            self.h = C.c_void_p()


def changed(obj, **kw):
    c = type(obj).from_buffer_copy(bytes(obj))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def check_render_frames(case, given, out, images, pitch):
    """what asciichat_hip_box_render_frames documents, field for field"""
    for i, (f, d) in enumerate(zip(given, out)):
        assert d.src == images + i * pitch and d.comp is None, i
        assert (d.src_w, d.src_h, d.out_w, d.out_h) == (f.out_w, f.out_h, f.out_w, f.out_h), i
        assert (d.x_ratio, d.y_ratio, d.src_stride) == (65537, 65537, 3 * f.out_w), i
        assert (d.pad_left, d.pad_top) == (f.pad_left, f.pad_top) and d.ops == f.ops & ~(FLIP_X | FLIP_Y), i


def refusal_case():
    """two frames: an I420 source with the extremes and a packed one, flipped"""
    return Case([(YS.Src(I420, 16, 8, 950, extremes=True), 5, 3), (YS.Src(UYVY, 18, 6, 951), 4, 2, 3)], max_frames=2)


def check_refusals(L, place, new_images, stream=0, synchronize=lambda: None):
    """Every refusal of include/asciichat_yuvbox.h at its limit -- the last accepted value passes, the first refused is refused
    with its code --, that a refused call launches nothing and leaves the handle as it was, and that the handle still works.
    place(srcs) -> (keep, [sources at addresses L's kernel can read]); new_images(case) -> (address of image 0, pitch,
    read: () -> (buffer, start))"""
    case = refusal_case()
    keep, sources = place([i[0] for i in case.items])
    frames = case.frames(Frame)
    images, pitch, read = new_images(case)
    # create
    for bad in (0, -1, 65536):
        h = C.c_void_p(1)
        assert L.asciichat_yuvbox_create(C.byref(h), bad) == INVALID and not h.value and str(bad) in L.asciichat_yuvbox_last_error().decode()
    assert L.asciichat_yuvbox_create(None, 2) == INVALID
    for good in (1, 65535):
        Handle(L, good).close()
    # a handle that is not one of this library's
    junk = np.zeros(512, dtype=np.uint8)
    for address in (junk.ctypes.data, None):
        hh = Handle.__new__(Handle)
        hh.L, hh.h, hh.stream = L, C.c_void_p(address), stream
        assert hh.set(sources, frames) == INVALID and hh.run(images, pitch) == INVALID and hh.render_frames(images, pitch, 2)[0] == INVALID
        assert hh.pitch() == 0 and "not a handle" in hh.error()

    g = Handle(L, 2, stream)
    try:
        # before any set
        assert g.run(images, pitch) == INVALID and "nothing is set" in g.error()
        assert g.render_frames(images, pitch, 2)[0] == INVALID and g.pitch() == 0

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

        def sized(i, w, h):
            """source and descriptor i at w x h (the planes are not read: the set is refused, or replaced before any run)"""
            return dict(srcs=with_source(i, width=w, height=h), frs=with_frame(i, src_w=w, src_h=h))

        assert code() == 0
        # the arrays and their number
        assert code(frs=None, n=2) == INVALID and "required" in g.error()
        assert code(srcs=None, n=2) == INVALID
        assert code(n=0) == INVALID and code(n=-1) == INVALID and code(n=1) == 0 and code(n=2) == 0
        assert code(srcs=sources + sources[:1], frs=frames + frames[:1]) == INVALID and "max_frames" in g.error()
        # the box pass's source limit: 3840 x 2160 passes, 3841 and 2161 do not (8192 is yuv_source_check's own)
        assert code(**sized(0, MAX_W, MAX_H)) == 0
        assert code(**sized(0, MAX_W + 1, 8), named="frame 0") == INVALID and "3840" in g.error()
        assert code(**sized(0, 16, MAX_H + 1), named="frame 0") == INVALID
        assert code(**sized(1, MAX_W + 2, 6), named="frame 1") == INVALID
        # the image's size: 1..16384 a side
        for field in ("out_w", "out_h"):
            for v, want in ((0, INVALID), (-1, INVALID), (1, 0), (MAX_OUT, 0), (MAX_OUT + 1, INVALID)):
                assert code(frs=with_frame(1, **{field: v}), named="frame 1") == want, (field, v)
        # comp: refused as unsupported, nothing else is
        assert code(frs=with_frame(1, comp=1), named="frame 1") == NOT_SUPPORTED
        # the descriptor's size is the source's
        for kw in (dict(src_w=15), dict(src_w=17), dict(src_h=7), dict(src_h=9)):
            assert code(frs=with_frame(0, **kw), named="frame 0") == INVALID, kw
        # the source itself (yuv_source_check): an odd packed width, a format, a missing plane, a short stride
        assert code(**sized(1, 17, 6), named="frame 1") == INVALID and "odd width" in g.error()
        assert code(srcs=with_source(0, format=4)) == INVALID and code(srcs=with_source(0, format=NV12)) == INVALID  # (a third plane on NV12)
        assert code(srcs=with_source(1, stride=(C.c_int32 * 3)(35, 0, 0))) == INVALID and code(srcs=with_source(1, stride=(C.c_int32 * 3)(36, 0, 0))) == 0
        # x_ratio, y_ratio, src and src_stride are not read; paddings, tints and the other bits of ops pass through
        assert code(frs=with_frame(0, x_ratio=0xFFFFFFFF, y_ratio=0, src=1, src_stride=-9, pad_left=3, pad_top=2, ops=3 | 4 | 0x112233 << 8)) == 0

        # a refused set leaves the set before: its pitch, its descriptors, its sources
        assert code() == 0
        before = g.pitch(), [bytes(f) for f in g.render_frames(images, pitch, 2)[1]]
        assert before[0] == 128
        assert code(frs=with_frame(0, out_w=0)) == INVALID and code(frs=with_frame(1, comp=1)) == NOT_SUPPORTED and code(n=0) == INVALID
        assert code(**sized(0, MAX_W + 1, 8)) == INVALID and code(frs=None, n=2) == INVALID
        assert (g.pitch(), [bytes(f) for f in g.render_frames(images, pitch, 2)[1]]) == before
        # the images' place
        assert g.run(None, pitch) == INVALID and g.run(images + 8, pitch) == INVALID and g.run(images, pitch + 8) == INVALID
        assert g.run(images, 32) == INVALID and "below" in g.error()  # below the largest image's 45 bytes
        assert g.render_frames(None, pitch, 2)[0] == INVALID and g.render_frames(images, 32, 2)[0] == INVALID
        assert L.asciichat_yuvbox_render_frames(g.h, images, pitch, None) == INVALID and "no descriptors" in g.error()
        # downscale
        one = sources[0]
        down = lambda s, dst, w, h: L.asciichat_yuvbox_downscale(C.byref(s) if s is not None else None, dst, w, h, 0, 0, stream)  # noqa: E731
        assert down(None, images, 5, 3) == INVALID and down(one, None, 5, 3) == INVALID
        assert down(one, images, 0, 3) == INVALID and down(one, images, 5, MAX_OUT + 1) == INVALID
        assert down(changed(one, width=MAX_W + 1), images, 5, 3) == INVALID and down(changed(sources[1], width=17), images, 5, 3) == INVALID
        synchronize()
        buf, start = read()
        assert (buf == FILL).all(), "a refused call launched something"
        # and the handle still works, with the set it was left with
        assert g.run(images, pitch) == 0
        synchronize()
        buf, start = read()
        check_images("after the refusals", case, buf, start, pitch)
        rc, out = g.render_frames(images, pitch, 2)
        assert rc == 0
        check_render_frames(case, frames, out, images, pitch)
    finally:
        g.close()
    return keep
