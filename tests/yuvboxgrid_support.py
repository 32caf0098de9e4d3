"""Support of the averaged grid-tile tests (libasciichat_yuvboxgrid.so): the one case table the emulated and the GPU tests share
-- composites over the test sources of yuv_support.py, built with yuvgrid_support's Slot / Comp --, the kernel under the CPU
emulator at a segment width of the caller's choice (tests/hipemu/yuvboxgrid_emu_driver.cpp), yuvboxgrid.c itself over the mock
HIP runtime, and the refusals.  Expected tiles come from tests/yuvbox_ref.py (box_ref over yuv_ref), the slab's layout from
tests/yuvgrid_ref.py; the guard-filled slab and its check are yuvgrid_support's.  TESTS ONLY."""
import ctypes as C
import os

import numpy as np

import emubuild
import orc
import yuv_ref as YR
import yuv_support as YS
import yuvbox_ref as BR
import yuvbox_support as BS
import yuvgrid_ref as GR
import yuvgrid_support as GS
from achip_ctypes import Composite

FILL = YS.FILL
I420, NV12, YUYV, UYVY = YS.I420, YS.NV12, YS.YUYV, YS.UYVY
FORMATS, PLANAR, PACKED = YS.FORMATS, YS.PLANAR, YR.PACKED
INVALID = 86
MAX_W, MAX_H, MAX_TILE = 3840, 2160, 8192
NO_SPLIT = 0
SEG_WIDTHS = (NO_SPLIT, 256, 4)  # what the CPU tests run every case at: no split, a candidate, and a box a segment
CANDIDATES = (NO_SPLIT, 1024, 512, 256)  # what the shipped width is chosen among
HEADERS = ("yuvboxgrid_kernels.hpp", "yuvboxgrid.h", "yuvbox_kernels.hpp", "yuvbox.h", "yuvgrid_math.h", "yuv_math.h", "asciichat_yuvboxgrid.h",
           "asciichat_yuvbox.h", "asciichat_yuv.h", "achip_desc.h", "achip_types.h")

Slot, Comp, single, slab, check_slab, check_rewrite, place_on_host, Placed, Trial = (GS.Slot, GS.Comp, GS.single, GS.slab, GS.check_slab,
                                                                                     GS.check_rewrite, GS.place_on_host, GS.Placed, GS.Trial)

_emu = None


def emulator():
    global _emu
    if _emu is None:
        drv = os.path.join(emubuild.EMU_DIR, "yuvboxgrid_emu_driver.cpp")
        assert os.path.exists(drv), "tests/hipemu/yuvboxgrid_emu_driver.cpp is missing: the emulator driver of libasciichat_yuvboxgrid.so"
        L = C.CDLL(emubuild.shared_library("libyuvboxgrid_emu.so", "yuvboxgrid_emu_driver.cpp", HEADERS))
        vp, ci, u32 = C.c_void_p, C.c_int, C.c_uint32
        L.emu_yuvboxgrid_seg_cols.restype = u32
        L.emu_yuvboxgrid_seg_cols.argtypes = []
        L.emu_yuvboxgrid_set_check.restype = ci
        L.emu_yuvboxgrid_set_check.argtypes = [vp, vp, ci, ci, u32, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(C.c_char_p)]
        L.emu_yuvboxgrid_layout.restype = C.c_int64
        L.emu_yuvboxgrid_layout.argtypes = [vp, vp, ci, ci, u32, vp, vp, vp, vp, vp, vp, C.POINTER(u32), C.POINTER(u32)]
        L.emu_yuvboxgrid_run.restype = ci
        L.emu_yuvboxgrid_run.argtypes = [vp, vp, ci, ci, u32, vp, ci]
        L.emu_yuvboxgrid_composites.restype = ci
        L.emu_yuvboxgrid_composites.argtypes = [vp, vp, ci, ci, vp, vp]
        _emu = L
    return _emu


class BoxGridCase(GS.GridCase):
    """a yuvgrid_support.GridCase whose expected tiles are the box averages of the whole conversions (tests/yuvbox_ref.py)"""

    def expected(self):
        if self._expected is None:
            self._expected = [BR.image(t.source.ref, t.tile_w, t.tile_h) for t in self.tiles]
            for e in self._expected:
                e.setflags(write=False)
        return self._expected


# ---- the cut of a row, said again (independent of yuvboxgrid.h) ---------------------------------------------------------------
def bounds(src, out, i):
    lo, hi = i * src // out, (i + 1) * src // out
    return lo, max(hi, lo + 1)


def segments(src_w, tile_w, seg_out):
    """-> [(xa, xb, first source column rounded down to four, the column behind the last)] of a row cut every seg_out boxes"""
    out = []
    for xa in range(0, tile_w, seg_out):
        xb = min(xa + seg_out, tile_w)
        out.append((xa, xb, bounds(src_w, tile_w, xa)[0] & ~3, bounds(src_w, tile_w, xb - 1)[1]))
    return out


# ---- the kernel under the emulator ------------------------------------------------------------------------------------------------
def _args(case, p):
    return C.cast(p.comp_ptrs, C.c_void_p), C.cast(p.nine_ptrs, C.c_void_p), len(case.comps), case.max_tiles


def emu_run(case, seg=NO_SPLIT, host=False, whole=False):
    """-> (buffer, start, Placed) of the pass under the emulator at segment width seg (host: yuvboxgrid.h's host walk in the
    kernel's place)"""
    p = place_on_host(case, whole)
    buf, start = slab(case)
    rc = emulator().emu_yuvboxgrid_run(*_args(case, p), seg, buf.ctypes.data + start, 1 if host else 0)
    assert rc == 0, f"refused ({rc})"
    return buf, start, p


def emu_layout(case, p, seg):
    """-> dict(bytes, at, first_wg, segs, seg_out, cols, slices, workgroups, stage_cols) as yuvboxgrid.h lays the set out"""
    n = max(1, case.max_tiles)
    at, first, segs, seg_out, cols_of, slices = (C.c_uint64 * n)(), *[(C.c_uint32 * n)() for _ in range(5)]
    wgs, cols = C.c_uint32(), C.c_uint32()
    total = emulator().emu_yuvboxgrid_layout(*_args(case, p), seg, C.cast(at, C.c_void_p), C.cast(first, C.c_void_p), C.cast(segs, C.c_void_p),
                                             C.cast(seg_out, C.c_void_p), C.cast(cols_of, C.c_void_p), C.cast(slices, C.c_void_p), C.byref(wgs),
                                             C.byref(cols))
    assert total >= 0, "refused"
    k = len(case.tiles)
    return dict(bytes=total, at=list(at)[:k], first_wg=list(first)[:k], segs=list(segs)[:k], seg_out=list(seg_out)[:k], cols=list(cols_of)[:k], slices=list(slices)[:k],
                workgroups=wgs.value,
                stage_cols=cols.value)


def emu_composites(case, p, tiles_address):
    out = (Composite * len(case.comps))()
    rc = emulator().emu_yuvboxgrid_composites(*_args(case, p), tiles_address, C.cast(out, C.c_void_p))
    assert rc == 0, f"refused ({rc})"
    return [out[i] for i in range(len(case.comps))]


# ---- the cases ------------------------------------------------------------------------------------------------------------------
MIXED = "mixed set: composites of 9, 4 and 1 slots, four formats, four source sizes, an RGB24 slot, an empty slot, max_tiles 20"
RATIOS_NOT_READ = "NV12 16x8 -> tile 5x3 with ratios no sampler would take"
_cases = None


def _padded(fmt, w, pad):
    return tuple(YR.row_bytes(fmt, k, w) + pad if k < YR.planes_of(fmt) else 0 for k in range(3))


def mixed_set(seed=700, shift=0):
    """three composites; another seed and shift: the same geometry over other contents in other formats (another tick)"""
    sizes = [(64, 48), (30, 18), (16, 8), (300, 6)]
    srcs = [YS.Src(FORMATS[(i + shift) % 4], *sizes[(i + i // 4) % 4], seed + i, offs=(i % 4, (i + 1) % 4, (i + 2) % 4)) for i in range(9)]
    nine_tiles = [(20, 15), (7, 4), (5, 3), (19, 2), None, (1, 1), None, (9, 11), (13, 6)]
    slots = []
    for k, size in enumerate(nine_tiles):
        if k == 4:
            slots.append(Slot(orc.frame_hash_noise(33, 21, seed + 40), 16, 12, 22, 18))  # RGB24: left as it stands
        elif size is None:
            slots.append(None)  # empty
        else:
            slots.append(Slot(srcs[k], size[0], size[1], (k % 3) * 20, (k // 3) * 16))
    nine = Comp((60, 48), (3, 3), (20, 16), slots)
    four = Comp((40, 24), (2, 2), (20, 12), [Slot(srcs[k], *t, (i % 2) * 20, (i // 2) * 12) for i, (k, t) in
                                            enumerate(((0, (20, 12)), (3, (17, 5)), (2, (8, 8)), (8, (20, 3))))])
    one = Comp((24, 10), (1, 1), (24, 10), [Slot(srcs[1], 24, 10)])
    return BoxGridCase([nine, four, one], max_tiles=20)


def cases():
    global _cases
    if _cases is not None:
        return _cases
    c = {}
    for fmt in FORMATS:
        n = YR.NAMES[fmt]
        planar = fmt in PLANAR
        # columns [0,2) [2,5) [5,7) [7,10): two edges split a chroma pair; rows [0,1) [1,3) [3,4) [4,6): boxes share chroma rows
        c[f"{n} 10x6 -> tile 4x4 box edges inside chroma blocks"] = BoxGridCase([single(YS.Src(fmt, 10, 6, 30 + fmt), 4, 4)])
        wide = 1031 if planar else 1030
        c[f"{n} {wide}x3 -> tile 7x2 a second group per lane, segments start off a multiple of four"] = \
            BoxGridCase([single(YS.Src(fmt, wide, 3 if planar else 2, 200 + fmt), 7, 2)])
        c[f"{n} 3840x2 -> tile 80x1 the widest source"] = BoxGridCase([single(YS.Src(fmt, MAX_W, 2, 100 + fmt), 80, 1)])
        c[f"{n} 4x2160 -> tile 1x1 the tallest source"] = BoxGridCase([single(YS.Src(fmt, 4, MAX_H, 90 + fmt), 1, 1)])
        up = (3, 2) if planar else (4, 2)
        c[f"{n} {up[0]}x{up[1]} -> tile 7x5 upscale: every box one pixel"] = BoxGridCase([single(YS.Src(fmt, *up, 190 + fmt), 7, 5)])
        c[f"{n} 600x4 -> tile 2x2 saturating white: sums pass 16 bits"] = BoxGridCase([single(BS.Flat(fmt, 600, 4, BS.WHITE, 80 + fmt), 2, 2)])
        for off in range(4):  # every plane `off` bytes behind a 16-byte boundary, strides padded by a multiple of 4
            c[f"{n} 20x6 -> tile 5x3 planes +{off} strides +4"] = \
                BoxGridCase([single(YS.Src(fmt, 20, 6, 60 + fmt, strides=_padded(fmt, 20, 4), offs=(off,) * 3), 5, 3)])
        c[f"{n} 20x6 -> tile 5x3 planes +0 strides +1"] = BoxGridCase([single(YS.Src(fmt, 20, 6, 70 + fmt, strides=_padded(fmt, 20, 1)), 5, 3)])
    for fmt in PLANAR:
        for w in (9, 10, 11):
            c[f"{YR.NAMES[fmt]} {w}x4 -> tile 3x2 width 4k+{w % 4}"] = BoxGridCase([single(YS.Src(fmt, w, 4, 170 + fmt + w), 3, 2)])
    c[RATIOS_NOT_READ] = BoxGridCase([single(YS.Src(NV12, 16, 8, 210), 5, 3, ratios=(0xFFFFFFFF, 0))])
    c[MIXED] = mixed_set()
    _cases = c
    return c


# ---- the host side (yuvboxgrid.c) through its C interface: the real library on a GPU, or the mock build without one ------------
NAMES = ("device_count", "last_error", "create", "set", "tiles_bytes", "run", "composites", "destroy")


def bind(L):
    vp, ci = C.c_void_p, C.c_int
    for name, res, args in (("device_count", ci, []), ("last_error", C.c_char_p, []), ("create", ci, [C.POINTER(vp), ci]),
                            ("set", ci, [vp, vp, vp, ci, vp]), ("tiles_bytes", C.c_size_t, [vp]), ("run", ci, [vp, vp, vp]),
                            ("composites", ci, [vp, vp, vp]), ("destroy", None, [vp])):
        fn = getattr(L, "asciichat_yuvboxgrid_" + name)
        fn.restype, fn.argtypes = res, args
    return L


_mock = None


def mock_library():
    """yuvboxgrid.c as it stands over the mock HIP runtime (tests/mockhip/mock_hip.c: device memory is host memory), its launcher
    the emulator's (yuvboxgrid_emu_driver.cpp): the handle's own code, at the segment width it ships with, without a GPU"""
    global _mock
    if _mock is None:
        import subprocess
        import mockgpu
        so = os.path.join(emubuild.OUT_DIR, "libyuvboxgrid_mock.so")
        srcs = [os.path.join(emubuild.CSRC, "yuvboxgrid.c"), os.path.join(mockgpu.MOCK, "mock_hip.c"),
                os.path.join(emubuild.EMU_DIR, "yuvboxgrid_emu_driver.cpp")]
        for s in srcs:
            assert os.path.exists(s), f"{s} is missing"
        deps = srcs + [emubuild._header(h) for h in ("hip_emu.h", "gfx950_ops.hpp") + HEADERS]
        if not (os.path.exists(so) and all(os.path.getmtime(d) <= os.path.getmtime(so) for d in deps)):
            os.makedirs(emubuild.OUT_DIR, exist_ok=True)
            tag = ".%d" % os.getpid()
            objs = []
            for src in srcs[:2]:
                objs.append(os.path.join(emubuild.OUT_DIR, "yuvboxgrid_" + os.path.basename(src) + tag + ".o"))
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
    """asciichat_yuvboxgrid_* of a bound library, return codes as they come"""

    def __init__(self, L, max_tiles, stream=0):
        self.L, self.h, self.stream = L, C.c_void_p(), stream
        rc = L.asciichat_yuvboxgrid_create(C.byref(self.h), max_tiles)
        assert rc == 0, (rc, self.error())

    def error(self):
        return self.L.asciichat_yuvboxgrid_last_error().decode()

    def set(self, p, n=None):
        return self.L.asciichat_yuvboxgrid_set(self.h, C.cast(p.comp_ptrs, C.c_void_p), C.cast(p.nine_ptrs, C.c_void_p),
                                               len(p.comps) if n is None else n, self.stream)

    def tiles_bytes(self):
        return int(self.L.asciichat_yuvboxgrid_tiles_bytes(self.h))

    def run(self, tiles):
        return self.L.asciichat_yuvboxgrid_run(self.h, tiles, self.stream)

    def composites(self, tiles, n, cls=Composite):
        out = (cls * n)()
        rc = self.L.asciichat_yuvboxgrid_composites(self.h, tiles, C.cast(out, C.c_void_p))
        return rc, [out[i] for i in range(n)]

    def close(self):
        if self.h:
            self.L.asciichat_yuvboxgrid_destroy(self.h)
            self.h = C.c_void_p()


def refusal_case():
    """two composites, three YUV slots: composite 1 has a YUV slot, an RGB24 slot and a YUV slot, n_src 3"""
    one = Comp((12, 4), (3, 1), (6, 4), [Slot(YS.Src(NV12, 16, 8, 951), 5, 3), Slot(orc.frame_hash_noise(8, 6, 952), 6, 4, 6, 0),
                                        Slot(YS.Src(UYVY, 16, 8, 953), 6, 4, 12, 0)])
    return BoxGridCase([single(YS.Src(I420, 16, 8, 950, extremes=True), 5, 3), one], max_tiles=3)


def check_refusals(L, place, new_slab, stream=0, synchronize=lambda: None):
    """Every refusal of include/asciichat_yuvboxgrid.h at its limit -- the last accepted value passes, the first refused is
    refused with ERR_INVALID_PARAM --, that a refused call launches nothing and leaves the handle as it was, and that the handle
    still works.  place(case) -> Placed at addresses L's kernel can read; new_slab(case) -> (address of tile 0, read: () ->
    (buffer, start))"""
    case = refusal_case()
    p = place(case)
    n = len(case.comps)
    tiles, read = new_slab(case)
    # create
    for bad in (0, -1, 4097):
        h = C.c_void_p(1)
        assert L.asciichat_yuvboxgrid_create(C.byref(h), bad) == INVALID and not h.value and str(bad) in L.asciichat_yuvboxgrid_last_error().decode()
    assert L.asciichat_yuvboxgrid_create(None, 3) == INVALID
    for good in (1, 4096):
        Handle(L, good).close()
    # a handle that is not one of this library's
    junk = np.zeros(512, dtype=np.uint8)
    for address in (junk.ctypes.data, None):
        hh = Handle.__new__(Handle)
        hh.L, hh.h, hh.stream = L, C.c_void_p(address), stream
        assert hh.set(p) == INVALID and hh.run(tiles) == INVALID and hh.composites(tiles, n)[0] == INVALID and hh.tiles_bytes() == 0
        assert "not a handle" in hh.error()

    g = Handle(L, 3, stream)
    try:
        # before any set
        assert g.run(tiles) == INVALID and "nothing is set" in g.error()
        assert g.composites(tiles, n)[0] == INVALID and g.tiles_bytes() == 0

        def refused(change=None, count=None, named=None):
            t = Trial(p)
            if change:
                change(t)
                t.link()
            rc = g.set(t, count)
            assert rc in (0, INVALID), (rc, g.error())
            if rc and named:
                assert named in g.error(), g.error()
            return rc == INVALID

        def slot(c, k, **kw):
            def change(t):
                for f, v in kw.items():
                    setattr(t.comps[c].s[k], f, v)
            return change

        def source(c, k, **kw):
            def change(t):
                for f, v in kw.items():
                    setattr(t.nines[c][k], f, v)
            return change

        def comp(c, **kw):
            def change(t):
                for f, v in kw.items():
                    setattr(t.comps[c], f, v)
            return change

        def both(*changes):
            def change(t):
                for ch in changes:
                    ch(t)
            return change

        def null_entry(which, c):
            def change(t):
                t.link()
                getattr(t, which)[c] = None
                t.link = lambda: None
            return change

        def sized(c, k, w, h):
            """source and slot at w x h (the planes are not read: the set is refused, or replaced before any run)"""
            return both(source(c, k, width=w, height=h), slot(c, k, src_w=w, src_h=h))

        # the number of composites: 0 and max_tiles + 1 (a handle of 3 takes 3 composites, not 4)
        assert refused(count=0) and refused(count=-1) and not refused(count=1) and not refused(count=2)
        three = Trial(p)
        three.comps.append(type(p.comps[0]).from_buffer_copy(bytes(p.comps[0])))
        three.nines.append((type(p.nines[0][0]) * 9)())  # (a third composite without YUV slots)
        three.link()
        assert g.set(three, 3) == 0
        three.comps.append(three.comps[2]), three.nines.append(three.nines[2])
        three.link()
        assert g.set(three, 4) == INVALID and "max_tiles" in g.error()
        # NULL arrays and entries
        assert L.asciichat_yuvboxgrid_set(g.h, None, C.cast(p.nine_ptrs, C.c_void_p), n, stream) == INVALID
        assert L.asciichat_yuvboxgrid_set(g.h, C.cast(p.comp_ptrs, C.c_void_p), None, n, stream) == INVALID
        assert refused(null_entry("comp_ptrs", 1), named="composite 1") and refused(null_entry("nine_ptrs", 0), named="composite 0")
        # n_src: 0..9 (composite 0 without its YUV source has no YUV slot: any n_src in range passes)
        no_yuv = source(0, 0, plane=(C.c_void_p * 3)())
        for v, want in ((-1, True), (0, False), (9, False), (10, True)):
            assert refused(both(no_yuv, comp(0, n_src=v)), named="composite 0") == want, v
        # a YUV slot at or behind n_src, and one that is not placed
        assert not refused(comp(1, n_src=3)) and refused(comp(1, n_src=2), named="composite 1 slot 2") and not refused(comp(1, n_src=9))
        assert refused(slot(1, 2, src=None), named="composite 1 slot 2") and not refused(slot(1, 2, src=1))
        # an RGB24 slot is not looked at
        assert not refused(slot(1, 1, src=None, src_w=-5, tile_w=0, x_ratio=0xFFFFFFFF))
        # the source itself (yuv_source_check), and its size against the slot's
        assert refused(source(1, 0, format=4), named="composite 1 slot 0") and refused(source(1, 2, width=15))
        assert refused(source(1, 0, stride=(C.c_int32 * 3)(15, 0, 0))) and not refused(source(1, 0, stride=(C.c_int32 * 3)(16, 16, 0)))
        for f in ("src_w", "src_h"):
            base = getattr(p.comps[1].s[0], f)
            assert refused(slot(1, 0, **{f: base - 1})) and refused(slot(1, 0, **{f: base + 1})) and not refused(slot(1, 0, **{f: base}))
        # yuvbox's limit on a source: 3840 x 2160 passes, 3841 and 2161 do not
        assert not refused(sized(1, 0, MAX_W, MAX_H))
        assert refused(sized(1, 0, MAX_W + 1, 8), named="composite 1 slot 0") and "3840" in g.error()
        assert refused(sized(0, 0, 16, MAX_H + 1), named="composite 0 slot 0") and refused(sized(1, 2, MAX_W + 2, 8), named="composite 1 slot 2")
        # the tile's size: 1..8192
        for f in ("tile_w", "tile_h"):
            for v, want in ((0, True), (-1, True), (1, False), (MAX_TILE, False), (MAX_TILE + 1, True)):
                assert refused(slot(1, 0, **{f: v}), named="composite 1 slot 0") == want, (f, v)
        # the ratios are not read: values no sampler would take pass
        assert not refused(slot(1, 2, x_ratio=0xFFFFFFFF, y_ratio=0)) and not refused(slot(0, 0, x_ratio=0, y_ratio=0xFFFFFFFF))
        # more YUV slots than max_tiles (3): a fourth -- slot 1 of composite 1 given as YUV
        def fourth(t):
            C.memmove(C.addressof(t.nines[1][1]), C.addressof(t.nines[1][0]), C.sizeof(t.nines[1][0]))
            for f in ("src_w", "src_h"):
                setattr(t.comps[1].s[1], f, getattr(t.comps[1].s[0], f))
        assert refused(fourth, named="max_tiles")
        g4 = Handle(L, 4, stream)
        t = Trial(p)
        fourth(t)
        assert g4.set(t) == 0 and g4.tiles_bytes() == GR.layout([(5, 3), (5, 3), (6, 4), (6, 4)])[1]
        g4.close()
        g1 = Handle(L, 1, stream)  # and as many composites at the most
        assert g1.set(p, 1) == 0 and g1.set(p, 2) == INVALID and g1.tiles_bytes() == 128
        g1.close()

        # a refused set leaves the set before: its offsets, its tile count, its descriptors
        assert g.set(p) == 0
        before = g.tiles_bytes(), [bytes(c) for c in g.composites(tiles, n)[1]]
        assert before[0] == case.layout()[1] and len(case.tiles) == 3
        assert refused(count=1, change=slot(0, 0, tile_w=0)) and refused(comp(1, n_src=2)) and refused(count=0)
        assert refused(sized(1, 0, MAX_W + 1, 8)) and refused(fourth)
        assert (g.tiles_bytes(), [bytes(c) for c in g.composites(tiles, n)[1]]) == before
        # the slab and the output
        assert g.run(None) == INVALID and g.run(tiles + 8) == INVALID and g.run(tiles + 1) == INVALID
        assert g.composites(None, n)[0] == INVALID and g.composites(tiles + 4, n)[0] == INVALID
        assert L.asciichat_yuvboxgrid_composites(g.h, tiles, None) == INVALID and "no descriptors" in g.error()
        synchronize()
        buf, start = read()
        assert (buf == FILL).all(), "a refused call launched something"
        # and the handle still works, with the set it was left with
        assert g.run(tiles) == 0
        synchronize()
        buf, start = read()
        check_slab("after the refusals", case, buf, start)
        rc, out = g.composites(tiles, n, type(p.comps[0]))
        assert rc == 0
        check_rewrite("after the refusals", case, p.comps, out, tiles)
    finally:
        g.close()
