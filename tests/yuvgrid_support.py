"""Support of the grid-tile tests (libasciichat_yuvgrid.so): composites built by hand or by achip_composite_setup over the test
sources of yuv_support.py, the one case table the emulated and the GPU tests share, the guard-filled tile slab, and the kernel
under the CPU emulator (tests/hipemu/yuvgrid_emu_driver.cpp).  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu
import emubuild
import orc
import yuv_ref as YR
import yuv_support as YS
import yuvgrid_ref as GR
from achip_ctypes import MODE_CAPS, Composite

FILL = YS.FILL
I420, NV12, YUYV, UYVY = YS.I420, YS.NV12, YS.YUYV, YS.UYVY
PLACED = 0x10  # the src of a YUV slot as the caller leaves it: not NULL, never read

_emu = None


def emulator():
    global _emu
    if _emu is None:
        L = C.CDLL(emubuild.shared_library("libyuvgrid_emu.so", "yuvgrid_emu_driver.cpp",
                                           ("yuvgrid_kernels.hpp", "yuvgrid.h", "yuvgrid_math.h", "yuv_math.h", "asciichat_yuv.h", "achip_desc.h",
                                            "achip_types.h")))
        vp, ci = C.c_void_p, C.c_int
        L.emu_yuvgrid_layout.restype = C.c_int64
        L.emu_yuvgrid_layout.argtypes = [vp, vp, ci, ci, vp]
        L.emu_yuvgrid_run.restype = ci
        L.emu_yuvgrid_run.argtypes = [vp, vp, ci, ci, vp, ci]
        L.emu_yuvgrid_composites.restype = ci
        L.emu_yuvgrid_composites.argtypes = [vp, vp, ci, ci, vp, vp]
        _emu = L
    return _emu


_host = None


def host_lib():
    """achip_host.c alone as a small library (achip_composite_setup, achip_frame_setup): what the case table needs of the host
    code, built in a second, so that the GPU tests do not build the kernel emulator to collect their cases"""
    global _host
    if _host is None:
        import os
        import subprocess
        src = os.path.join(emubuild.CSRC, "achip_host.c")
        so = os.path.join(emubuild.OUT_DIR, "libachip_host_only.so")
        deps = [src, os.path.join(emubuild.INC, "achip_host.h"), os.path.join(emubuild.INC, "achip_types.h")]
        if not (os.path.exists(so) and all(os.path.getmtime(d) <= os.path.getmtime(so) for d in deps)):
            os.makedirs(emubuild.OUT_DIR, exist_ok=True)
            tmp = so + ".%d.tmp" % os.getpid()
            subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-shared", "-fPIC", "-I" + emubuild.INC, src, "-o", tmp, "-lm"])
            os.replace(tmp, so)
        L = C.CDLL(so)
        L.achip_composite_setup.restype = None
        L.achip_composite_setup.argtypes = [C.POINTER(Composite), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int]
        L.achip_frame_setup.restype = C.c_int
        L.achip_frame_setup.argtypes = [C.POINTER(emu.Frame), C.c_void_p, C.c_int, C.c_int, C.c_ssize_t, C.c_ssize_t, C.c_int, C.c_bool, C.c_bool, C.c_bool]
        _host = L
    return _host


# ---- composites over test sources ---------------------------------------------------------------------------------------------
class Slot:
    """one placed slot: source a yuv_support.Src (a YUV slot) or an HxWx3 array (RGB24, left as it is)"""

    def __init__(self, source, tile_w, tile_h, org_x=0, org_y=0, ratios=None):
        self.source, self.tile_w, self.tile_h, self.org_x, self.org_y = source, tile_w, tile_h, org_x, org_y
        self.yuv = isinstance(source, YS.Src)
        self.src_w, self.src_h = (source.width, source.height) if self.yuv else (source.shape[1], source.shape[0])
        self.x_ratio, self.y_ratio = ratios or (GR.ratio(self.src_w, tile_w), GR.ratio(self.src_h, tile_h))

    def rgb(self):
        """the slot's whole RGB24 image"""
        return self.source.whole() if self.yuv else self.source


class Comp:
    """slots: up to nine Slot or None (an empty slot: src == NULL); yuv: whether its YUV slots are given to set() as YUV (else
    the composite goes in with the whole conversions as RGB24 sources: no YUV slot)"""

    def __init__(self, canvas, grid, cell, slots, n_src=None, yuv=True):
        self.canvas, self.grid, self.cell, self.slots, self.yuv = canvas, grid, cell, list(slots), yuv
        self.n_src = len(self.slots) if n_src is None else n_src

    @property
    def term(self):
        assert self.canvas[1] % 2 == 0
        return self.canvas[0], self.canvas[1] // 2

    def is_yuv(self, k):
        return self.yuv and k < len(self.slots) and self.slots[k] is not None and self.slots[k].yuv

    def descriptor(self, address, cls=Composite, whole=False):
        """address(object) -> where a slot's RGB24 image lies (an array; with whole, a Src's whole conversion too).  Without
        whole, a YUV slot carries PLACED"""
        c = cls()
        (c.canvas_w, c.canvas_h), (c.cols, c.rows), (c.cell_w, c.cell_h), c.n_src = self.canvas, self.grid, self.cell, self.n_src
        for k, s in enumerate(self.slots):
            if s is None:
                continue
            d = c.s[k]
            d.src = PLACED if self.is_yuv(k) and not whole else address(s.rgb())
            d.src_w, d.src_h, d.src_stride = s.src_w, s.src_h, 3 * s.src_w
            d.tile_w, d.tile_h, d.org_x, d.org_y, d.x_ratio, d.y_ratio = s.tile_w, s.tile_h, s.org_x, s.org_y, s.x_ratio, s.y_ratio
        return c

    def nine(self, base_of, cls=YS.CSource):
        """the nine sources beside the slots; base_of(Src) -> the 16-aligned address of its image"""
        arr = (cls * 9)()
        for k in range(9):
            if self.is_yuv(k):
                arr[k] = self.slots[k].source.c_source(base_of(self.slots[k].source), cls)
        return arr

    def oracle_canvas(self):
        """the canvas by the oracle's resize of every placed source's whole image (slots with the reference's ratios only)"""
        cv = np.zeros((self.canvas[1], self.canvas[0], 3), np.uint8)
        for k, s in enumerate(self.slots[:self.n_src]):
            if s is None:
                continue
            assert (s.x_ratio, s.y_ratio) == (GR.ratio(s.src_w, s.tile_w), GR.ratio(s.src_h, s.tile_h))
            cv[s.org_y:s.org_y + s.tile_h, s.org_x:s.org_x + s.tile_w] = orc.resize_nn(s.rgb(), s.tile_w, s.tile_h)
        return cv


def single(src, tile_w, tile_h, ratios=None):
    """one source as the only tile of a canvas of the tile's size"""
    return Comp((tile_w, tile_h), (1, 1), (tile_w, tile_h), [Slot(src, tile_w, tile_h, 0, 0, ratios)])


def from_setup(srcs, term, yuv=True):
    """the composite achip_composite_setup makes of the sources (Src or arrays) at a terminal size"""
    n = len(srcs)
    dims = [(s.width, s.height) if isinstance(s, YS.Src) else (s.shape[1], s.shape[0]) for s in srcs]
    ptrs = (C.c_void_p * n)(*[PLACED] * n)
    c = Composite()
    host_lib().achip_composite_setup(C.byref(c), ptrs, (C.c_int * n)(*[d[0] for d in dims]), (C.c_int * n)(*[d[1] for d in dims]), n, *term)
    assert c.n_src == n <= 9 and (c.canvas_w, c.canvas_h) == (term[0], 2 * term[1])
    slots = []
    for k in range(n):
        d = c.s[k]
        assert d.src and (d.src_w, d.src_h) == dims[k]
        slots.append(Slot(srcs[k], d.tile_w, d.tile_h, d.org_x, d.org_y, (d.x_ratio, d.y_ratio)))
        assert (d.x_ratio, d.y_ratio) == (GR.ratio(d.src_w, d.tile_w), GR.ratio(d.src_h, d.tile_h)), "setup makes the reference's ratios"
    return Comp((c.canvas_w, c.canvas_h), (c.cols, c.rows), (c.cell_w, c.cell_h), slots, yuv=yuv)


class GridCase:
    def __init__(self, comps, max_tiles=None):
        self.comps = list(comps)
        self.tiles = [c.slots[k] for c in self.comps for k in range(9) if c.is_yuv(k)]  # composites in order, then slots in order
        self.max_tiles = max_tiles or max(1, len(self.tiles), len(self.comps))
        self._expected = None

    def srcs(self):
        """the distinct YUV sources given as YUV"""
        seen = {}
        for t in self.tiles:
            seen[id(t.source)] = t.source
        return list(seen.values())

    def rgbs(self, whole=False):
        """the distinct RGB24 images the descriptors point at: the RGB slots and the sources of the composites that go in
        without YUV slots; with whole, the whole conversion of every YUV source too (for the descriptors over whole frames)"""
        seen = {}
        for c in self.comps:
            for k, s in enumerate(c.slots):
                if s is not None and (whole or not c.is_yuv(k)):
                    seen[id(s.rgb())] = s.rgb()
        return list(seen.values())

    def expected(self):
        if self._expected is None:
            self._expected = [GR.tile(t.source.ref, t.tile_w, t.tile_h, t.x_ratio, t.y_ratio) for t in self.tiles]
            for e in self._expected:
                e.setflags(write=False)
        return self._expected

    def layout(self):
        return GR.layout([(t.tile_w, t.tile_h) for t in self.tiles])


class Placed:
    """a case's memory at addresses: base_of(Src) and address(array), from dictionaries by id"""

    def __init__(self, case, bases, addresses, cls=Composite, src_cls=YS.CSource, whole=False):
        self.case = case
        self.base_of = lambda s: bases[id(s)]
        self.address = lambda a: addresses[id(a)]
        self.comps = [c.descriptor(self.address, cls) for c in case.comps]
        self.whole = [c.descriptor(self.address, cls, whole=True) for c in case.comps] if whole else None
        self.nines = [c.nine(self.base_of, src_cls) for c in case.comps]
        n = len(case.comps)
        self.comp_ptrs = (C.c_void_p * n)(*[C.addressof(c) for c in self.comps])
        self.nine_ptrs = (C.c_void_p * n)(*[C.addressof(a) for a in self.nines])


def place_on_host(case, whole=False):
    """whole: with the descriptors over the whole conversions beside the case's own (Placed.whole)"""
    keep = {id(s): YS.host_copy(s) for s in case.srcs()}
    rgbs = {id(a): np.ascontiguousarray(a) for a in case.rgbs(whole)}
    p = Placed(case, {k: v[1] for k, v in keep.items()}, {k: v.ctypes.data for k, v in rgbs.items()}, whole=whole)
    p.keep = (keep, rgbs)
    return p


# ---- the slab -------------------------------------------------------------------------------------------------------------------
def slab(case, base=None):
    """-> (guard-filled buffer, byte index of tile 0: a 16-byte boundary of the address the bytes will live at)"""
    buf = np.full(64 + 16 + case.layout()[1] + 256, FILL, dtype=np.uint8)
    start = 64 + (-((buf.ctypes.data if base is None else base) + 64)) % 16
    return buf, start


def check_slab(name, case, buf, start):
    """every tile the restatement's, every other byte of the buffer still the guard"""
    at, total = case.layout()
    assert (buf[:start] == FILL).all(), f"{name}: a store in front of the first tile"
    pos = start
    for t, (want, a) in enumerate(zip(case.expected(), at)):
        assert (buf[pos:start + a] == FILL).all(), f"{name}: a store between tiles {t - 1} and {t}"
        nb = want.size
        got = buf[start + a:start + a + nb]
        if not np.array_equal(got, want.reshape(-1)):
            k = int(np.argmax(got != want.reshape(-1)))
            raise AssertionError(f"{name} tile {t}: byte {k} (pixel {k // 3} of {nb // 3}) is {int(got[k])}, restatement {int(want.reshape(-1)[k])}")
        pos = start + a + nb
    assert (buf[pos:] == FILL).all(), f"{name}: a store behind the last tile"
    assert pos - start <= total


def emu_run(case, host=False, whole=False):
    """-> (buffer, start, Placed) of the tile pass under the emulator (host: yuvgrid_math.h's host fill in the kernel's place)"""
    p = place_on_host(case, whole)
    buf, start = slab(case)
    rc = emulator().emu_yuvgrid_run(C.cast(p.comp_ptrs, C.c_void_p), C.cast(p.nine_ptrs, C.c_void_p), len(case.comps), case.max_tiles,
                                    buf.ctypes.data + start, 1 if host else 0)
    assert rc == 0, f"refused ({rc})"
    return buf, start, p


def emu_composites(case, p, tiles_address):
    out = (Composite * len(case.comps))()
    rc = emulator().emu_yuvgrid_composites(C.cast(p.comp_ptrs, C.c_void_p), C.cast(p.nine_ptrs, C.c_void_p), len(case.comps), case.max_tiles,
                                           tiles_address, C.cast(out, C.c_void_p))
    assert rc == 0, f"refused ({rc})"
    return [out[i] for i in range(len(case.comps))]


def check_rewrite(name, case, given, out, tiles_address):
    """composites() rewrites src, src_w, src_h, src_stride and the ratios of every YUV slot and nothing else"""
    at, _ = case.layout()
    t = 0
    for ci, (comp, g, o) in enumerate(zip(case.comps, given, out)):
        for f in GR.COMP_FIELDS:
            assert getattr(o, f) == getattr(g, f), (name, ci, f)
        for k in range(9):
            have = {f: getattr(o.s[k], f) for f in GR.SLOT_FIELDS}
            if comp.is_yuv(k):
                want = GR.rewritten_slot(g.s[k], tiles_address + at[t])
                t += 1
            else:
                want = {f: getattr(g.s[k], f) for f in GR.SLOT_FIELDS}
            assert have == want, (name, ci, k, have, want)
    assert t == len(case.tiles)


def comp_frame(comp, comp_address, mode):
    """the frame that renders a composite's canvas in `mode` (as tests/test_composite_boundaries.py makes it)"""
    tw, th = comp.term
    rm = MODE_CAPS.get(mode, (3, 0))[1]
    f = emu.Frame()
    assert host_lib().achip_frame_setup(C.byref(f), None, tw, 2 * th, tw, 2 * th if rm == 2 else th, rm, True, True, False) == 0
    f.comp = comp_address
    return f


def oracle_text(canvas, term, mode):
    cl, rm = MODE_CAPS[mode]
    return orc.convert_with_caps(canvas, term[0], 2 * term[1] if rm == 2 else term[1], cl, rm, True, True, False)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
GRID_3X3 = "3x3 by hand: n_src 8, formats mixed, an RGB24 slot, an empty slot"
THREE_COMPOSITES = "three composites over the same nine sources, one without YUV slots, max_tiles 64"
NO_YUV = "a set without any YUV slot"
NINE_1080P = "nine NV12 1920x1080 through achip_composite_setup at 160x48"
RENDERED = (GRID_3X3, THREE_COMPOSITES)

_cases = None


def grid_3x3(seed=900):
    """the 3x3 composite by hand; another seed: the same geometry over other contents (another tick)"""
    cw, ch = 20, 16
    srcs = [YS.Src(I420, 64, 48, seed, strides=(70, 0, 35), offs=(1, 0, 2)), YS.Src(NV12, 7, 5, seed + 1), YS.Src(YUYV, 16, 8, seed + 2, extremes=True),
            YS.Src(UYVY, 300, 2, seed + 3, offs=(3, 0, 0)), orc.frame_hash_noise(33, 21, seed + 4), YS.Src(NV12, 4, 2, seed + 5), None,
            YS.Src(I420, 30, 17, seed + 7)]
    sizes = [(20, 15), (18, 16), (20, 16), (13, 9), (16, 12), (5, 3), None, (19, 7)]
    assert len({s for s in sizes if s}) == 7
    slots = []
    for k, (s, size) in enumerate(zip(srcs, sizes)):
        if s is None:
            slots.append(None)
            continue
        tw, th = size
        slots.append(Slot(s, tw, th, (k % 3) * cw + (cw - tw) // 2, (k // 3) * ch + (ch - th) // 2))
    return Comp((60, 48), (3, 3), (cw, ch), slots, n_src=8)


def cases():
    global _cases
    if _cases is not None:
        return _cases
    c = {}
    stride = YS.sample_cases()
    for fmt in YS.FORMATS:
        n = YR.NAMES[fmt]
        c[f"{n} 16x8 -> tile 5x3: three whole lanes and a three-pixel tail"] = GridCase([single(YS.Src(fmt, 16, 8, 810 + fmt, extremes=True), 5, 3)])
        c[f"{n} 2x2 -> tile 1x1"] = GridCase([single(YS.Src(fmt, 2, 2, 820 + fmt), 1, 1)])
        up = YS.Src(fmt, 4, 2, 830 + fmt)
        c[f"{n} upscale 4x2 -> tile 9x5"] = GridCase([single(up, 9, 5)])
        c[f"{n} 4x2 -> tile 9x5, both ratios doubled: into the clamp"] = GridCase([single(up, 9, 5, (2 * GR.ratio(4, 9), 2 * GR.ratio(2, 5)))])
    for fmt in YS.PLANAR:  # odd in both axes
        s = YS.Src(fmt, 7, 5, 840 + fmt)
        c[f"{YR.NAMES[fmt]} 7x5 -> tiles 7x5 and 4x3"] = GridCase([single(s, 7, 5), single(s, 4, 3)])
    for fmt in YR.PACKED:
        c[f"{YR.NAMES[fmt]} 8x2 -> tile 8x2: both pixels of every pair"] = GridCase([single(YS.Src(fmt, 8, 2, 850 + fmt), 8, 2)])
    for name in ("I420 strides 24 / 13 / 11", "NV12 strides 19 / 22", "YUYV stride 37", "UYVY stride 40"):  # padded, bases off alignment
        c[f"{name} -> tile 5x3"] = GridCase([single(stride[name].items[0][0], 5, 3)])
    c["UYVY 300x2 -> tile 299x2: lanes straddle the rows"] = GridCase([single(YS.Src(UYVY, 300, 2, 860), 299, 2)])
    c["NV12 64x48 -> tile 37x29: two workgroups, one pixel in the last lane"] = GridCase([single(YS.Src(NV12, 64, 48, 861), 37, 29)])
    c[GRID_3X3] = GridCase([grid_3x3()])
    nine = [YS.Src(YS.FORMATS[i % 4], *[(64, 48), (32, 18), (16, 8), (30, 40)][(i // 2) % 4], 870 + i, offs=(i % 4, 0, (i + 1) % 4)) for i in range(9)]
    c[THREE_COMPOSITES] = GridCase([from_setup(nine, (60, 30)), from_setup(nine, (48, 20), yuv=False), from_setup(nine, (90, 24))], max_tiles=64)
    c[NO_YUV] = GridCase([Comp((20, 16), (1, 1), (20, 16), [Slot(orc.frame_hash_noise(8, 6, 880), 20, 15, 0, 0)])])
    c[NINE_1080P] = GridCase([from_setup([YS.Src(NV12, 1920, 1080, 890 + i) for i in range(9)], (160, 48))])
    _cases = c
    return c


# ---- the host side (yuvgrid.c) through its C interface: the real library on a GPU, or the mock build without one ---------------
def bind(L):
    vp, ci = C.c_void_p, C.c_int
    for name, res, args in (("device_count", ci, []), ("last_error", C.c_char_p, []), ("create", ci, [C.POINTER(vp), ci]),
                            ("set", ci, [vp, vp, vp, ci, vp]), ("tiles_bytes", C.c_size_t, [vp]), ("run", ci, [vp, vp, vp]),
                            ("composites", ci, [vp, vp, vp]), ("destroy", None, [vp])):
        fn = getattr(L, "asciichat_yuvgrid_" + name)
        fn.restype, fn.argtypes = res, args
    return L


_mock = None


def mock_library():
    """yuvgrid.c as it stands over the mock HIP runtime (tests/mockhip/mock_hip.c: device memory is host memory), its launcher the
    emulator's (yuvgrid_emu_driver.cpp): the handle's own code without a GPU"""
    global _mock
    if _mock is None:
        import os
        import subprocess
        import mockgpu
        so = os.path.join(emubuild.OUT_DIR, "libyuvgrid_mock.so")
        srcs = [os.path.join(emubuild.CSRC, "yuvgrid.c"), os.path.join(mockgpu.MOCK, "mock_hip.c"), os.path.join(emubuild.EMU_DIR, "yuvgrid_emu_driver.cpp")]
        deps = srcs + [emubuild._header(h) for h in ("hip_emu.h", "gfx950_ops.hpp", "yuvgrid_kernels.hpp", "yuvgrid.h", "yuvgrid_math.h", "yuv_math.h",
                                                    "asciichat_yuvgrid.h", "asciichat_yuv.h", "achip_desc.h", "achip_types.h")]
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
    """asciichat_yuvgrid_* of a bound library, return codes as they come"""

    stream = 0

    def __init__(self, L, max_tiles, stream=0):
        self.L, self.h, self.stream = L, C.c_void_p(), stream
        rc = L.asciichat_yuvgrid_create(C.byref(self.h), max_tiles)
        assert rc == 0, (rc, self.error())

    def error(self):
        return self.L.asciichat_yuvgrid_last_error().decode()

    def set(self, p, n=None):
        return self.L.asciichat_yuvgrid_set(self.h, C.cast(p.comp_ptrs, C.c_void_p), C.cast(p.nine_ptrs, C.c_void_p), len(p.comps) if n is None else n,
                                            self.stream)

    def tiles_bytes(self):
        return int(self.L.asciichat_yuvgrid_tiles_bytes(self.h))

    def run(self, tiles):
        return self.L.asciichat_yuvgrid_run(self.h, tiles, self.stream)

    def composites(self, tiles, n, cls=Composite):
        out = (cls * n)()
        rc = self.L.asciichat_yuvgrid_composites(self.h, tiles, C.cast(out, C.c_void_p))
        return rc, [out[i] for i in range(n)]

    def close(self):
        if self.h:
            self.L.asciichat_yuvgrid_destroy(self.h)
            self.h = C.c_void_p()


INVALID = 86


class Trial:
    """a set to try: private copies of a Placed's descriptors and sources, free to be changed"""

    def __init__(self, p):
        self.comps = [type(c).from_buffer_copy(bytes(c)) for c in p.comps]
        self.nines = [type(a).from_buffer_copy(bytes(a)) for a in p.nines]
        self.link()

    def link(self):
        n = len(self.comps)
        self.comp_ptrs = (C.c_void_p * n)(*[C.addressof(c) for c in self.comps])
        self.nine_ptrs = (C.c_void_p * n)(*[C.addressof(a) for a in self.nines])


def refusal_case():
    """two composites, three YUV slots: composite 1 has a YUV slot, an RGB24 slot and a YUV slot, n_src 3"""
    one = Comp((12, 4), (3, 1), (6, 4), [Slot(YS.Src(NV12, 16, 8, 951), 5, 3), Slot(orc.frame_hash_noise(8, 6, 952), 6, 4, 6, 0),
                                        Slot(YS.Src(UYVY, 16, 8, 953), 6, 4, 12, 0)])
    return GridCase([single(YS.Src(I420, 16, 8, 950, extremes=True), 5, 3), one], max_tiles=3)


def check_refusals(L, place, new_slab, stream=0, synchronize=lambda: None):
    """Every refusal of include/asciichat_yuvgrid.h at its limit -- the last accepted value passes, the first refused is refused
    with ERR_INVALID_PARAM --, and that a refused set leaves the handle as it was.  place(case) -> Placed at addresses L's kernel
    can read; new_slab(case) -> (address of tile 0, read: () -> (buffer, start))"""
    case = refusal_case()
    p = place(case)
    n = len(case.comps)
    tiles, read = new_slab(case)
    # create
    for bad in (0, -1, 4097):
        h = C.c_void_p(1)
        assert L.asciichat_yuvgrid_create(C.byref(h), bad) == INVALID and not h.value and str(bad) in L.asciichat_yuvgrid_last_error().decode()
    assert L.asciichat_yuvgrid_create(None, 3) == INVALID
    for good in (1, 4096):
        Handle(L, good).close()
    # a handle that is not one of this library's
    junk = np.zeros(512, dtype=np.uint8)
    fake = Handle.__new__(Handle)
    fake.L, fake.h = L, C.c_void_p(junk.ctypes.data)
    for who in (fake, None):
        hh = who or Handle.__new__(Handle)
        if who is None:
            hh.L, hh.h = L, C.c_void_p()
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

        def null_entry(which, c):
            def change(t):
                t.link()
                getattr(t, which)[c] = None
                t.link = lambda: None
            return change

        # the number of composites
        assert refused(count=0) and refused(count=-1) and not refused(count=1) and not refused(count=2)
        # NULL arrays and entries
        assert L.asciichat_yuvgrid_set(g.h, None, C.cast(p.nine_ptrs, C.c_void_p), n, stream) == INVALID
        assert L.asciichat_yuvgrid_set(g.h, C.cast(p.comp_ptrs, C.c_void_p), None, n, stream) == INVALID
        assert refused(null_entry("comp_ptrs", 1), named="composite 1") and refused(null_entry("nine_ptrs", 0), named="composite 0")
        # n_src: 0..9 (composite 0 without its YUV source has no YUV slot: any n_src in range passes)
        no_yuv = source(0, 0, plane=(C.c_void_p * 3)())
        for v, want in ((-1, True), (0, False), (9, False), (10, True)):
            def change(t, v=v):
                no_yuv(t)
                comp(0, n_src=v)(t)
            assert refused(change, named="composite 0") == want, v
        # a YUV slot at or behind n_src, and one that is not placed
        assert not refused(comp(1, n_src=3)) and refused(comp(1, n_src=2), named="composite 1 slot 2") and not refused(comp(1, n_src=9))
        assert refused(slot(1, 2, src=None), named="composite 1 slot 2") and not refused(slot(1, 2, src=1))
        # an RGB24 slot is not looked at
        assert not refused(slot(1, 1, src=None, src_w=-5, tile_w=0, x_ratio=0xFFFFFFFF))
        # the source itself (yuv_source_check), and its size against the slot's
        assert refused(source(1, 0, format=4), named="composite 1 slot 0") and refused(source(0, 0, width=8193)) and refused(source(1, 2, width=15))
        assert refused(source(1, 0, stride=(C.c_int32 * 3)(15, 0, 0))) and not refused(source(1, 0, stride=(C.c_int32 * 3)(16, 16, 0)))
        for f in ("src_w", "src_h"):
            base = getattr(p.comps[1].s[0], f)
            assert refused(slot(1, 0, **{f: base - 1})) and refused(slot(1, 0, **{f: base + 1})) and not refused(slot(1, 0, **{f: base}))
        # the tile's size: 1..8192 (ratios small enough not to be the reason)
        for f, r in (("tile_w", "x_ratio"), ("tile_h", "y_ratio")):
            for v, want in ((0, True), (-1, True), (1, False), (8192, False), (8193, True)):
                assert refused(slot(1, 0, **{f: v, r: 4097})) == want, (f, v)
        # a wrapping ratio: (tile - 1) * ratio below 2^32
        top = (1 << 32) - 1
        assert not refused(slot(1, 2, x_ratio=top // 5)) and refused(slot(1, 2, x_ratio=top // 5 + 1), named="composite 1 slot 2")
        assert not refused(slot(1, 2, y_ratio=top // 3)) and refused(slot(1, 2, y_ratio=top // 3 + 1))
        assert not refused(slot(0, 0, tile_w=1, tile_h=1, x_ratio=top, y_ratio=top))  # a tile of one pixel: any ratio
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
        assert (g.tiles_bytes(), [bytes(c) for c in g.composites(tiles, n)[1]]) == before
        # the slab and the output
        assert g.run(None) == INVALID and g.run(tiles + 8) == INVALID and g.run(tiles + 1) == INVALID
        assert g.composites(None, n)[0] == INVALID and g.composites(tiles + 4, n)[0] == INVALID
        assert L.asciichat_yuvgrid_composites(g.h, tiles, None) == INVALID and "no descriptors" in g.error()
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
