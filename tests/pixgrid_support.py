"""Support of the packed RGB tile tests (libasciichat_pixgrid.so): the one case table the emulated and the GPU tests share --
composites over the test sources of pix_support.py, built with yuvgrid_support's Comp over a Slot of its own --, the two kernels
under the CPU emulator at the shipped segment width or at another (tests/hipemu/pixgrid_emu_driver.cpp), pixgrid.c itself over the
mock HIP runtime, the guard-filled slab and its check per tile form, the rewrite check, and the refusals.  Expected tiles come
from tests/pixgrid_ref.py.  TESTS ONLY."""
import ctypes as C
import os

import numpy as np

import emubuild
import orc
import pix_ref as PR
import pix_support as PS
import pixgrid_ref as GR
import yuvgrid_support as GS
from achip_ctypes import Composite

FILL = PS.FILL
RGB, RGBA, BGR, BGRA = PS.RGB, PS.RGBA, PS.BGR, PS.BGRA
FORMATS, NAMES, BPP = PS.FORMATS, PS.NAMES, PS.BPP
INVALID, NOT_SUPPORTED = 86, 30
MAX_W, MAX_H, MAX_TILE = 3840, 2160, 8192
KINDS = ("run", "box")
NO_SPLIT = 0
SHIPPED = 512
CANDIDATES = (NO_SPLIT, 1024, 512, 256)  # what the shipped width is chosen among
OTHER_WIDTHS = (NO_SPLIT, 1024, 256, 16)  # the other candidates, and a width at which the small cases have segments too
HEADERS = ("pixgrid_kernels.hpp", "pixgrid.h", "pix_kernels.hpp", "pix.h", "pix_math.h", "yuvboxgrid.h", "yuvbox.h", "yuvgrid_math.h", "yuv_math.h",
           "asciichat_pixgrid.h", "asciichat_pix.h", "asciichat_yuv.h", "achip_desc.h", "achip_types.h")
PLACED = GS.PLACED
Comp, Placed, Trial, slab, check_rewrite = GS.Comp, GS.Placed, GS.Trial, GS.slab, GS.check_rewrite

_emu = {}


def emulator(seg=None):
    """the driver built at the shipped segment width (None), or with -DPIXGRID_SEG_COLS=seg"""
    if seg not in _emu:
        drv = os.path.join(emubuild.EMU_DIR, "pixgrid_emu_driver.cpp")
        assert os.path.exists(drv), "tests/hipemu/pixgrid_emu_driver.cpp is missing: the emulator driver of libasciichat_pixgrid.so"
        if seg is None:
            L = C.CDLL(emubuild.shared_library("libpixgrid_emu.so", "pixgrid_emu_driver.cpp", HEADERS))
        else:
            L = C.CDLL(emubuild.shared_library(f"libpixgrid_emu_seg{seg}.so", "pixgrid_emu_driver.cpp", HEADERS, defines=(f"PIXGRID_SEG_COLS={seg}",)))
        vp, ci, u32 = C.c_void_p, C.c_int, C.c_uint32
        L.emu_pixgrid_seg_cols.restype = u32
        L.emu_pixgrid_seg_cols.argtypes = []
        L.emu_pixgrid_launches.restype = C.c_long
        L.emu_pixgrid_launches.argtypes = []
        L.emu_pixgrid_set_check.restype = ci
        L.emu_pixgrid_set_check.argtypes = [vp, vp, ci, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(C.c_char_p)]
        L.emu_pixgrid_layout.restype = C.c_int64
        L.emu_pixgrid_layout.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp]
        L.emu_pixgrid_run.restype = ci
        L.emu_pixgrid_run.argtypes = [vp, vp, ci, ci, vp, ci, ci]
        L.emu_pixgrid_composites.restype = ci
        L.emu_pixgrid_composites.argtypes = [vp, vp, ci, ci, vp, vp]
        assert L.emu_pixgrid_seg_cols() == (SHIPPED if seg is None else seg)
        _emu[seg] = L
    return _emu[seg]


# ---- composites over packed test sources ------------------------------------------------------------------------------------------
class Slot:
    """one placed slot: source a pix_support.Src (a packed slot) or an HxWx3 array (RGB24, left as it is).  The fields
    yuvgrid_support.Comp reads: `yuv` there says "a slot of the pass", here a packed one"""

    def __init__(self, source, tile_w, tile_h, org_x=0, org_y=0, ratios=None):
        self.source, self.tile_w, self.tile_h, self.org_x, self.org_y = source, tile_w, tile_h, org_x, org_y
        self.yuv = not isinstance(source, np.ndarray)
        self.src_w, self.src_h = (source.width, source.height) if self.yuv else (source.shape[1], source.shape[0])
        self.x_ratio, self.y_ratio = ratios or (GR.ratio(self.src_w, tile_w), GR.ratio(self.src_h, tile_h))

    def rgb(self):
        """the slot's whole RGB24 image"""
        return self.source.whole() if self.yuv else self.source


def single(src, tile_w, tile_h, ratios=None):
    """one source as the only tile of a canvas of the tile's size"""
    return Comp((tile_w, tile_h), (1, 1), (tile_w, tile_h), [Slot(src, tile_w, tile_h, 0, 0, ratios)])


class Case(GS.GridCase):
    """a yuvgrid_support.GridCase over packed sources whose expected tiles come per tile form: "run" sampled, "box" averaged"""

    def __init__(self, comps, max_tiles=None):
        super().__init__(comps, max_tiles)
        self._expected = {}

    def expected(self, kind):
        if kind not in self._expected:
            if kind == "run":
                e = [GR.tile(t.source.whole(), t.tile_w, t.tile_h, t.x_ratio, t.y_ratio) for t in self.tiles]
            else:
                e = [GR.box_tile(t.source.whole(), t.tile_w, t.tile_h) for t in self.tiles]
            for a in e:
                a.setflags(write=False)
            self._expected[kind] = e
        return self._expected[kind]

    def layout(self):
        return GR.layout([(t.tile_w, t.tile_h) for t in self.tiles])


def place_on_host(case, whole=False):
    """whole: with the descriptors over the whole conversions beside the case's own (Placed.whole)"""
    keep = {id(s): PS.host_copy(s) for s in case.srcs()}
    rgbs = {id(a): np.ascontiguousarray(a) for a in case.rgbs(whole)}
    p = Placed(case, {k: v[1] for k, v in keep.items()}, {k: v.ctypes.data for k, v in rgbs.items()}, src_cls=PS.CSource, whole=whole)
    p.keep = (keep, rgbs)
    return p


def check_slab(name, case, kind, buf, start):
    """every tile the restatement's, every other byte of the buffer -- in front, in the gaps of the 16-byte rounding, behind --
    still the guard"""
    at, total = case.layout()
    assert (buf[:start] == FILL).all(), f"{name} ({kind}): a store in front of the first tile"
    pos = start
    for t, (want, a) in enumerate(zip(case.expected(kind), at)):
        assert (buf[pos:start + a] == FILL).all(), f"{name} ({kind}): a store between tiles {t - 1} and {t}"
        nb = want.size
        got = buf[start + a:start + a + nb]
        if not np.array_equal(got, want.reshape(-1)):
            k = int(np.argmax(got != want.reshape(-1)))
            raise AssertionError(f"{name} ({kind}) tile {t}: byte {k} (pixel {k // 3} of {nb // 3}) is {int(got[k])}, restatement {int(want.reshape(-1)[k])}")
        pos = start + a + nb
    assert (buf[pos:] == FILL).all(), f"{name} ({kind}): a store behind the last tile"
    assert pos - start <= total


# ---- the kernels under the emulator -----------------------------------------------------------------------------------------------
def _args(case, p):
    return C.cast(p.comp_ptrs, C.c_void_p), C.cast(p.nine_ptrs, C.c_void_p), len(case.comps), case.max_tiles


def emu_run(case, kind, seg=None, host=False, whole=False):
    """-> (buffer, start, Placed) of the sampled ("run") or the averaged ("box") pass under the emulator built at segment width
    seg (host: pixgrid.h's host walk in the kernel's place)"""
    p = place_on_host(case, whole)
    buf, start = slab(case)
    rc = emulator(seg).emu_pixgrid_run(*_args(case, p), buf.ctypes.data + start, int(kind == "box"), int(host))
    assert rc == 0, f"refused ({rc})"
    return buf, start, p


def emu_layout(case, p, seg=None):
    """-> dict(bytes, at, first_wg, segs, seg_out, cols, slices, max_pixels, workgroups, stage_cols, boxable) as pixgrid.h lays the
    set out at segment width seg"""
    n = max(1, case.max_tiles)
    at, first, segs, seg_out, cols_of, slices = (C.c_uint64 * n)(), *[(C.c_uint32 * n)() for _ in range(5)]
    launch = (C.c_uint32 * 4)()
    total = emulator(seg).emu_pixgrid_layout(*_args(case, p), *[C.cast(a, C.c_void_p) for a in (at, first, segs, seg_out, cols_of, slices, launch)])
    assert total >= 0, "refused"
    k = len(case.tiles)
    return dict(bytes=total, at=list(at)[:k], first_wg=list(first)[:k], segs=list(segs)[:k], seg_out=list(seg_out)[:k], cols=list(cols_of)[:k],
                slices=list(slices)[:k], max_pixels=launch[0], workgroups=launch[1], stage_cols=launch[2], boxable=bool(launch[3]))


def emu_composites(case, p, tiles_address):
    out = (Composite * len(case.comps))()
    rc = emulator().emu_pixgrid_composites(*_args(case, p), tiles_address, C.cast(out, C.c_void_p))
    assert rc == 0, f"refused ({rc})"
    return [out[i] for i in range(len(case.comps))]


# ---- the cut of a row, said again (independent of yuvboxgrid.h) -------------------------------------------------------------------
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


# ---- the cases ------------------------------------------------------------------------------------------------------------------
MIXED = "three composites: 8, 4 and 1 slots, four formats, tiles of many sizes, n_src 8, an empty slot, an RGB24 slot, max_tiles 20"
NO_PACKED = "a set without any packed slot"
THREE_SEGMENTS = "1300x6 -> tile 13x2 three segments, the last shorter, two slices"
WIDE_BOX = "1300x6 -> tile 2x2 one box wider than the bound, one slice"
MANY_ROWS = "40x37 -> tile 5x3 four slices, more box rows than slices"
FEW_ROWS = "40x3 -> tile 5x3 four slices, fewer box rows than slices"
WHITE = "RGBA 3840x18 all 255 -> tile 1x2 the widest stage, sums pass 2^24"
CLAMPED = "4x2 -> tile 9x5, both ratios doubled: into the clamp"
STRIDES = ("tight", "16", "1")
_cases = None


def _stride(fmt, w, kind):
    return 0 if kind == "tight" else PS._stride(fmt, w, kind)


def white():
    return PS.Src(RGBA, MAX_W, 18, 480, pixels=np.full((18, MAX_W, 3), 255, np.uint8))


def alpha_pairs():
    """[(name, Case, Case)]: the same pixels of a 4-byte format under alpha 0x00 and alpha 0xFF -- the tiles must be equal"""
    px = np.random.default_rng(77).integers(0, 256, (6, 20, 3), dtype=np.uint8)
    out = []
    for fmt in (RGBA, BGRA):
        pair = [Case([single(PS.Src(fmt, 20, 6, 78, off=3, stride=87, pixels=px, alpha=alpha), 5, 3)]) for alpha in (0x00, 0xFF)]
        assert all((c.tiles[0].source.whole() == px).all() for c in pair) and not np.array_equal(pair[0].tiles[0].source.image, pair[1].tiles[0].source.image)
        out.append((NAMES[fmt], *pair))
    return out


def mixed_set(seed=700, shift=0):
    """three composites; another seed and shift: the same geometry over other contents in other formats (another tick)"""
    sizes = [(64, 48), (30, 18), (16, 8), (300, 6)]
    srcs = []
    for i in range(9):
        fmt, (w, h), pad = FORMATS[(i + shift) % 4], sizes[(i + i // 4) % 4], (0, 3, 4, 16)[i % 4]
        srcs.append(PS.Src(fmt, w, h, seed + i, stride=BPP[fmt] * w + pad if pad else 0, off=(0, 1, 2, 3, 5)[i % 5]))
    nine_tiles = [(20, 15), (7, 4), (5, 3), (19, 2), None, (1, 1), None, (9, 11), (13, 6)]
    slots = []
    for k, size in enumerate(nine_tiles):
        if k == 4:
            slots.append(Slot(orc.frame_hash_noise(33, 21, seed + 40), 16, 12, 22, 18))  # RGB24 without a packed source: left as it stands
        elif size is None:
            slots.append(None)  # empty
        else:
            slots.append(Slot(srcs[k], size[0], size[1], (k % 3) * 20, (k // 3) * 16))
    nine = Comp((60, 48), (3, 3), (20, 16), slots[:8], n_src=8)  # (slot 8's source serves the second composite)
    four = Comp((40, 24), (2, 2), (20, 12), [Slot(srcs[k], *t, (i % 2) * 20, (i // 2) * 12) for i, (k, t) in
                                            enumerate(((0, (20, 12)), (3, (17, 5)), (2, (8, 8)), (8, (20, 3))))])
    one = Comp((24, 10), (1, 1), (24, 10), [Slot(srcs[1], 24, 10)])
    return Case([nine, four, one], max_tiles=20)


def cases():
    """{name: Case}: every case is run by the sampled pass and by the averaged pass"""
    global _cases
    if _cases is not None:
        return _cases
    c = {}
    for fmt in FORMATS:
        n = NAMES[fmt]
        # base +0 and +1..3, stride tight, padded to a multiple of 16, and odd: 15 pixels, three whole lanes and a three-pixel tail
        for off in (0, 1 + fmt % 3):
            for kind in STRIDES:
                c[f"{n} 20x6 -> tile 5x3 base +{off} stride {kind}"] = Case([single(PS.Src(fmt, 20, 6, 40 + fmt, stride=_stride(fmt, 20, kind), off=off), 5, 3)])
        for w in (1, 2, 3, 5, 6, 7):  # below one group, and w % 4 in {1, 2, 3}
            c[f"{n} {w}x1 -> tile 2x1"] = Case([single(PS.Src(fmt, w, 1, 50 + fmt + 4 * w), 2, 1)])
    f = lambda i: FORMATS[i % 4]  # noqa: E731
    # sampled tiles
    c["BGRA 2x2 -> tile 1x1"] = Case([single(PS.Src(BGRA, 2, 2, 410), 1, 1)])
    c["RGB 16x8 -> tile 5x1 five pixels: one in the last lane"] = Case([single(PS.Src(RGB, 16, 8, 411), 5, 1)])
    c["BGR 16x8 -> tile 3x2 six pixels, lanes straddle the rows"] = Case([single(PS.Src(BGR, 16, 8, 412), 3, 2)])
    c["RGBA 16x8 -> tile 3x3 nine pixels, lanes straddle the rows"] = Case([single(PS.Src(RGBA, 16, 8, 413), 3, 3)])
    up = PS.Src(BGRA, 4, 2, 414, off=2)
    c["BGRA 4x2 -> tile 9x5 larger than its source"] = Case([single(up, 9, 5)])
    c["BGRA " + CLAMPED] = Case([single(up, 9, 5, (2 * GR.ratio(4, 9), 2 * GR.ratio(2, 5)))])
    c["BGR 64x48 -> tile 37x29 two workgroups of samples"] = Case([single(PS.Src(BGR, 64, 48, 415), 37, 29)])
    # averaged tiles
    c["RGBA 64x36 -> tile 1x1"] = Case([single(PS.Src(RGBA, 64, 36, 420), 1, 1)])
    for i in (1, 2):
        c[f"{NAMES[f(i)]} 6x4 -> tile 6x4 identity"] = Case([single(PS.Src(f(i), 6, 4, 421 + i), 6, 4)])
        c[f"{NAMES[f(i + 1)]} 5x8 -> tile 11x3 larger than its source in one axis"] = Case([single(PS.Src(f(i + 1), 5, 8, 423 + i), 11, 3)])
    # averaged tiles, the cut shapes (asserted from the library's own cut by the emulated tests), in a 4-byte and a 3-byte format
    for fmt in (BGRA, BGR):
        n = NAMES[fmt]
        wide = PS.Src(fmt, 1300, 6, 430 + fmt, off=fmt)
        c[f"{n} {THREE_SEGMENTS}"] = Case([single(wide, 13, 2)])
        c[f"{n} {WIDE_BOX}"] = Case([single(wide, 2, 2)])
        c[f"{n} {MANY_ROWS}"] = Case([single(PS.Src(fmt, 40, 37, 440 + fmt), 5, 3)])
        c[f"{n} {FEW_ROWS}"] = Case([single(PS.Src(fmt, 40, 3, 450 + fmt), 5, 3)])
        c[f"{n} 1031x3 -> tile 7x2 a second group per lane, segments start off a multiple of four"] = Case([single(PS.Src(fmt, 1031, 3, 460 + fmt), 7, 2)])
    c[WHITE] = Case([single(white(), 1, 2)])
    c[MIXED] = mixed_set()
    c[NO_PACKED] = Case([Comp((20, 16), (1, 1), (20, 16), [Slot(orc.frame_hash_noise(8, 6, 880), 20, 15, 0, 0)])])
    _cases = c
    return c


# ---- the host side (pixgrid.c) through its C interface: the real library on a GPU, or the mock build without one ----------------
EXPORTS = ("device_count", "last_error", "create", "set", "tiles_bytes", "run", "run_box", "composites", "destroy")


def bind(L):
    vp, ci = C.c_void_p, C.c_int
    for name, res, args in (("device_count", ci, []), ("last_error", C.c_char_p, []), ("create", ci, [C.POINTER(vp), ci]),
                            ("set", ci, [vp, vp, vp, ci, vp]), ("tiles_bytes", C.c_size_t, [vp]), ("run", ci, [vp, vp, vp]),
                            ("run_box", ci, [vp, vp, vp]), ("composites", ci, [vp, vp, vp]), ("destroy", None, [vp])):
        fn = getattr(L, "asciichat_pixgrid_" + name)
        fn.restype, fn.argtypes = res, args
    return L


_mock = None


def mock_library():
    """pixgrid.c as it stands over the mock HIP runtime (tests/mockhip/mock_hip.c: device memory is host memory), its launchers the
    emulator's (pixgrid_emu_driver.cpp): the handle's own code, at the segment width it ships with, without a GPU.  Its
    emu_pixgrid_launches counts the launches the handle makes"""
    global _mock
    if _mock is None:
        import subprocess
        import mockgpu
        so = os.path.join(emubuild.OUT_DIR, "libpixgrid_mock.so")
        srcs = [os.path.join(emubuild.CSRC, "pixgrid.c"), os.path.join(mockgpu.MOCK, "mock_hip.c"), os.path.join(emubuild.EMU_DIR, "pixgrid_emu_driver.cpp")]
        for s in srcs:
            assert os.path.exists(s), f"{s} is missing"
        deps = srcs + [emubuild._header(h) for h in ("hip_emu.h", "gfx950_ops.hpp") + HEADERS]
        if not (os.path.exists(so) and all(os.path.getmtime(d) <= os.path.getmtime(so) for d in deps)):
            os.makedirs(emubuild.OUT_DIR, exist_ok=True)
            tag = ".%d" % os.getpid()
            objs = []
            for src in srcs[:2]:
                objs.append(os.path.join(emubuild.OUT_DIR, "pixgrid_" + os.path.basename(src) + tag + ".o"))
                subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fPIC", "-pthread", "-I" + emubuild.INC, "-I" + emubuild.CSRC, "-I" + mockgpu.HIP_INC,
                                       "-c", src, "-o", objs[-1]])
            # -Bsymbolic: the hip* calls bind to the mock runtime inside this library whatever else the process has loaded
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wl,-Bsymbolic", *["-I" + d for d in emubuild.INCLUDE], srcs[2], *objs,
                                   "-o", so + tag, "-lpthread"])
            os.replace(so + tag, so)
            for o in objs:
                os.remove(o)
        _mock = bind(C.CDLL(so))
        _mock.emu_pixgrid_launches.restype = C.c_long
        _mock.emu_pixgrid_launches.argtypes = []
    return _mock


class Handle:
    """asciichat_pixgrid_* of a bound library, return codes as they come"""

    def __init__(self, L, max_tiles, stream=0):
        self.L, self.h, self.stream = L, C.c_void_p(), stream
        rc = L.asciichat_pixgrid_create(C.byref(self.h), max_tiles)
        assert rc == 0, (rc, self.error())

    def error(self):
        return self.L.asciichat_pixgrid_last_error().decode()

    def set(self, p, n=None):
        return self.L.asciichat_pixgrid_set(self.h, C.cast(p.comp_ptrs, C.c_void_p), C.cast(p.nine_ptrs, C.c_void_p), len(p.comps) if n is None else n,
                                            self.stream)

    def tiles_bytes(self):
        return int(self.L.asciichat_pixgrid_tiles_bytes(self.h))

    def run(self, tiles, kind="run"):
        return (self.L.asciichat_pixgrid_run_box if kind == "box" else self.L.asciichat_pixgrid_run)(self.h, tiles, self.stream)

    def composites(self, tiles, n, cls=Composite):
        out = (cls * n)()
        rc = self.L.asciichat_pixgrid_composites(self.h, tiles, C.cast(out, C.c_void_p))
        return rc, [out[i] for i in range(n)]

    def close(self):
        if self.h:
            self.L.asciichat_pixgrid_destroy(self.h)
            self.h = C.c_void_p()


def refusal_case():
    """two composites, three packed slots: composite 1 has a packed slot, an RGB24 slot and a packed slot, n_src 3"""
    one = Comp((12, 4), (3, 1), (6, 4), [Slot(PS.Src(BGRA, 16, 8, 951, stride=16 * 4 + 12, off=4), 5, 3), Slot(orc.frame_hash_noise(8, 6, 952), 6, 4, 6, 0),
                                        Slot(PS.Src(RGB, 16, 8, 953), 6, 4, 12, 0)])
    return Case([single(PS.Src(BGR, 16, 8, 950, off=1), 5, 3), one], max_tiles=3)


def check_refusals(L, place, new_slab, stream=0, synchronize=lambda: None):
    """Every refusal of include/asciichat_pixgrid.h at its limit -- the last accepted value passes, the first refused is refused
    with ERR_INVALID_PARAM --, that a refused call launches nothing and leaves the handle as it was, and that the handle still
    works in both tile forms.  place(case) -> Placed at addresses L's kernels can read; new_slab(case) -> (address of tile 0,
    read: () -> (buffer, start))"""
    case = refusal_case()
    p = place(case)
    n = len(case.comps)
    tiles, read = new_slab(case)
    # create
    for bad in (0, -1, 4097):
        h = C.c_void_p(1)
        assert L.asciichat_pixgrid_create(C.byref(h), bad) == INVALID and not h.value and str(bad) in L.asciichat_pixgrid_last_error().decode()
    assert L.asciichat_pixgrid_create(None, 3) == INVALID
    for good in (1, 4096):
        Handle(L, good).close()
    # a handle that is not one of this library's
    junk = np.zeros(512, dtype=np.uint8)
    for address in (junk.ctypes.data, None):
        hh = Handle.__new__(Handle)
        hh.L, hh.h, hh.stream = L, C.c_void_p(address), stream
        assert hh.set(p) == INVALID and hh.run(tiles) == INVALID and hh.run(tiles, "box") == INVALID and hh.composites(tiles, n)[0] == INVALID
        assert hh.tiles_bytes() == 0 and "not a handle" in hh.error()

    g = Handle(L, 3, stream)
    try:
        # before any set
        assert g.run(tiles) == INVALID and "nothing is set" in g.error() and g.run(tiles, "box") == INVALID and "nothing is set" in g.error()
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

        def sized(c, k, w, h, **kw):
            """source and slot at w x h (the pixels are not read: the set is refused, or replaced before any run)"""
            return both(source(c, k, width=w, height=h, **kw), slot(c, k, src_w=w, src_h=h))

        # the number of composites: 0 and max_tiles + 1 (a handle of 3 takes 3 composites, not 4)
        assert refused(count=0) and refused(count=-1) and not refused(count=1) and not refused(count=2)
        three = Trial(p)
        three.comps.append(type(p.comps[0]).from_buffer_copy(bytes(p.comps[0])))
        three.nines.append((type(p.nines[0][0]) * 9)())  # (a third composite without packed slots)
        three.link()
        assert g.set(three, 3) == 0
        three.comps.append(three.comps[2]), three.nines.append(three.nines[2])
        three.link()
        assert g.set(three, 4) == INVALID and "max_tiles" in g.error()
        # NULL arrays and entries
        assert L.asciichat_pixgrid_set(g.h, None, C.cast(p.nine_ptrs, C.c_void_p), n, stream) == INVALID
        assert L.asciichat_pixgrid_set(g.h, C.cast(p.comp_ptrs, C.c_void_p), None, n, stream) == INVALID
        assert refused(null_entry("comp_ptrs", 1), named="composite 1") and refused(null_entry("nine_ptrs", 0), named="composite 0")
        # n_src: 0..9 (composite 0 without its packed source has no packed slot: any n_src in range passes)
        no_packed = source(0, 0, pixels=None)
        for v, want in ((-1, True), (0, False), (9, False), (10, True)):
            assert refused(both(no_packed, comp(0, n_src=v)), named="composite 0") == want, v
        # a packed slot at or behind n_src, and one that is not placed
        assert not refused(comp(1, n_src=3)) and refused(comp(1, n_src=2), named="composite 1 slot 2") and not refused(comp(1, n_src=9))
        assert refused(slot(1, 2, src=None), named="composite 1 slot 2") and not refused(slot(1, 2, src=1))
        # a slot without a packed source is not looked at
        assert not refused(slot(1, 1, src=None, src_w=-5, tile_w=0, x_ratio=0xFFFFFFFF))
        # the source itself (THE RULE of asciichat_pix.h), and its size against the slot's
        for fmt, want in ((-1, True), (4, True), (RGBA, True), (BGR, False)):  # (RGBA over 16 x 8 tight needs 64 bytes a row: a stride of 0 is tight)
            assert refused(source(1, 2, format=fmt, stride=48), named="composite 1 slot 2") == want, fmt
        for w, h, want in ((0, 8, True), (8193, 8, True), (16, 0, True), (16, 8193, True), (-1, 8, True), (1, 1, False), (8192, 1, False), (1, 8192, False)):
            assert refused(sized(1, 2, w, h, stride=0), named="composite 1 slot 2") == want, (w, h)
        for c_, k_, bpp in ((1, 0, 4), (1, 2, 3)):
            for stride, want in ((bpp * 16 - 1, True), (bpp * 16, False), (0, False), (PS.MAX_STRIDE - 1, False), (PS.MAX_STRIDE, True), (-1, True),
                                 (-bpp * 16, True)):
                assert refused(source(c_, k_, stride=stride), named=f"composite {c_} slot {k_}") == want, (k_, stride)
        for f in ("src_w", "src_h"):
            base = getattr(p.comps[1].s[0], f)
            assert refused(slot(1, 0, **{f: base - 1})) and refused(slot(1, 0, **{f: base + 1})) and not refused(slot(1, 0, **{f: base}))
        # a source beyond the box pass is taken by set: run serves it, run_box reports it (check_too_large_for_the_box)
        assert not refused(sized(1, 0, MAX_W + 1, 8, stride=0)) and not refused(sized(1, 0, 16, MAX_H + 1))
        # the tile's size: 1..8192 (ratios small enough not to be the reason)
        for f, r in (("tile_w", "x_ratio"), ("tile_h", "y_ratio")):
            for v, want in ((0, True), (-1, True), (1, False), (MAX_TILE, False), (MAX_TILE + 1, True)):
                assert refused(slot(1, 0, **{f: v, r: 4097}), named="composite 1 slot 0") == want, (f, v)
        # a wrapping ratio: (tile - 1) * ratio below 2^32 -- refused at set for both tile forms
        top = (1 << 32) - 1
        assert not refused(slot(1, 2, x_ratio=top // 5)) and refused(slot(1, 2, x_ratio=top // 5 + 1), named="composite 1 slot 2") and "2^32" in g.error()
        assert not refused(slot(1, 2, y_ratio=top // 3)) and refused(slot(1, 2, y_ratio=top // 3 + 1))
        assert not refused(slot(0, 0, tile_w=1, tile_h=1, x_ratio=top, y_ratio=top))  # a tile of one pixel: any ratio
        # more packed slots than max_tiles (3): a fourth -- slot 1 of composite 1 given as packed
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
        assert refused(source(1, 0, stride=63)) and refused(fourth) and refused(slot(1, 2, x_ratio=top))
        assert (g.tiles_bytes(), [bytes(c) for c in g.composites(tiles, n)[1]]) == before
        # the slab and the output
        for kind in KINDS:
            assert g.run(None, kind) == INVALID and g.run(tiles + 8, kind) == INVALID and g.run(tiles + 1, kind) == INVALID
        assert g.composites(None, n)[0] == INVALID and g.composites(tiles + 4, n)[0] == INVALID
        assert L.asciichat_pixgrid_composites(g.h, tiles, None) == INVALID and "no descriptors" in g.error()
        synchronize()
        buf, start = read()
        assert (buf == FILL).all(), "a refused call launched something"
        # and the handle still works, with the set it was left with: a run afterwards leaves the earlier set's tiles
        for kind in KINDS:
            assert g.run(tiles, kind) == 0
            synchronize()
            buf, start = read()
            check_slab("after the refusals", case, kind, buf, start)
        rc, out = g.composites(tiles, n, type(p.comps[0]))
        assert rc == 0
        check_rewrite("after the refusals", case, p.comps, out, tiles)
    finally:
        g.close()


def too_large_case():
    """a 3841-wide source beside one the box pass takes"""
    return Case([Comp((18, 2), (2, 1), (9, 2), [Slot(PS.Src(BGRA, MAX_W + 1, 2, 960), 9, 2), Slot(PS.Src(RGB, 12, 2, 961), 9, 2, 9, 0)])])


def check_too_large_for_the_box(L, place, new_slab, stream=0, synchronize=lambda: None):
    """3841 x 2: taken by set; run_box refuses with ERR_NOT_SUPPORTED and launches nothing, run serves the set"""
    case = too_large_case()
    p = place(case)
    tiles, read = new_slab(case)
    g = Handle(L, 2, stream)
    try:
        assert g.set(p) == 0 and g.tiles_bytes() == case.layout()[1]
        assert g.run(tiles, "box") == NOT_SUPPORTED and "3840" in g.error()
        synchronize()
        assert (read()[0] == FILL).all(), "a refused run_box launched something"
        assert g.run(tiles) == 0
        synchronize()
        buf, start = read()
        check_slab("3841x2", case, "run", buf, start)
    finally:
        g.close()
