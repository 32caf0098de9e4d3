"""Grid composites through the area-average pass, test support: the emulator driver (tests/hipemu/box_comp_emu_driver.cpp)
and the scenes the emulated and the GPU tests share -- sources, the composite descriptor over them (achip_composite_setup of
the product library, or filled by hand), the geometry that setup is expected to give, the averaged sizes to run.  TESTS ONLY."""
import ctypes as C

import numpy as np

import box_comp_ref as CR
import box_support as BS
import emubuild


class CompSrc(C.Structure):  # achip_comp_src_t (include/achip_types.h)
    _fields_ = [("src", C.c_void_p), ("src_w", C.c_int32), ("src_h", C.c_int32), ("src_stride", C.c_int32),
                ("_pad0", C.c_int32), ("tile_w", C.c_int32), ("tile_h", C.c_int32), ("org_x", C.c_int32),
                ("org_y", C.c_int32), ("x_ratio", C.c_uint32), ("y_ratio", C.c_uint32)]


class Composite(C.Structure):  # achip_composite_t
    _fields_ = [("canvas_w", C.c_int32), ("canvas_h", C.c_int32), ("cols", C.c_int32), ("rows", C.c_int32),
                ("cell_w", C.c_int32), ("cell_h", C.c_int32), ("n_src", C.c_int32), ("_pad", C.c_int32),
                ("s", CompSrc * 9)]


_emu = None
_lib = None


def emulator():
    global _emu
    if _emu is None:
        L = C.CDLL(emubuild.shared_library("libbox_comp_emu.so", "box_comp_emu_driver.cpp", ("box_kernels.hpp", "box.h", "achip_types.h")))
        L.emu_box_composites.restype = C.c_int
        L.emu_box_composites.argtypes = [C.POINTER(BS.Frame), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_uint64,
                                         C.POINTER(C.c_int)]
        _emu = L
    return _emu


def lib():
    """the product library's host helpers (no device needed)"""
    global _lib
    if _lib is None:
        L = C.CDLL(BS.LIB)
        L.achip_composite_setup.restype = None
        L.achip_composite_setup.argtypes = [C.POINTER(Composite), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                            C.c_int, C.c_int, C.c_int]
        L.asciichat_hip_box_composites.restype = C.c_int
        L.asciichat_hip_box_composites.argtypes = [C.POINTER(C.c_void_p), C.POINTER(BS.Frame), C.POINTER(C.c_void_p), C.c_int,
                                                   C.c_void_p]
        L.asciichat_hip_device_count.restype = C.c_int
        _lib = L
    return _lib


def setup(addrs, sizes, term_w, term_h):
    """achip_composite_setup over sources at addrs[i] (0: none) of sizes[i] = (w, h)"""
    n = len(addrs)
    comp = Composite()
    lib().achip_composite_setup(C.byref(comp), (C.c_void_p * n)(*[a or None for a in addrs]), (C.c_int * n)(*[s[0] for s in sizes]),
                                (C.c_int * n)(*[s[1] for s in sizes]), n, term_w, term_h)
    return comp


def geometry(comp):
    """what the tests pin of a descriptor: (canvas, grid, cells, n_src, [(tile_w, tile_h, org_x, org_y) of placed sources])"""
    return ((comp.canvas_w, comp.canvas_h), (comp.cols, comp.rows), (comp.cell_w, comp.cell_h), comp.n_src,
            [(s.tile_w, s.tile_h, s.org_x, s.org_y) for s in list(comp.s)[:comp.n_src] if s.src])


class Scene:
    """sources: [(image or None, stride (0 = tight), byte offset from a 16-byte boundary)], in the order given to setup; one
    buffer per source unless share_address.  term: the terminal achip_composite_setup lays out for, or fill: a function
    (scene, addresses of the sources) -> Composite.  expect: geometry() of the descriptor.  sizes: [(out_w, out_h, flips)]."""

    def __init__(self, sources, sizes, term=None, fill=None, expect=None, share_address=False, tiles=None):
        self.sources, self.sizes, self.term, self.fill, self.expect = sources, sizes, term, fill, expect
        self.share_address, self.tiles = share_address, tiles
        self._canvas, self._expected = None, {}

    def placed_images(self):
        """the images by placed index k (setup skips absent sources and stops at nine)"""
        return [img for img, _, _ in self.sources if img is not None][:9]

    def build(self, upload=None):
        """-> (Composite, the buffers to keep alive).  upload: buffer -> (device tensor, its address), for the GPU tests;
        None: the sources stay in host memory (the emulator)"""
        keep, addrs, strides = [], [], []
        for i, (img, stride, off) in enumerate(self.sources):
            if img is None:
                addrs.append(0)
                strides.append(0)
                continue
            if self.share_address and i > 0:
                addrs.append(addrs[0])
                strides.append(strides[0])
                continue
            buf, start, stride_b = BS.place(img, stride, off, base=0 if upload else None)
            if upload:
                t, base = upload(buf)
                keep.append(t)
            else:
                base = buf.ctypes.data
                keep.append(buf)
            addrs.append(base + start)
            strides.append(stride_b)
        if self.fill:
            comp = self.fill(self, addrs)
        else:
            comp = setup(addrs, [(0, 0) if img is None else img.shape[1::-1] for img, _, _ in self.sources], *self.term)
        k = 0
        for a, st in zip(addrs, strides):  # setup assumes tight rows: the padded strides go in by hand
            if a and k < 9:
                if comp.s[k].src:
                    assert comp.s[k].src == a
                    comp.s[k].src_stride = st
                k += 1
        return comp, keep

    def expected(self, comp, out_w, out_h, flips=0):
        """composite_ref of the scene at one averaged size, the canvas and each size computed once"""
        if self._canvas is None:
            self._canvas = CR.canvas_ref(comp, CR.tiles_ref(comp, self.placed_images()))
            self._canvas.setflags(write=False)
        key = (out_w, out_h, flips)
        if key not in self._expected:
            e = CR.BR.box_ref(self._canvas, out_w, out_h, bool(flips & BS.FLIP_X), bool(flips & BS.FLIP_Y))
            e.setflags(write=False)
            self._expected[key] = e
        return self._expected[key]


def frame_for(comp, out_w, out_h, flips=0, ops=0):
    """the render descriptor of a composite frame: the canvas as its source size; src and comp are not read"""
    f = BS.Frame()
    f.src_w, f.src_h, f.out_w, f.out_h, f.ops = comp.canvas_w, comp.canvas_h, out_w, out_h, flips | ops
    f.x_ratio, f.y_ratio = (comp.canvas_w << 16) // out_w + 1, (comp.canvas_h << 16) // out_h + 1
    return f


def comp_array(comps):
    """the comps_host argument: pointers to the descriptors, NULL for a plain frame"""
    return (C.c_void_p * len(comps))(*[C.addressof(c) if c is not None else None for c in comps])


def emu_run(frames, comps):
    """-> (images, pitch, {tiles, plain, canvas, launches}) of a batch under the emulator"""
    arr = (BS.Frame * len(frames))(*frames)
    pitch = BS.pitch_of(frames)
    images = np.full(len(frames) * pitch + 256, BS.FILL, dtype=np.uint8)
    counts = (C.c_int * 4)()
    rc = emulator().emu_box_composites(arr, comp_array(comps), len(frames), images.ctypes.data, pitch, counts)
    assert rc == 0, f"refused: {-rc} (frame {counts[0]}, source {counts[1]})"
    return images, pitch, dict(tiles=counts[0], plain=counts[1], canvas=counts[2], launches=counts[3])


def _hand(canvas, grid, cell, tiles, n_src=None):
    """a descriptor filled by hand: tiles = [(tile_w, tile_h, org_x, org_y)] for the sources in order"""
    def fill(scene, addrs):
        c = Composite()
        c.canvas_w, c.canvas_h = canvas
        c.cols, c.rows = grid
        c.cell_w, c.cell_h = cell
        c.n_src = len(tiles) if n_src is None else n_src
        for k, ((tw, th, ox, oy), a, (img, stride, _)) in enumerate(zip(tiles, addrs, scene.sources)):
            s = c.s[k]
            s.src, s.src_w, s.src_h, s.src_stride = a, img.shape[1], img.shape[0], stride or 3 * img.shape[1]
            s.tile_w, s.tile_h, s.org_x, s.org_y = tw, th, ox, oy
            s.x_ratio, s.y_ratio = 0xDEAD, 0xBEEF  # not read
        return c
    return fill


def _white(w, h):
    return np.full((h, w, 3), 255, dtype=np.uint8)


def scenes():
    n = BS.noise
    all_flips = lambda sizes: [(w, h, fl) for (w, h) in sizes for fl in range(4)]  # noqa: E731
    plain = lambda sizes: [(w, h, 0) for (w, h) in sizes]  # noqa: E731
    return {
        "two sources on 16x4": Scene(
            [(n(32, 18, 21), 0, 0), (n(20, 30, 22), 67, 5)], all_flips([(16, 8), (16, 4), (5, 3)]), term=(16, 4),
            expect=((16, 8), (1, 2), (16, 4), 2, [(7, 4, 4, 0), (3, 4, 6, 4)]), tiles=2),
        "four slots, one empty, on 60x20": Scene(
            [(n(64, 36, 23), 0, 0), (None, 0, 0), (n(17, 33, 24), 0, 3), (n(40, 40, 25), 3 * 40 + 16, 0)],
            plain([(60, 40), (60, 20), (7, 7)]), term=(60, 20),
            expect=((60, 40), (2, 2), (30, 20), 3, [(30, 17, 0, 1), (10, 20, 40, 0), (20, 20, 5, 20)]), tiles=3),
        "nine sources on 8x4: cell_h 0": Scene(
            [(n(64, 36, 30 + i), 0, 0) for i in range(9)], plain([(8, 8), (3, 2)]), term=(8, 4),
            expect=((8, 8), (1, 9), (8, 0), 9, []), tiles=0),
        "7x5 upscaled on 9x3": Scene(
            [(n(7, 5, 40), 0, 1)], plain([(9, 6), (9, 3)]), term=(9, 3),
            expect=((9, 6), (1, 1), (9, 6), 1, [(8, 6, 0, 0)]), tiles=1),
        "200x3 and 64x36 on 40x10": Scene(
            [(n(200, 3, 41), 0, 0), (n(64, 36, 42), 0, 0)], plain([(40, 20), (13, 5)]), term=(40, 10),
            expect=((40, 20), (1, 2), (40, 10), 2, [(40, 1, 0, 4), (18, 10, 11, 10)]), tiles=2),
        "ten sources at one address on 90x30": Scene(
            [(n(64, 36, 43), 0, 0)] * 10, plain([(90, 60)]), term=(90, 30), share_address=True,
            expect=((90, 60), (4, 3), (22, 20), 9, [(22, 12, 22 * (k % 4), 20 * (k // 4) + 4) for k in range(9)]), tiles=1),
        # ---- filled by hand
        "a tile wider than its cell": Scene(
            [(n(30, 12, 50), 0, 0), (n(9, 9, 51), 0, 7)], plain([(12, 6), (5, 2)]),
            fill=_hand((12, 6), (2, 1), (6, 6), [(9, 6, 0, 0), (4, 4, 7, 1)]), tiles=2),
        "negative origins": Scene(
            [(n(16, 12, 52), 0, 0), (n(11, 7, 53), 40, 2)], plain([(10, 8), (4, 3)]),
            fill=_hand((10, 8), (1, 2), (10, 4), [(8, 6, -3, -2), (6, 5, -2, 3)]), tiles=2),
        "more cells than sources": Scene(
            [(n(12, 8, 54), 0, 0), (n(6, 4, 55), 0, 0)], plain([(12, 8), (5, 3)]),
            fill=_hand((12, 8), (2, 2), (6, 4), [(6, 4, 0, 0), (5, 3, 6, 1)]), tiles=2),
        "3840x2 white canvas-wide tile -> 1x1": Scene(
            [(_white(3840, 2), 0, 0)], plain([(1, 1)]), fill=_hand((3840, 2), (1, 1), (3840, 2), [(3840, 2, 0, 0)]), tiles=1),
    }
