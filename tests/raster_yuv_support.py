"""Support of the rasteriser's YUV 4:2:0 tests: draw_yuv_kernel under the CPU emulator (tests/hipemu/raster_yuv_emu_driver.cpp),
one more atlas, guard-filled plane buffers, and the case table the emulated and the GPU tests share -- every case with even
width and height, each run in both layouts.  Builds on raster_support.py.  TESTS ONLY."""
import ctypes as C

import numpy as np

import emubuild
import raster_ref as RR
import raster_support as RS
import raster_yuv_ref as YR

FILL = RS.FILL
LAYOUTS = {"I420": YR.I420, "NV12": YR.NV12}

_emu = None


def emulator():
    global _emu
    if _emu is None:
        L = C.CDLL(emubuild.shared_library("libraster_yuv_emu.so", "raster_yuv_emu_driver.cpp",
                                           ("raster_yuv_kernels.hpp", "raster_yuv.h", "raster_kernels.hpp", "raster.h", "asciichat_raster.h",
                                            "achip_types.h")))
        L.emu_raster_yuv_tile.restype = C.c_int
        L.emu_raster_yuv_tile.argtypes = [C.c_int]
        L.emu_raster_yuv_convert.restype = None
        L.emu_raster_yuv_convert.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.emu_raster_yuv_avg.restype = C.c_uint32
        L.emu_raster_yuv_avg.argtypes = [C.c_uint32]
        L.emu_raster_yuv_all.restype = None
        L.emu_raster_yuv_all.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.emu_raster_yuv.restype = C.c_int
        L.emu_raster_yuv.argtypes = [C.POINTER(RS.CFont), C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_uint64, C.c_int, C.c_void_p, C.c_int, C.c_int]
        _emu = L
    return _emu


def tile_px(atlas="one"):
    """the kernel's tile width in pixels with that atlas' cells, as built"""
    return emulator().emu_raster_yuv_tile(RS.ATLASES[atlas].cell_w)


# ---- one more atlas -----------------------------------------------------------------------------------------------------------
def _synth_5x8():
    """the glyph set of `synth` in a 5x8 cell (odd width, even height), the baseline one lower: every rectangle one row further
    down, still within [-5, 10] x [-8, 16]"""
    src = RS.ATLASES["synth"]
    spec = []
    for g in src.glyphs:
        body = src.coverage[g.offset:g.offset + g.rows * g.pitch].reshape(g.rows, g.pitch)[:, :g.width]
        spec.append((g.codepoint, g.left, g.top, g.width, g.rows, g.pitch, body))
    return RS._atlas(5, 8, 6, spec, 8, default_fg=0xC8C9CA, default_bg=0x101112, flat_fg=0xCCCCCC, flat_bg=0x000000)


RS.ATLASES.setdefault("synth58", _synth_5x8())


# ---- cases --------------------------------------------------------------------------------------------------------------------
def _colours(k):
    return RS.fgc(200 - 20 * k, 10 + 25 * k, 90 + k) + RS.bgc(5 + 11 * k, 250 - 9 * k, 40 + 17 * k)


def _four_cell_frames():
    """4 x 2 cells of `synth`: each overhanging glyph at each of the 8 positions among other glyphs, then overhangs that meet"""
    others = ["A", "P", "L", "R", "U", "D", "Z", "é", "▀"]
    out = []
    for gi, g in enumerate("LRUDZB"):
        for pos in range(8):
            rows = []
            for r in range(2):
                row = b""
                for c in range(4):
                    k = 4 * r + c
                    row += _colours(k) + RS._u(g if k == pos else others[(k + gi + pos) % len(others)])
                rows.append(row)
            out.append(b"\n".join(rows))
    red, green = RS.fgc(255, 0, 0) + RS.bgc(0, 0, 60), RS.fgc(0, 255, 0) + RS.bgc(60, 0, 0)
    # R from the left and L from the right over the blank between them, in both rows; D from above and U from below
    out.append(red + b"R" + RS.sgr(0) + b" " + green + b"L" + RS.sgr(0) + b" \n " + red + b"R" + RS.sgr(0) + b" " + green + b"L")
    out.append(red + b" D D\n" + green + b" U U")
    return out


def _three_row_frames(rows):
    """2 cells wide, odd cell height: D in row 1 reaches into row 2 across a pair boundary, B in row 2 reaches up"""
    if rows == 4:
        return [_colours(0) + b"AP\n" + _colours(1) + b"DA\n" + _colours(2) + b"BL\n" + _colours(3) + b"UR",
                _colours(4) + b"UD\n" + _colours(5) + b"PD\n" + _colours(6) + b"LB\n" + _colours(7) + b"ZU",
                b"\n" + _colours(2) + b"D\n\n" + _colours(5) + b" B", b"BB\nBB\nBB\nBB"]
    return [_colours(0) + b"DB\n" + _colours(3) + b"UL", _colours(1) + b"BD\n" + _colours(2) + b"BU", b"A"]


def _text_frames():
    return [RS.fgc(250, 200, 10) + b"Why?\n" + RS.bgc(0, 40, 90) + b"g{}_", RS.sgr(31) + b"Qj" + RS.sgr(44) + b"|W\n" + RS._u("▀▀▀▀")]


def _tile_frames(cols, rows):
    body = (RS.fgc(250, 240, 230) + b"xo" + RS.bgc(3, 99, 180) + b"ox" + RS.fgc(9, 120, 33) + b"oo" + RS.bgc(200, 0, 77) + b"x") * (cols // 7 + 1)
    one = b"".join(RS.fgc(k * 37 % 256, k * 91 % 256, k * 53 % 256) + b"o" for k in range(cols))
    return [b"\n".join([one, body][(r + 1) % 2] for r in range(rows)), b"o" * cols]


def cases():
    T = tile_px()
    c = {}
    c["yuv smallest image"] = RS.Case("one", 2, 2, [RS.fgc(255, 0, 0) + b"xo\n" + RS.bgc(0, 0, 255) + b"ox", b"", b"o"])
    c["yuv odd plane starts"] = RS.Case("one", 6, 2, [RS.fgc(255, 255, 255) + b"xoxoxo\n" + RS.bgc(90, 0, 0) + b"ooxx o", b"x"])
    c["yuv chroma across four cells"] = RS.Case("synth", 4, 2, _four_cell_frames())
    c["yuv three cell rows 2x4"] = RS.Case("synth", 2, 4, _three_row_frames(4))
    c["yuv three cell rows 2x2"] = RS.Case("synth", 2, 2, _three_row_frames(2))
    c["yuv odd width, even height"] = RS.Case("synth58", 4, 3, [_colours(1) + b"LRUD\n" + _colours(4) + b"ZBAP\n" + _colours(6) + b"DULR",
                                                               b"BBBB\nBBBB\nBBBB"])
    c["yuv even width, odd height"] = RS.Case("text", 4, 2, _text_frames())
    c["yuv division pin"] = RS.Case("ramp", 16, 16, [RS._division_frame()])
    for cols, rows in ((T + 2, 2), (2 * T + 2, 4), (T - 2, 2)):
        c[f"yuv tile edges {cols}x{rows}"] = RS.Case("one", cols, rows, _tile_frames(cols, rows))
    big = RS.fgc(255, 128, 0) + RS.bgc(0, 64, 128)
    c["yuv cell 32x64 single cell"] = RS.Case("big", 1, 1, [big + b"G", b"H", b" "], pitch_extra=16)
    c["yuv cell 32x64 2x2"] = RS.Case("big", 2, 2, [RS.fgc(255, 128, 0) + b"GH\n" + RS.bgc(0, 64, 128) + b"HG"])
    c["yuv cell 32x64 2x2 atlas through L2"] = RS.Case("big", 2, 2, [big + b"HG\nGH"], l2=True)
    geo = RS.fgc(200, 100, 50) + b"AR\n" + RS.bgc(20, 40, 60) + b"UD"
    for off in (0, 4, 8, 12):
        for extra in (4, 20):
            c[f"yuv 10x14 base +{off} pitch +{extra}"] = RS.Case("synth", 2, 2, [geo, geo[::-1], geo], base_off=off, pitch_extra=extra)
    # 1088 strips of 288 slots each: as in a large batch, one workgroup walks a strip and every thread holds more than one slot
    many = [b"\n".join(RS.fgc((r * 4 + k) % 256, 255 - r * 3, r) + RS.bgc(200 - r, r * 2, 77 * k) + b"r" * 9 for r in range(64)) for k in range(3)]
    c["yuv many strips"] = RS.Case("ramp", 9, 64, [many[i % 3] for i in range(17)])
    c["yuv batch of 40"] = RS.Case("synth", 8, 4, RS._batch_frames(), stride_extra=3)
    c["yuv flags"] = RS.Case("synth", 4, 2, [f for f, _ in RS._flag_frames()] + RS._grammar_frames())
    return c


# ---- running a case -----------------------------------------------------------------------------------------------------------
def size_px(case):
    return case.cols * case.font.cell_w, case.rows * case.font.cell_h


def image_bytes(case):
    W, H = size_px(case)
    return W * H * 3 // 2


def yuv_buffer(case, base=None):
    """-> (guard-filled buffer, byte index of image 0, pitch): image 0 `base_off` bytes behind a 16-byte boundary of the address
    the buffer's bytes will live at (base: a device copy's); the pitch is the image rounded up to 4, plus pitch_extra"""
    pitch = (image_bytes(case) + 3) // 4 * 4 + case.pitch_extra
    buf = np.full(64 + 16 + case.base_off + len(case.frames) * pitch + 256, FILL, dtype=np.uint8)
    start = 64 + (-((buf.ctypes.data if base is None else base) + 64)) % 16 + case.base_off
    return buf, start, pitch


_rendered, _expected = {}, {}


def _render(case, frame):
    """(image, status) of one frame by raster_ref, once per distinct frame of a grid: batches repeat frames"""
    key = (case.atlas, case.cols, case.rows, frame)
    if key not in _rendered:
        img, st = RR.render(frame, case.cols, case.rows, case.font)
        img.setflags(write=False)
        _rendered[key] = (img, st)
    return _rendered[key]


def expected(name, case, layout):
    """[(planes, status)] of a case's frames: the conversion restated over the render restated (computed once each)"""
    key = (name, layout)
    if key not in _expected:
        out = []
        for f in case.frames:
            img, st = _render(case, f)
            planes = YR.yuv420(img, layout)
            planes.setflags(write=False)
            out.append((planes, st))
        _expected[key] = out
    return _expected[key]


def first_difference(got, exp, W, H):
    i = int(np.argmax(got != exp))
    if i < W * H:
        return f"Y at (y {i // W}, x {i % W}): {int(got[i])}, restatement {int(exp[i])}"
    return f"chroma byte {i - W * H} of {W * H // 2}: {int(got[i])}, restatement {int(exp[i])}"


def check(name, case, layout, planes, start, pitch, status):
    exp = expected(name, case, layout)
    W, H = size_px(case)
    nb = image_bytes(case)
    assert (planes[:start] == FILL).all(), f"{name}: a store in front of the first image"
    for i, (want, st) in enumerate(exp):
        got = planes[start + i * pitch:start + i * pitch + nb]
        assert np.array_equal(got, want), f"{name} frame {i}: {first_difference(got, want, W, H)}"
        assert (planes[start + i * pitch + nb:start + (i + 1) * pitch] == FILL).all(), f"{name} frame {i}: a store beyond the image"
        assert int(status[i]) == st, f"{name} frame {i}: status {int(status[i])}, restatement {st}"
        if case.status is not None:
            assert st == case.status[i], f"{name} frame {i}: the restatement reports {st}, the case expects {case.status[i]}"
    assert (planes[start + len(exp) * pitch:] == FILL).all(), f"{name}: a store past the last image"


def emu_run(case, layout, split=0):
    """-> (planes, start, pitch, status).  split: the workgroups a strip's slots are spread over (0: as the library chooses)"""
    n = len(case.frames)
    frames, stride, lens = RS.slab(case)
    planes, start, pitch = yuv_buffer(case)
    status = np.full(n, 0xABABABAB, dtype=np.uint32)
    font = RS.c_font(case.font)
    rc = emulator().emu_raster_yuv(C.byref(font), case.cols, case.rows, frames.ctypes.data, stride, lens.ctypes.data, n,
                                   planes.ctypes.data + start, pitch, layout, status.ctypes.data, int(case.l2), split)
    assert rc == 0, f"refused ({rc})"
    return planes, start, pitch, status

