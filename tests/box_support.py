"""Area-average downscale test support: the kernel under the CPU emulator (tests/hipemu/box_emu_driver.cpp), guard-filled
source buffers, and the cases the emulated and the GPU tests share.  TESTS ONLY."""
import ctypes as C
import os

import numpy as np

import box_ref as BR
import emubuild

LIB = os.path.join(emubuild.ROOT, "ascii-chat_amd", "libasciichat_hip.so")
FLIP_X, FLIP_Y = 1, 2
FILL = 0xEE   # every image slot before the pass
GUARD = 0xA5  # around and between the rows of a source


class Frame(C.Structure):  # achip_frame_t (include/achip_types.h)
    _fields_ = [("src", C.c_void_p), ("comp", C.c_void_p), ("src_w", C.c_int32), ("src_h", C.c_int32),
                ("out_w", C.c_int32), ("out_h", C.c_int32), ("pad_left", C.c_int32), ("pad_top", C.c_int32),
                ("x_ratio", C.c_uint32), ("y_ratio", C.c_uint32), ("src_stride", C.c_int32), ("ops", C.c_uint32)]


_emu = None


def emulator():
    global _emu
    if _emu is None:
        L = C.CDLL(emubuild.shared_library("libbox_emu.so", "box_emu_driver.cpp", ("box_kernels.hpp", "box.h", "achip_types.h")))
        L.emu_box.restype = C.c_int
        L.emu_box.argtypes = [C.POINTER(Frame), C.c_int, C.c_void_p, C.c_uint64, C.c_int]
        _emu = L
    return _emu


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def place(img, stride=0, offset=0, base=None):
    """-> (buffer, byte index of the image's first pixel, stride in bytes): the image's rows `stride` bytes apart (0 = tight)
    inside a guard-filled buffer, its first byte at a 16-byte aligned address plus `offset`; the last row ends where its
    pixels end.  base: the address the buffer's bytes will live at when that is not the array's own (a device copy)."""
    h, w = img.shape[:2]
    stride = stride or 3 * w
    buf = np.full(64 + 16 + offset + (h - 1) * stride + 3 * w + 64, GUARD, dtype=np.uint8)
    start = 64 + (-((buf.ctypes.data if base is None else base) + 64)) % 16 + offset
    for y in range(h):
        buf[start + y * stride:start + y * stride + 3 * w] = img[y].ravel()
    return buf, start, stride


def frame_for(addr, w, h, out_w, out_h, stride=0, flips=0, ops=0):
    f = Frame()
    f.src, f.src_w, f.src_h, f.out_w, f.out_h, f.src_stride, f.ops = addr, w, h, out_w, out_h, stride, flips | ops
    f.x_ratio, f.y_ratio = (w << 16) // out_w + 1, (h << 16) // out_h + 1
    return f


def pitch_of(frames):
    return (max(3 * f.out_w * f.out_h for f in frames) + 127) // 128 * 128


def check_images(images, pitch, frames, expected, what=""):
    """every image equal to its expectation, every other byte of the slots (and behind them) still FILL"""
    for i, (f, exp) in enumerate(zip(frames, expected)):
        nb = 3 * f.out_w * f.out_h
        got = images[i * pitch:i * pitch + nb].reshape(f.out_h, f.out_w, 3)
        assert np.array_equal(got, exp), f"{what} frame {i}: {np.argwhere(got != exp)[:4].tolist()}"
        assert (images[i * pitch + nb:(i + 1) * pitch] == FILL).all(), f"{what} frame {i}: a store beyond the image"
    assert (images[len(frames) * pitch:] == FILL).all(), f"{what}: a store past the last slot"


def emu_run(frames, allow_uniform=True):
    """-> (images, pitch, whether the launch took its uniform form)"""
    arr = (Frame * len(frames))(*frames)
    pitch = pitch_of(frames)
    images = np.full(len(frames) * pitch + 256, FILL, dtype=np.uint8)
    rc = emulator().emu_box(arr, len(frames), images.ctypes.data, pitch, 1 if allow_uniform else 0)
    assert rc >= 0, f"refused: {-rc}"
    return images, pitch, bool(rc)


# ---- the cases both suites run: name -> (image, out_w, out_h, stride, offset, flips) ------------------------------------------
def _white(w, h):
    return np.full((h, w, 3), 255, dtype=np.uint8)


def cases():
    out = {
        "48x9->16x3 integer boxes": (noise(48, 9, 1), 16, 3, 0, 0, 0),
        "16x4 identity": (noise(16, 4, 2), 16, 4, 0, 0, 0),
        "1x1": (noise(1, 1, 3), 1, 1, 0, 0, 0),
        "1x5->1x1": (noise(1, 5, 4), 1, 1, 0, 0, 0),
        "5x1->3x1": (noise(5, 1, 5), 3, 1, 0, 0, 0),
        "4x4->7x3 x upscaled": (noise(4, 4, 6), 7, 3, 0, 0, 0),
        "64x300 white ->1x1 (16-bit sums)": (_white(64, 300), 1, 1, 0, 0, 0),
        "300x300 white ->1x1 (sums past 2^24)": (_white(300, 300), 1, 1, 0, 0, 0),
        "300x300 white ->2x2": (_white(300, 300), 2, 2, 0, 0, 0),
        "64x600 noise ->3x2 (flushed sums add up)": (noise(64, 600, 7), 3, 2, 0, 0, 0),
        "3840x2->80x1 widest stage": (noise(3840, 2, 8), 80, 1, 0, 0, 0),
        "3840x2->3840x1": (noise(3840, 2, 9), 3840, 1, 0, 0, 0),
    }
    for fl in range(4):
        out[f"33x7->5x2 stride 99 flips {fl}"] = (noise(33, 7, 10), 5, 2, 99, 0, fl)
    for off in (1, 7, 15):
        out[f"48x6->8x2 base +{off}"] = (noise(48, 6, 11), 8, 2, 0, off, 0)
    for extra in (5, 16):
        out[f"48x6->8x2 stride 3w+{extra}"] = (noise(48, 6, 12), 8, 2, 3 * 48 + extra, 0, 0)
    return out


_expected = {}


def expected(name, case):
    """box_ref of a case, computed once"""
    if name not in _expected:
        img, ow, oh, _, _, fl = case
        e = BR.box_ref(img, ow, oh, bool(fl & FLIP_X), bool(fl & FLIP_Y))
        e.setflags(write=False)
        _expected[name] = e
    return _expected[name]
