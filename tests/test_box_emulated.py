"""The area-average downscale without a GPU: the NumPy restatement checked against itself and the host's box rule, the
kernel under the CPU emulator against the restatement (bytes equal, nothing stored outside an image), and what the product
library decides before it needs a device."""
import ctypes as C

import numpy as np
import pytest

import box_ref as BR
import box_support as BS

PAIRS = [(1920, 80), (3840, 200), (1080, 24), (2160, 60), (2160, 240), (7, 7), (4, 7), (3840, 1), (33, 5), (7, 2), (1, 1),
         (300, 2), (3840, 400), (1280, 120)]
CASES = BS.cases()


def _lib():
    L = C.CDLL(BS.LIB)
    L.achip_box_bounds.restype = None
    L.achip_box_bounds.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.asciichat_hip_box_create.restype = C.c_int
    L.asciichat_hip_box_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(BS.Frame), C.c_int]
    L.asciichat_hip_box_downscale.restype = C.c_int
    L.asciichat_hip_box_downscale.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_void_p]
    L.asciichat_hip_device_count.restype = C.c_int
    return L


def test_reference_loop_against_reshape_sum_and_by_hand():
    for (w, h, ow, oh) in ((48, 9, 16, 3), (12, 12, 12, 12), (64, 32, 1, 1), (20, 6, 4, 6)):
        img = BS.noise(w, h, w + h)
        assert np.array_equal(BR.box_ref(img, ow, oh), BR.box_ref_integer_factor(img, ow, oh))
    # rounds half up: (0 + 1) / 2 -> 1, (0 + 0 + 1) / 3 -> 0, (1 + 1 + 0) / 3 -> 1 (2 / 3 rounds up)
    assert BR.box_ref(np.array([[[0, 0, 1]], [[1, 0, 1]]], dtype=np.uint8), 1, 1).tolist() == [[[1, 0, 1]]]
    assert BR.box_ref(np.array([[[0, 1, 255]], [[0, 1, 255]], [[1, 0, 254]]], dtype=np.uint8), 1, 1).tolist() == [[[0, 1, 255]]]
    # flips mirror the averaged image, not the source: 3 -> 2 has boxes [0, 1) and [1, 3)
    row = np.array([[[10, 0, 0], [20, 0, 0], [40, 0, 0]]], dtype=np.uint8)
    assert BR.box_ref(row, 2, 1)[0, :, 0].tolist() == [10, 30]
    assert BR.box_ref(row, 2, 1, flip_x=True)[0, :, 0].tolist() == [30, 10]
    assert BR.box_ref(row[:, ::-1], 2, 1)[0, :, 0].tolist() == [40, 15]
    # an upscaled axis takes one pixel per output
    assert BR.box_ref(row, 7, 1)[0, :, 0].tolist() == [10, 10, 10, 20, 20, 40, 40]


def test_host_box_bounds_is_the_rule():
    L = _lib()
    lo, hi = C.c_int(), C.c_int()
    for src, out in PAIRS:
        prev_hi = 0
        for i in range(out):
            L.achip_box_bounds(src, out, i, C.byref(lo), C.byref(hi))
            assert (lo.value, hi.value) == BR.bounds(src, out, i), (src, out, i)
            assert 0 <= lo.value < hi.value <= src
            if src >= out:  # a partition: boxes meet, first at 0, last at src
                assert lo.value == prev_hi
            prev_hi = hi.value
        if src >= out:
            assert prev_hi == src


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_reference(name):
    img, ow, oh, stride, off, fl = CASES[name]
    h, w = img.shape[:2]
    buf, start, stride_b = BS.place(img, stride, off)
    f = BS.frame_for(buf.ctypes.data + start, w, h, ow, oh, stride, fl)
    images, pitch, uniform = BS.emu_run([f])
    assert uniform
    BS.check_images(images, pitch, [f], [BS.expected(name, CASES[name])], name)
    # a result that depended on bytes outside the image's rows would change with the guard
    buf[buf == BS.GUARD] ^= 0xFF
    for y in range(h):
        buf[start + y * stride_b:start + y * stride_b + 3 * w] = img[y].ravel()
    images2, _, _ = BS.emu_run([f])
    assert np.array_equal(images, images2), name


def test_white_frames_average_to_white():
    for name in CASES:
        if "white" in name:
            assert (BS.expected(name, CASES[name]) == 255).all()


def test_five_geometries_in_one_launch():
    shapes = [(48, 9, 16, 3, 0, 0, 0), (33, 7, 5, 2, 99, 3, BS.FLIP_X), (4, 4, 7, 3, 0, 0, BS.FLIP_Y), (130, 20, 9, 5, 400, 0, 0),
              (64, 300, 2, 1, 0, 0, 3)]
    frames, keep, exp = [], [], []
    for k, (w, h, ow, oh, stride, off, fl) in enumerate(shapes):
        img = BS.noise(w, h, 100 + k) if k != 4 else np.full((h, w, 3), 255, dtype=np.uint8)
        buf, start, _ = BS.place(img, stride, off)
        keep.append(buf)
        frames.append(BS.frame_for(buf.ctypes.data + start, w, h, ow, oh, stride, fl))
        exp.append(BR.box_ref(img, ow, oh, bool(fl & BS.FLIP_X), bool(fl & BS.FLIP_Y)))
    images, pitch, uniform = BS.emu_run(frames)
    assert not uniform
    BS.check_images(images, pitch, frames, exp, "mixed")


def test_forty_equal_frames_take_the_uniform_form():
    w, h, ow, oh, n = 40, 10, 7, 3, 40
    src_pitch = 3 * w * h + 16  # (a multiple of 16: every frame aligned)
    slab = np.full(n * src_pitch + 64, BS.GUARD, dtype=np.uint8)
    base = (-slab.ctypes.data) % 16
    imgs = [BS.noise(w, h, 200 + i) for i in range(n)]
    for i, img in enumerate(imgs):
        slab[base + i * src_pitch:base + i * src_pitch + 3 * w * h] = img.ravel()
    frames = [BS.frame_for(slab.ctypes.data + base + i * src_pitch, w, h, ow, oh, 0, BS.FLIP_X) for i in range(n)]
    exp = [BR.box_ref(img, ow, oh, True, False) for img in imgs]
    images, pitch, uniform = BS.emu_run(frames)
    assert uniform
    BS.check_images(images, pitch, frames, exp, "uniform")
    # the same batch through the descriptor array, and one frame out of step: no longer uniform, the same bytes
    images2, _, uniform2 = BS.emu_run(frames, allow_uniform=False)
    assert not uniform2 and np.array_equal(images, images2)
    frames[17] = BS.frame_for(slab.ctypes.data + base + 17 * src_pitch, w, h, ow, oh, 0, 0)
    exp[17] = BR.box_ref(imgs[17], ow, oh)
    images3, pitch3, uniform3 = BS.emu_run(frames)
    assert not uniform3
    BS.check_images(images3, pitch3, frames, exp, "one frame differs")


def test_library_refuses_before_it_needs_a_device_and_needs_one_after():
    L = _lib()
    NO_DEVICE, NOT_SUPPORTED, INVALID = 200, 30, 86
    img = BS.noise(8, 4, 1)
    h = C.c_void_p()
    good = BS.frame_for(img.ctypes.data, 8, 4, 2, 2)

    def create(f):
        return L.asciichat_hip_box_create(C.byref(h), (BS.Frame * 1)(f), 1)

    def variant(**kw):
        f = BS.frame_for(img.ctypes.data, 8, 4, 2, 2)
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    assert create(variant(comp=img.ctypes.data)) == NOT_SUPPORTED
    for bad in (variant(src=None), variant(src_w=0), variant(src_h=-1), variant(out_w=0), variant(out_h=-3),
                variant(src_stride=23), variant(src_w=3841), variant(src_h=2161)):
        assert create(bad) == INVALID
        assert not h.value
    assert L.asciichat_hip_box_create(C.byref(h), (BS.Frame * 1)(good), 0) == INVALID
    assert L.asciichat_hip_box_create(None, (BS.Frame * 1)(good), 1) == INVALID
    dst = np.zeros(12, dtype=np.uint8)
    assert L.asciichat_hip_box_downscale(None, 8, 4, 0, dst.ctypes.data, 2, 2, 0, 0, None) == INVALID
    assert L.asciichat_hip_box_downscale(img.ctypes.data, 8, 4, 0, None, 2, 2, 0, 0, None) == INVALID
    assert L.asciichat_hip_box_downscale(img.ctypes.data, 8, 4, 20, dst.ctypes.data, 2, 2, 0, 0, None) == INVALID
    assert L.asciichat_hip_box_downscale(img.ctypes.data, 3841, 4, 0, dst.ctypes.data, 2, 2, 0, 0, None) == INVALID
    if L.asciichat_hip_device_count() == 0:
        assert create(good) == NO_DEVICE and not h.value
        assert L.asciichat_hip_box_downscale(img.ctypes.data, 8, 4, 0, dst.ctypes.data, 2, 2, 0, 0, None) == NO_DEVICE
