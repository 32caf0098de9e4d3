"""Grid composites through the area-average pass without a GPU: the plan step, box_kernel over the tiles and
box_canvas_kernel under the CPU emulator against the NumPy restatement over box_ref (bytes equal, nothing stored outside an
image), the unique tiles the plan step reports, and what the product library refuses before it needs a device."""
import ctypes as C

import numpy as np
import pytest

import box_comp_ref as CR
import box_comp_support as CS
import box_ref as BR
import box_support as BS

SCENES = CS.scenes()
PLAIN, TILES, CANVAS = 1, 2, 4  # the launches the driver reports


def test_setup_gives_the_geometries_the_cases_were_chosen_for():
    for name, sc in SCENES.items():
        if sc.expect is not None:
            comp, _ = sc.build()
            assert CS.geometry(comp) == sc.expect, name


def test_oracle_by_hand():
    # one 2x2 source shown 1:1 at (1, 0) of a 4x2 canvas of one cell: black, the tile, black
    img = np.array([[[10, 20, 30], [50, 60, 70]], [[90, 100, 110], [130, 140, 150]]], dtype=np.uint8)
    c = CS.Composite()
    c.canvas_w, c.canvas_h, c.cols, c.rows, c.cell_w, c.cell_h, c.n_src = 4, 2, 1, 1, 4, 2, 1
    s = c.s[0]
    s.src, s.src_w, s.src_h, s.src_stride, s.tile_w, s.tile_h, s.org_x, s.org_y = 1, 2, 2, 6, 2, 2, 1, 0
    canvas = CR.canvas_ref(c, CR.tiles_ref(c, [img]))
    assert canvas[:, 0].tolist() == [[0, 0, 0]] * 2 and canvas[:, 3].tolist() == [[0, 0, 0]] * 2
    assert np.array_equal(canvas[:, 1:3], img)
    # black counts in n: columns {0, 1} and {2, 3}, both rows -> (10 + 90 + 2) // 4 and (50 + 130 + 2) // 4 in red
    assert CR.composite_ref(c, [img], 2, 1)[0, :, 0].tolist() == [25, 45]
    assert CR.composite_ref(c, [img], 2, 1, flip_x=True)[0, :, 0].tolist() == [45, 25]
    # rounded twice: the tile first (1x1: (10 + 50 + 90 + 130 + 2) // 4 = 70), then the canvas ((70 + 4) // 8 = 9)
    s.tile_w = s.tile_h = 1
    assert CR.composite_ref(c, [img], 1, 1)[0, 0, 0] == 9
    # a cell size of 0: black
    c.cell_h = 0
    assert not CR.composite_ref(c, [img], 2, 1).any()


@pytest.mark.parametrize("name", list(SCENES))
def test_kernels_match_reference(name):
    sc = SCENES[name]
    comp, keep = sc.build()
    frames = [CS.frame_for(comp, ow, oh, fl) for ow, oh, fl in sc.sizes]
    exp = [sc.expected(comp, ow, oh, fl) for ow, oh, fl in sc.sizes]
    images, pitch, counts = CS.emu_run(frames, [comp] * len(frames))
    BS.check_images(images, pitch, frames, exp, name)
    assert counts["tiles"] == sc.tiles and counts["plain"] == 0 and counts["canvas"] == len(frames)
    assert counts["launches"] == (CANVAS | TILES if sc.tiles else CANVAS), name  # nothing to do: no launch
    if sc.tiles == 0:
        assert not any(e.any() for e in exp)
    # one frame at a time gives the same bytes
    for f, e in zip(frames[:2], exp[:2]):
        one, p1, _ = CS.emu_run([f], [comp])
        BS.check_images(one, p1, [f], [e], name + " alone")
    # a result that depended on bytes outside the sources' rows would change with the guard
    for buf in keep:
        buf[buf == BS.GUARD] ^= 0xFF
    for k, img in enumerate(sc.placed_images()):
        s = comp.s[k]
        if s.src:
            host = next(b for b in keep if b.ctypes.data <= s.src < b.ctypes.data + b.size)
            off = s.src - host.ctypes.data
            for y in range(img.shape[0]):
                host[off + y * s.src_stride:off + y * s.src_stride + 3 * img.shape[1]] = img[y].ravel()
    images2, _, _ = CS.emu_run(frames, [comp] * len(frames))
    assert np.array_equal(images, images2), name


def test_white_tile_through_the_widest_stage_is_white():
    sc = SCENES["3840x2 white canvas-wide tile -> 1x1"]
    comp, _ = sc.build()
    assert sc.expected(comp, 1, 1).tolist() == [[[255, 255, 255]]]


def test_descriptors_that_are_valid_and_all_black():
    sc = SCENES["four slots, one empty, on 60x20"]
    comp, _keep = sc.build()
    for kw in (dict(cell_w=0), dict(cell_w=-1), dict(cell_h=0), dict(n_src=0), dict(cols=0), dict(rows=0)):
        c = CS.Composite.from_buffer_copy(bytes(comp))
        for k, v in kw.items():
            setattr(c, k, v)
        frames = [CS.frame_for(c, 60, 20), CS.frame_for(c, 7, 7, 3)]
        images, pitch, counts = CS.emu_run(frames, [c, c])
        BS.check_images(images, pitch, frames, [np.zeros((f.out_h, f.out_w, 3), dtype=np.uint8) for f in frames], str(kw))
        assert counts["tiles"] == 0 and counts["launches"] == CANVAS, kw
        assert not CR.composite_ref(c, sc.placed_images(), 7, 7).any()


def test_mixed_batch_of_two_plain_and_three_composite_frames():
    a, b = SCENES["four slots, one empty, on 60x20"], SCENES["negative origins"]
    ca, keep_a = a.build()
    cb, keep_b = b.build()
    imgs = [BS.noise(33, 7, 60), BS.noise(48, 9, 61)]
    placed = [BS.place(imgs[0], 99, 3), BS.place(imgs[1])]
    p0 = BS.frame_for(placed[0][0].ctypes.data + placed[0][1], 33, 7, 5, 2, 99, BS.FLIP_X)
    p1 = BS.frame_for(placed[1][0].ctypes.data + placed[1][1], 48, 9, 16, 3)
    frames = [CS.frame_for(ca, 60, 20), p0, CS.frame_for(cb, 4, 3, BS.FLIP_Y), CS.frame_for(ca, 7, 7, 3), p1]
    comps = [ca, None, cb, ca, None]
    exp = [a.expected(ca, 60, 20), BR.box_ref(imgs[0], 5, 2, True, False), b.expected(cb, 4, 3, BS.FLIP_Y),
           a.expected(ca, 7, 7, 3), BR.box_ref(imgs[1], 16, 3)]
    images, pitch, counts = CS.emu_run(frames, comps)
    BS.check_images(images, pitch, frames, exp, "mixed")
    assert counts == dict(tiles=5, plain=2, canvas=3, launches=PLAIN | TILES | CANVAS)
    # all plain: one launch, as before
    images, pitch, counts = CS.emu_run([p0, p1], [None, None])
    BS.check_images(images, pitch, [p0, p1], [exp[1], exp[4]], "plain only")
    assert counts == dict(tiles=0, plain=2, canvas=0, launches=PLAIN)


def test_unique_tiles_over_a_batch():
    one = SCENES["ten sources at one address on 90x30"]
    comp, _keep = one.build()
    _, _, counts = CS.emu_run([CS.frame_for(comp, 90, 60)], [comp])
    assert counts["tiles"] == 1
    nine = CS.Scene([(BS.noise(64, 36, 70 + i), 0, 0) for i in range(9)], [(45, 30, 0)], term=(90, 30))
    c1, keep1 = nine.build()
    assert len(CS.geometry(c1)[4]) == 9
    f = CS.frame_for(c1, 45, 30)
    images, pitch, counts = CS.emu_run([f], [c1])
    assert counts["tiles"] == 9
    BS.check_images(images, pitch, [f], [nine.expected(c1, 45, 30)], "nine sources")
    # a second target of the same terminal size on the same sources (a descriptor of its own): the same nine tiles
    c2 = CS.Composite.from_buffer_copy(bytes(c1))
    f2 = CS.frame_for(c2, 30, 20, BS.FLIP_X)
    images, pitch, counts = CS.emu_run([f, f2], [c1, c2])
    assert counts["tiles"] == 9
    BS.check_images(images, pitch, [f, f2], [nine.expected(c1, 45, 30), nine.expected(c1, 30, 20, BS.FLIP_X)], "two targets")
    # a target of another terminal size has tiles of its own
    c3 = CS.setup([s.src for s in list(c1.s)], [(64, 36)] * 9, 60, 20)
    _, _, counts = CS.emu_run([f, CS.frame_for(c3, 60, 40)], [c1, c3])
    assert counts["tiles"] == 18


def test_library_refuses_before_it_needs_a_device_and_needs_one_after():
    L = CS.lib()
    NO_DEVICE, NOT_SUPPORTED, INVALID = 200, 30, 86
    sc = SCENES["four slots, one empty, on 60x20"]
    comp, _keep = sc.build()
    img = BS.noise(8, 4, 1)
    plain = BS.frame_for(img.ctypes.data, 8, 4, 2, 2)
    h = C.c_void_p()

    def call(frames, comps):
        rc = L.asciichat_hip_box_composites(C.byref(h), (BS.Frame * len(frames))(*frames), CS.comp_array(comps), len(frames), None)
        if rc != 0:
            assert not h.value
        return rc

    def comp_with(src=None, **kw):
        c = CS.Composite.from_buffer_copy(bytes(comp))
        for k, v in kw.items():
            setattr(c, k, v)
        for k, v in (src or {}).items():
            setattr(c.s[2], k, v)
        return c

    def frame_with(**kw):
        f = CS.frame_for(comp, 60, 20)
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    good = frame_with()
    L.asciichat_hip_last_error.restype = C.c_char_p
    for f in (frame_with(src_w=59), frame_with(src_h=41), frame_with(out_w=0), frame_with(out_h=-1), frame_with(out_w=16385),
              frame_with(out_h=16385)):
        assert call([plain, f], [None, comp]) == INVALID
        assert b"frame 1" in L.asciichat_hip_last_error()
    bad = [comp_with(canvas_w=0), comp_with(canvas_h=0), comp_with(canvas_w=3841), comp_with(canvas_h=2161), comp_with(n_src=-1),
           comp_with(n_src=10), comp_with(cols=-1), comp_with(rows=-2),
           comp_with(src=dict(src_w=0)), comp_with(src=dict(src_h=-4)), comp_with(src=dict(src_w=3841, src_stride=3 * 3841)),
           comp_with(src=dict(src_h=2161)), comp_with(src=dict(src_stride=3 * 40 - 1)), comp_with(src=dict(src_stride=0)),
           comp_with(src=dict(tile_w=0)), comp_with(src=dict(tile_h=0)), comp_with(src=dict(tile_w=61)),
           comp_with(src=dict(tile_h=41))]
    for c in bad:
        f = CS.frame_for(c, 60, 20) if 0 < c.canvas_w <= 3840 and 0 < c.canvas_h <= 2160 else good
        assert call([plain, f], [None, c]) == INVALID, CS.geometry(c)
        assert b"frame 1" in L.asciichat_hip_last_error()
    # a plain frame of the batch keeps box_create's rules
    with_comp = BS.frame_for(img.ctypes.data, 8, 4, 2, 2)
    with_comp.comp = img.ctypes.data
    assert call([good, with_comp], [comp, None]) == NOT_SUPPORTED
    no_src = BS.frame_for(None, 8, 4, 2, 2)
    assert call([good, no_src], [comp, None]) == INVALID
    # bad arguments
    arr, cp = (BS.Frame * 1)(good), CS.comp_array([comp])
    assert L.asciichat_hip_box_composites(None, arr, cp, 1, None) == INVALID
    assert L.asciichat_hip_box_composites(C.byref(h), None, cp, 1, None) == INVALID
    assert L.asciichat_hip_box_composites(C.byref(h), arr, None, 1, None) == INVALID
    assert L.asciichat_hip_box_composites(C.byref(h), arr, cp, 0, None) == INVALID
    # valid and all black: cell sizes of 0, no sources -- and valid batches need a device
    black = [comp_with(cell_h=0), comp_with(cell_w=-1), comp_with(n_src=0)]
    if L.asciichat_hip_device_count() == 0:
        for c in black + [comp]:
            assert call([plain, good], [None, c]) == NO_DEVICE
