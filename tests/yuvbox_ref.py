"""The rule of include/asciichat_yuvbox.h as the composition of the two restatements already in the tree, independent of the
code under test: the box average (tests/box_ref.py) of the whole conversion (tests/yuv_ref.py).  No arithmetic of its own.
TESTS ONLY."""
import box_ref
import yuv_ref


def image(src, out_w, out_h, flip_x=False, flip_y=False):
    """src: a yuv_ref.Source -> the (out_h, out_w, 3) uint8 image the pass must leave"""
    return box_ref.box_ref(yuv_ref.convert_whole(src), out_w, out_h, flip_x, flip_y)
