"""The rasteriser's YUV 4:2:0 output restated in Python (asciichat_raster.h): the reference's h265_encoder_ascii_to_yuv420 over
the image raster_ref.render returns.  Line numbers are those of the reference's lib/video/h265/encoder.c.  TESTS ONLY."""
import numpy as np

I420, NV12 = 1, 2


def luma(r, g, b):
    """:264 -- int64 arrays or ints"""
    return ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16


def chroma(r, g, b):
    """:281 and :285 over a block's averages, with the clamps of :282 and :286 (numpy's >> of a negative int64 is arithmetic, as
    C's is here) -> (U, V)"""
    u = ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128          # :281
    v = ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128           # :285
    return np.clip(u, 0, 255), np.clip(v, 0, 255)                # :282, :286


def block_average(c):
    """:276-278 -- one channel (H, W), even both: (p00 + p10 + p01 + p11) / 4, truncating"""
    return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]) // 4


def yuv420(img_rgba, layout):
    """(H, W, 4) uint8, H and W even -> the W * H * 3 / 2 bytes of one image; alpha plays no part"""
    H, W = img_rgba.shape[:2]
    assert H % 2 == 0 and W % 2 == 0 and H >= 2 and W >= 2  # (the reference reads past an odd image, :268-274: not restated)
    rgb = img_rgba[:, :, :3].astype(np.int64)
    r, g, b = rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2]           # :259-261
    y = luma(r, g, b).astype(np.uint8)                            # :264, the (uint8_t) cast
    u, v = chroma(block_average(r), block_average(g), block_average(b))
    u, v = u.astype(np.uint8), v.astype(np.uint8)
    if layout == I420:                                            # :248-250: Y, then U, then V, rows tight
        return np.concatenate([y.ravel(), u.ravel(), v.ravel()])
    assert layout == NV12
    return np.concatenate([y.ravel(), np.stack([u, v], axis=-1).ravel()])  # U, V interleaved
