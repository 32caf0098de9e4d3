"""NumPy restatement of the YUV sources' rule and of the four layouts (include/asciichat_yuv.h states both), independent of
yuv_math.h: what the kernels of libasciichat_yuv.so must give.  The arithmetic and the I420 and UYVY layouts are the reference's
convert_pixel_buffer_to_rgb24 (lib/video/webcam/macos/webcam_avfoundation.m:406-472: UYVY bytes :413-416, I420 addressing
:457-459, the sums :419-421 / :461-463, the clamps :423-425 / :465-467); NV12 and YUYV are the same arithmetic over the other
two layouts the reference's Linux capture negotiates (lib/video/webcam/linux/webcam_v4l2.c:198-306).  TESTS ONLY."""
import numpy as np

I420, NV12, YUYV, UYVY = 0, 1, 2, 3
NAMES = {I420: "I420", NV12: "NV12", YUYV: "YUYV", UYVY: "UYVY"}
PACKED = (YUYV, UYVY)
FLIP_X, FLIP_Y = 1, 2

# the hand known answers: (Y, U, V) -> (R, G, B)
KNOWN = {(16, 128, 128): (0, 0, 0), (235, 128, 128): (255, 255, 255), (81, 90, 240): (255, 0, 0), (0, 0, 0): (0, 135, 0),
         (255, 255, 255): (255, 125, 255)}


def rule(Y, U, V):
    """arrays (or scalars) of samples -> uint8 array [..., 3] of R, G, B"""
    y = np.asarray(Y, dtype=np.int32) - 16
    u = np.asarray(U, dtype=np.int32) - 128
    v = np.asarray(V, dtype=np.int32) - 128
    r = (298 * y + 409 * v + 128) >> 8  # numpy's >> of a negative int32 is arithmetic, as the reference's is
    g = (298 * y - 100 * u - 208 * v + 128) >> 8
    b = (298 * y + 516 * u + 128) >> 8
    return np.clip(np.stack(np.broadcast_arrays(r, g, b), axis=-1), 0, 255).astype(np.uint8)


def chroma_size(w, h):
    return (w + 1) // 2, (h + 1) // 2


def planes_of(fmt):
    return 3 if fmt == I420 else 2 if fmt == NV12 else 1


def row_bytes(fmt, k, w):
    """the bytes of a row of plane k: the tight stride"""
    if fmt in PACKED:
        return 2 * w
    cw = chroma_size(w, 1)[0]
    return w if k == 0 else 2 * cw if fmt == NV12 else cw


def plane_rows(fmt, k, h):
    return h if k == 0 or fmt in PACKED else chroma_size(1, h)[1]


class Source:
    """format, width, height, planes: 1-D uint8 arrays (a plane starts at its element 0), strides: bytes per row, none 0"""

    def __init__(self, fmt, width, height, planes, strides):
        self.format, self.width, self.height, self.planes, self.strides = fmt, width, height, list(planes), list(strides)


def samples(src, sx, sy):
    """the (Y, U, V) of pixels (sx, sy): integer arrays of one shape"""
    sx, sy = np.asarray(sx, dtype=np.int64), np.asarray(sy, dtype=np.int64)
    P, s, f = src.planes, src.strides, src.format
    if f == I420:
        return P[0][sy * s[0] + sx], P[1][(sy // 2) * s[1] + sx // 2], P[2][(sy // 2) * s[2] + sx // 2]
    if f == NV12:
        at = (sy // 2) * s[1] + 2 * (sx // 2)
        return P[0][sy * s[0] + sx], P[1][at], P[1][at + 1]
    pair = sy * s[0] + 4 * (sx // 2)
    if f == UYVY:
        return P[0][pair + 1 + 2 * (sx & 1)], P[0][pair], P[0][pair + 2]
    assert f == YUYV
    return P[0][pair + 2 * (sx & 1)], P[0][pair + 1], P[0][pair + 3]


def convert_whole(src):
    """-> the RGB image [height, width, 3]"""
    sy, sx = np.mgrid[0:src.height, 0:src.width]
    return np.ascontiguousarray(rule(*samples(src, sx, sy)))


def sample(src, frame):
    """-> the image [out_h, out_w, 3] a descriptor (out_w, out_h, x_ratio, y_ratio, ops; achip_types.h's rule) samples"""
    assert (frame.src_w, frame.src_h) == (src.width, src.height)
    x = np.arange(frame.out_w, dtype=np.uint64)
    y = np.arange(frame.out_h, dtype=np.uint64)
    assert (frame.out_w - 1) * frame.x_ratio < 1 << 32 and (frame.out_h - 1) * frame.y_ratio < 1 << 32
    sx = np.minimum((x * np.uint64(frame.x_ratio)) >> np.uint64(16), np.uint64(src.width - 1)).astype(np.int64)
    sy = np.minimum((y * np.uint64(frame.y_ratio)) >> np.uint64(16), np.uint64(src.height - 1)).astype(np.int64)
    if frame.ops & FLIP_X:
        sx = src.width - 1 - sx
    if frame.ops & FLIP_Y:
        sy = src.height - 1 - sy
    return np.ascontiguousarray(rule(*samples(src, sx[None, :], sy[:, None])))


def pack(fmt, Y, U, V, strides=(0, 0, 0), fill=None):
    """The planes of a source from full sample arrays: Y [h, w]; U, V [ch, cw] (4:2:0) or [h, w / 2] (packed).  strides: bytes
    per row, 0 = tight; the bytes of a row behind its samples come from fill (a generator, or zeros).  -> (planes, strides)"""
    h, w = Y.shape
    strides = [strides[k] or row_bytes(fmt, k, w) for k in range(planes_of(fmt))]
    rows = []
    if fmt == I420:
        rows = [Y, U, V]
    elif fmt == NV12:
        rows = [Y, np.stack([U, V], axis=-1).reshape(U.shape[0], -1)]
    else:
        a, b = Y[:, 0::2], Y[:, 1::2]
        rows = [np.stack([U, a, V, b] if fmt == UYVY else [a, U, b, V], axis=-1).reshape(h, -1)]
    planes = []
    for k, body in enumerate(rows):
        assert body.shape == (plane_rows(fmt, k, h), row_bytes(fmt, k, w)) and strides[k] >= body.shape[1]
        full = np.zeros((body.shape[0], strides[k]), dtype=np.uint8) if fill is None else fill.integers(0, 256, (body.shape[0], strides[k]), dtype=np.uint8)
        full[:, :body.shape[1]] = body
        planes.append(full.reshape(-1)[:(body.shape[0] - 1) * strides[k] + body.shape[1]].copy())  # exactly what may be read
    return planes, strides
