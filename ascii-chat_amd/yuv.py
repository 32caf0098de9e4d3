"""ctypes binding of libasciichat_yuv.so (include/asciichat_yuv.h): camera and decoder frames -- I420, NV12, YUYV, UYVY -- to the
RGB24 the renderers read, on the device: only the pixels a render samples (Yuv.run), or whole frames (Yuv.run_whole, yuv_convert)."""
import ctypes as C
import os

__all__ = ["Yuv", "YuvSource", "yuv_source", "yuv_convert", "yuv_lib", "YUV_LIB_PATH", "YUV_I420", "YUV_NV12", "YUV_YUYV", "YUV_UYVY"]

HERE = os.path.dirname(os.path.abspath(__file__))
YUV_LIB_PATH = os.path.join(HERE, "libasciichat_yuv.so")

YUV_I420, YUV_NV12, YUV_YUYV, YUV_UYVY = 0, 1, 2, 3


class YuvSource(C.Structure):  # asciichat_yuv_source_t
    _fields_ = [("plane", C.c_void_p * 3), ("stride", C.c_int32 * 3), ("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


def yuv_source(fmt, width, height, planes, strides=(0, 0, 0)):
    """-> a YuvSource; planes: up to three device addresses (None: absent), strides: bytes per plane row, 0 = tight"""
    s = YuvSource()
    s.format, s.width, s.height = fmt, width, height
    for k in range(3):
        s.plane[k] = planes[k] if k < len(planes) else None
        s.stride[k] = strides[k] if k < len(strides) else 0
    return s


_lib = None


def yuv_lib():
    """Load libasciichat_yuv.so (never a substitute: raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        import torch  # noqa: F401  (its libamdhip64 first, as binding.lib() does)
    except ImportError:
        pass
    if not os.path.exists(YUV_LIB_PATH):
        raise RuntimeError(f"{YUV_LIB_PATH} is missing: run __graft_entry__.build() (hipcc, gfx950) first")
    L = C.CDLL(YUV_LIB_PATH)
    vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
    for name, res, args in (("asciichat_yuv_device_count", ci, []),
                            ("asciichat_yuv_last_error", C.c_char_p, []),
                            ("asciichat_yuv_convert", ci, [C.POINTER(YuvSource), vp, ci, vp]),
                            ("asciichat_yuv_create", ci, [C.POINTER(vp), ci]),
                            ("asciichat_yuv_set", ci, [vp, vp, vp, ci, vp]),
                            ("asciichat_yuv_image_pitch", sz, [vp]),
                            ("asciichat_yuv_run", ci, [vp, vp, sz, vp]),
                            ("asciichat_yuv_render_frames", ci, [vp, vp, sz, vp]),
                            ("asciichat_yuv_whole_pitch", sz, [vp]),
                            ("asciichat_yuv_run_whole", ci, [vp, vp, sz, vp]),
                            ("asciichat_yuv_destroy", None, [vp])):
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _last_error(L):
    return L.asciichat_yuv_last_error().decode("utf-8", "replace")


def yuv_convert(source, rgb_ptr, rgb_stride=0, stream=0):
    """one source, whole: RGB24 row y at rgb_ptr + y * rgb_stride (0: tight), any alignment; asynchronous"""
    L = yuv_lib()
    rc = L.asciichat_yuv_convert(C.byref(source), rgb_ptr, rgb_stride, stream)
    if rc != 0:
        raise RuntimeError(f"asciichat_yuv_convert failed ({rc}): {_last_error(L)}")


class Yuv:
    """A handle for up to max_frames YUV sources per tick (asciichat_yuv_*): set() takes the tick's sources and, with them, the
    descriptors frame_setup made; run() leaves the image each descriptor samples, render_frames() the descriptors a Plan renders
    those images with; run_whole() converts every source entirely."""

    def __init__(self, max_frames):
        self.L = yuv_lib()
        self._h = C.c_void_p()
        rc = self.L.asciichat_yuv_create(C.byref(self._h), max_frames)
        if rc != 0:
            raise RuntimeError(f"asciichat_yuv_create failed ({rc}): {self.last_error()}")
        self.n = 0

    def last_error(self):
        return _last_error(self.L)

    def set(self, sources, frames=None, stream=0):
        """sources: a list (or ctypes array) of YuvSource; frames: as many binding.Frame, or None (run_whole only).  Checked on
        the host, copied asynchronously on `stream` (the handle's one stream)"""
        from .binding import Frame
        n = len(sources)
        src = sources if isinstance(sources, C.Array) else (YuvSource * max(1, n))(*sources)
        arr = None
        if frames is not None:
            if len(frames) != n:
                raise ValueError("as many descriptors as sources")
            arr = frames if isinstance(frames, C.Array) else (Frame * max(1, n))(*frames)
        rc = self.L.asciichat_yuv_set(self._h, C.cast(src, C.c_void_p), C.cast(arr, C.c_void_p) if arr is not None else None, n, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_yuv_set failed ({rc}): {self.last_error()}")
        self.n = n

    @property
    def pitch(self):
        return int(self.L.asciichat_yuv_image_pitch(self._h))

    @property
    def whole_pitch(self):
        return int(self.L.asciichat_yuv_whole_pitch(self._h))

    def run(self, images_ptr, pitch=None, stream=0):
        """frame i's sampled image (out_w x out_h RGB24, rows tight) at images_ptr + i * pitch; asynchronous"""
        rc = self.L.asciichat_yuv_run(self._h, images_ptr, self.pitch if pitch is None else pitch, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_yuv_run failed ({rc}): {self.last_error()}")

    def render_frames(self, images_ptr, pitch=None):
        """-> the set's descriptors rewritten onto the images (a ctypes array of binding.Frame): what a Plan is created with"""
        from .binding import Frame
        out = (Frame * max(1, self.n))()
        rc = self.L.asciichat_yuv_render_frames(self._h, images_ptr, self.pitch if pitch is None else pitch, C.cast(out, C.c_void_p))
        if rc != 0:
            raise RuntimeError(f"asciichat_yuv_render_frames failed ({rc}): {self.last_error()}")
        return [out[i] for i in range(self.n)]

    def run_whole(self, rgb_ptr, pitch=None, stream=0):
        """source i whole (3 * width * height bytes, rows tight) at rgb_ptr + i * pitch; asynchronous"""
        rc = self.L.asciichat_yuv_run_whole(self._h, rgb_ptr, self.whole_pitch if pitch is None else pitch, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_yuv_run_whole failed ({rc}): {self.last_error()}")

    def close(self):
        if self._h:
            self.L.asciichat_yuv_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
