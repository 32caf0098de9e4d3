"""ctypes binding of libasciichat_yuvbox.so (include/asciichat_yuvbox.h): camera and decoder frames -- I420, NV12, YUYV, UYVY --
box-averaged to the size a render target samples, straight from their planes, on the device: what Yuv.run_whole followed by
Box.run leaves, byte for byte, without the whole RGB24 frames between them (YuvBox.run), or one source (yuvbox_downscale)."""
import ctypes as C
import os

from .yuv import YuvSource

__all__ = ["YuvBox", "yuvbox_downscale", "yuvbox_lib", "YUVBOX_LIB_PATH"]

HERE = os.path.dirname(os.path.abspath(__file__))
YUVBOX_LIB_PATH = os.path.join(HERE, "libasciichat_yuvbox.so")

_lib = None


def yuvbox_lib():
    """Load libasciichat_yuvbox.so (never a substitute: raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        import torch  # noqa: F401  (its libamdhip64 first, as binding.lib() does)
    except ImportError:
        pass
    if not os.path.exists(YUVBOX_LIB_PATH):
        raise RuntimeError(f"{YUVBOX_LIB_PATH} is missing: run __graft_entry__.build() (hipcc, gfx950) first")
    L = C.CDLL(YUVBOX_LIB_PATH)
    vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
    for name, res, args in (("asciichat_yuvbox_device_count", ci, []),
                            ("asciichat_yuvbox_last_error", C.c_char_p, []),
                            ("asciichat_yuvbox_create", ci, [C.POINTER(vp), ci]),
                            ("asciichat_yuvbox_set", ci, [vp, vp, vp, ci, vp]),
                            ("asciichat_yuvbox_image_pitch", sz, [vp]),
                            ("asciichat_yuvbox_run", ci, [vp, vp, sz, vp]),
                            ("asciichat_yuvbox_render_frames", ci, [vp, vp, sz, vp]),
                            ("asciichat_yuvbox_downscale", ci, [C.POINTER(YuvSource), vp, ci, ci, ci, ci, vp]),
                            ("asciichat_yuvbox_destroy", None, [vp])):
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _last_error(L):
    return L.asciichat_yuvbox_last_error().decode("utf-8", "replace")


def yuvbox_downscale(source, dst_ptr, dst_w, dst_h, flip_x=False, flip_y=False, stream=0):
    """one source averaged to dst_w x dst_h (3 * dst_w * dst_h bytes at dst_ptr, rows tight, any alignment); asynchronous"""
    L = yuvbox_lib()
    rc = L.asciichat_yuvbox_downscale(C.byref(source), dst_ptr, dst_w, dst_h, int(flip_x), int(flip_y), stream)
    if rc != 0:
        raise RuntimeError(f"asciichat_yuvbox_downscale failed ({rc}): {_last_error(L)}")


class YuvBox:
    """A handle for up to max_frames YUV sources per tick (asciichat_yuvbox_*): set() takes the tick's sources and the
    descriptors frame_setup made for them; run() leaves each source averaged to its descriptor's out_w x out_h,
    render_frames() the descriptors a Plan renders those images with."""

    def __init__(self, max_frames):
        self.L = yuvbox_lib()
        self._h = C.c_void_p()
        rc = self.L.asciichat_yuvbox_create(C.byref(self._h), max_frames)
        if rc != 0:
            raise RuntimeError(f"asciichat_yuvbox_create failed ({rc}): {self.last_error()}")
        self.n = 0

    def last_error(self):
        return _last_error(self.L)

    def set(self, sources, frames, stream=0):
        """sources: a list (or ctypes array) of YuvSource; frames: as many binding.Frame.  Checked on the host, copied
        asynchronously on `stream` (the handle's one stream)"""
        from .binding import Frame
        n = len(sources)
        if frames is None or len(frames) != n:
            raise ValueError("as many descriptors as sources")
        src = sources if isinstance(sources, C.Array) else (YuvSource * max(1, n))(*sources)
        arr = frames if isinstance(frames, C.Array) else (Frame * max(1, n))(*frames)
        rc = self.L.asciichat_yuvbox_set(self._h, C.cast(src, C.c_void_p), C.cast(arr, C.c_void_p), n, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_yuvbox_set failed ({rc}): {self.last_error()}")
        self.n = n

    @property
    def pitch(self):
        return int(self.L.asciichat_yuvbox_image_pitch(self._h))

    def run(self, images_ptr, pitch=None, stream=0):
        """source i's averaged image (out_w x out_h RGB24, rows tight) at images_ptr + i * pitch; one launch; asynchronous"""
        rc = self.L.asciichat_yuvbox_run(self._h, images_ptr, self.pitch if pitch is None else pitch, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_yuvbox_run failed ({rc}): {self.last_error()}")

    def render_frames(self, images_ptr, pitch=None):
        """-> the set's descriptors rewritten onto the images (a list of binding.Frame): what a Plan is created with"""
        from .binding import Frame
        out = (Frame * max(1, self.n))()
        rc = self.L.asciichat_yuvbox_render_frames(self._h, images_ptr, self.pitch if pitch is None else pitch, C.cast(out, C.c_void_p))
        if rc != 0:
            raise RuntimeError(f"asciichat_yuvbox_render_frames failed ({rc}): {self.last_error()}")
        return [out[i] for i in range(self.n)]

    def close(self):
        if self._h:
            self.L.asciichat_yuvbox_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
