"""ctypes binding of libasciichat_pix.so (include/asciichat_pix.h): packed RGB camera frames -- RGB24, RGBA, BGR24, BGRA -- to the
RGB24 the renderers read, on the device: only the pixels a render samples (Pix.run), whole frames (Pix.run_whole, pix_convert),
or the box average straight from the source (Pix.run_box, pix_downscale)."""
import ctypes as C
import os

__all__ = ["Pix", "PixSource", "pix_source", "pix_convert", "pix_downscale", "pix_lib", "PIX_LIB_PATH", "PIX_RGB", "PIX_RGBA", "PIX_BGR", "PIX_BGRA"]

HERE = os.path.dirname(os.path.abspath(__file__))
PIX_LIB_PATH = os.path.join(HERE, "libasciichat_pix.so")

PIX_RGB, PIX_RGBA, PIX_BGR, PIX_BGRA = 0, 1, 2, 3


class PixSource(C.Structure):  # asciichat_pix_source_t
    _fields_ = [("pixels", C.c_void_p), ("stride", C.c_int32), ("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


def pix_source(fmt, width, height, pixels, stride=0):
    """-> a PixSource; pixels: a device address, stride: bytes per row, 0 = tight"""
    s = PixSource()
    s.format, s.width, s.height, s.pixels, s.stride = fmt, width, height, pixels, stride
    return s


_lib = None


def pix_lib():
    """Load libasciichat_pix.so (never a substitute: raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        import torch  # noqa: F401  (its libamdhip64 first, as binding.lib() does)
    except ImportError:
        pass
    if not os.path.exists(PIX_LIB_PATH):
        raise RuntimeError(f"{PIX_LIB_PATH} is missing: run __graft_entry__.build() (hipcc, gfx950) first")
    L = C.CDLL(PIX_LIB_PATH)
    vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
    for name, res, args in (("asciichat_pix_device_count", ci, []),
                            ("asciichat_pix_last_error", C.c_char_p, []),
                            ("asciichat_pix_convert", ci, [C.POINTER(PixSource), vp, ci, vp]),
                            ("asciichat_pix_downscale", ci, [C.POINTER(PixSource), vp, ci, ci, ci, ci, vp]),
                            ("asciichat_pix_create", ci, [C.POINTER(vp), ci]),
                            ("asciichat_pix_set", ci, [vp, vp, vp, ci, vp]),
                            ("asciichat_pix_image_pitch", sz, [vp]),
                            ("asciichat_pix_run", ci, [vp, vp, sz, vp]),
                            ("asciichat_pix_run_box", ci, [vp, vp, sz, vp]),
                            ("asciichat_pix_render_frames", ci, [vp, vp, sz, vp]),
                            ("asciichat_pix_whole_pitch", sz, [vp]),
                            ("asciichat_pix_run_whole", ci, [vp, vp, sz, vp]),
                            ("asciichat_pix_destroy", None, [vp])):
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _last_error(L):
    return L.asciichat_pix_last_error().decode("utf-8", "replace")


def pix_convert(source, rgb_ptr, rgb_stride=0, stream=0):
    """one source, whole: RGB24 row y at rgb_ptr + y * rgb_stride (0: tight), any alignment; asynchronous"""
    L = pix_lib()
    rc = L.asciichat_pix_convert(C.byref(source), rgb_ptr, rgb_stride, stream)
    if rc != 0:
        raise RuntimeError(f"asciichat_pix_convert failed ({rc}): {_last_error(L)}")


def pix_downscale(source, dst_ptr, dst_w, dst_h, flip_x=False, flip_y=False, stream=0):
    """one source averaged to dst_w x dst_h (3 * dst_w * dst_h bytes at dst_ptr, rows tight, any alignment); asynchronous"""
    L = pix_lib()
    rc = L.asciichat_pix_downscale(C.byref(source), dst_ptr, dst_w, dst_h, int(flip_x), int(flip_y), stream)
    if rc != 0:
        raise RuntimeError(f"asciichat_pix_downscale failed ({rc}): {_last_error(L)}")


class Pix:
    """A handle for up to max_frames packed RGB sources per tick (asciichat_pix_*): set() takes the tick's sources and, with them,
    the descriptors frame_setup made; run() leaves the image each descriptor samples, run_box() each source averaged to its
    descriptor's out_w x out_h, render_frames() the descriptors a Plan renders either's images with; run_whole() converts every
    source entirely."""

    def __init__(self, max_frames):
        self.L = pix_lib()
        self._h = C.c_void_p()
        rc = self.L.asciichat_pix_create(C.byref(self._h), max_frames)
        if rc != 0:
            raise RuntimeError(f"asciichat_pix_create failed ({rc}): {self.last_error()}")
        self.n = 0

    def last_error(self):
        return _last_error(self.L)

    def set(self, sources, frames=None, stream=0):
        """sources: a list (or ctypes array) of PixSource; frames: as many binding.Frame, or None (run_whole only).  Checked on
        the host, copied asynchronously on `stream` (the handle's one stream)"""
        from .binding import Frame
        n = len(sources)
        src = sources if isinstance(sources, C.Array) else (PixSource * max(1, n))(*sources)
        arr = None
        if frames is not None:
            if len(frames) != n:
                raise ValueError("as many descriptors as sources")
            arr = frames if isinstance(frames, C.Array) else (Frame * max(1, n))(*frames)
        rc = self.L.asciichat_pix_set(self._h, C.cast(src, C.c_void_p), C.cast(arr, C.c_void_p) if arr is not None else None, n, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_pix_set failed ({rc}): {self.last_error()}")
        self.n = n

    @property
    def pitch(self):
        return int(self.L.asciichat_pix_image_pitch(self._h))

    @property
    def whole_pitch(self):
        return int(self.L.asciichat_pix_whole_pitch(self._h))

    def run(self, images_ptr, pitch=None, stream=0):
        """frame i's sampled image (out_w x out_h RGB24, rows tight) at images_ptr + i * pitch; one launch; asynchronous"""
        rc = self.L.asciichat_pix_run(self._h, images_ptr, self.pitch if pitch is None else pitch, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_pix_run failed ({rc}): {self.last_error()}")

    def run_box(self, images_ptr, pitch=None, stream=0):
        """source i's averaged image (out_w x out_h RGB24, rows tight) at images_ptr + i * pitch; one launch; asynchronous"""
        rc = self.L.asciichat_pix_run_box(self._h, images_ptr, self.pitch if pitch is None else pitch, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_pix_run_box failed ({rc}): {self.last_error()}")

    def render_frames(self, images_ptr, pitch=None):
        """-> the set's descriptors rewritten onto the images (a list of binding.Frame): what a Plan is created with"""
        from .binding import Frame
        out = (Frame * max(1, self.n))()
        rc = self.L.asciichat_pix_render_frames(self._h, images_ptr, self.pitch if pitch is None else pitch, C.cast(out, C.c_void_p))
        if rc != 0:
            raise RuntimeError(f"asciichat_pix_render_frames failed ({rc}): {self.last_error()}")
        return [out[i] for i in range(self.n)]

    def run_whole(self, rgb_ptr, pitch=None, stream=0):
        """source i whole (3 * width * height bytes, rows tight) at rgb_ptr + i * pitch; asynchronous"""
        rc = self.L.asciichat_pix_run_whole(self._h, rgb_ptr, self.whole_pitch if pitch is None else pitch, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_pix_run_whole failed ({rc}): {self.last_error()}")

    def close(self):
        if self._h:
            self.L.asciichat_pix_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
