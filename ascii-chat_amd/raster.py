"""ctypes binding of libasciichat_raster.so (include/asciichat_raster.h): rendered ANSI frames -- or the source images behind
them, without the text -- to RGBA pixels, or straight to YUV 4:2:0 planes, on the device."""
import ctypes as C
import os

__all__ = ["Raster", "RasterFont", "RasterGlyph", "raster_font", "raster_lib", "RASTER_LIB_PATH", "RASTER_NO_FRAME", "RASTER_BAD_UTF8",
           "RASTER_UNKNOWN", "RASTER_OVERFLOW_COLS", "RASTER_OVERFLOW_ROWS", "RASTER_INDEXED_FLAT", "RASTER_INDEXED_XTERM", "RASTER_YUV_I420",
           "RASTER_YUV_NV12"]

HERE = os.path.dirname(os.path.abspath(__file__))
RASTER_LIB_PATH = os.path.join(HERE, "libasciichat_raster.so")

RASTER_NO_FRAME, RASTER_BAD_UTF8, RASTER_UNKNOWN, RASTER_OVERFLOW_COLS, RASTER_OVERFLOW_ROWS = 1, 2, 4, 8, 16
RASTER_INDEXED_FLAT, RASTER_INDEXED_XTERM = 1, 2
RASTER_YUV_I420, RASTER_YUV_NV12 = 1, 2  # Y, U, V planes | Y plane, then U V pairs


class RasterGlyph(C.Structure):  # asciichat_raster_glyph_t
    _fields_ = [("codepoint", C.c_uint32), ("left", C.c_int16), ("top", C.c_int16), ("width", C.c_uint16), ("rows", C.c_uint16),
                ("pitch", C.c_uint32), ("offset", C.c_uint32)]


class RasterFont(C.Structure):  # asciichat_raster_font_t
    _fields_ = [("cell_w", C.c_int32), ("cell_h", C.c_int32), ("baseline", C.c_int32), ("n_glyphs", C.c_int32),
                ("glyphs", C.POINTER(RasterGlyph)), ("coverage", C.c_void_p), ("coverage_bytes", C.c_size_t),
                ("default_fg", C.c_uint32), ("default_bg", C.c_uint32), ("indexed", C.c_int32), ("flat_fg", C.c_uint32),
                ("flat_bg", C.c_uint32), ("matrix_map", C.c_int32)]


_lib = None


def raster_lib():
    """Load libasciichat_raster.so (never a substitute: raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        import torch  # noqa: F401  (its libamdhip64 first, as binding.lib() does)
    except ImportError:
        pass
    if not os.path.exists(RASTER_LIB_PATH):
        raise RuntimeError(f"{RASTER_LIB_PATH} is missing: run __graft_entry__.build() (hipcc, gfx950) first")
    L = C.CDLL(RASTER_LIB_PATH)
    vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
    for name, res, args in (("asciichat_raster_device_count", ci, []),
                            ("asciichat_raster_last_error", C.c_char_p, []),
                            ("asciichat_raster_create", ci, [C.POINTER(vp), C.POINTER(RasterFont), ci, ci, ci]),
                            ("asciichat_raster_width_px", ci, [vp]),
                            ("asciichat_raster_height_px", ci, [vp]),
                            ("asciichat_raster_image_pitch", sz, [vp]),
                            ("asciichat_raster_run", ci, [vp, vp, sz, vp, ci, vp, sz, vp, vp]),
                            ("asciichat_raster_parse", ci, [vp, vp, sz, vp, ci, vp, vp]),
                            ("asciichat_raster_draw", ci, [vp, ci, vp, sz, vp]),
                            ("asciichat_raster_yuv420_bytes", sz, [ci, ci]),
                            ("asciichat_raster_yuv420_pitch", sz, [vp]),
                            ("asciichat_raster_run_yuv420", ci, [vp, vp, sz, vp, ci, vp, sz, ci, vp, vp]),
                            ("asciichat_raster_draw_yuv420", ci, [vp, ci, vp, sz, ci, vp]),
                            ("asciichat_raster_images_set", ci, [vp, ci, C.c_char_p, vp, ci, vp]),
                            ("asciichat_raster_images_set_composites", ci, [vp, ci, C.c_char_p, vp, ci, vp]),
                            ("asciichat_raster_images_set_dithered", ci, [vp, C.c_char_p, vp, ci, vp]),
                            ("asciichat_raster_cells_from_images", ci, [vp, ci, vp, vp]),
                            ("asciichat_raster_run_images", ci, [vp, ci, vp, sz, vp, vp]),
                            ("asciichat_raster_run_images_yuv420", ci, [vp, ci, vp, sz, ci, vp, vp]),
                            ("asciichat_raster_destroy", None, [vp])):
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def raster_font(cell_w, cell_h, baseline, glyphs, coverage, default_fg=0xCCCCCC, default_bg=0, indexed=RASTER_INDEXED_FLAT,
                flat_fg=0xCCCCCC, flat_bg=0, matrix_map=False):
    """-> a RasterFont (it keeps its arrays alive).  glyphs: (codepoint, left, top, width, rows, pitch, offset) tuples in ascending
    codepoint order; coverage: bytes-like, 8-bit alpha."""
    f = RasterFont()
    f._glyphs = (RasterGlyph * max(1, len(glyphs)))(*[RasterGlyph(*g) for g in glyphs])
    cov = bytes(coverage)
    f._coverage = (C.c_uint8 * max(1, len(cov))).from_buffer_copy(cov or b"\0")
    f.cell_w, f.cell_h, f.baseline, f.n_glyphs = cell_w, cell_h, baseline, len(glyphs)
    f.glyphs = f._glyphs
    f.coverage, f.coverage_bytes = C.addressof(f._coverage), len(cov)
    f.default_fg, f.default_bg, f.indexed, f.flat_fg, f.flat_bg, f.matrix_map = (default_fg, default_bg, indexed, flat_fg, flat_bg,
                                                                                  int(bool(matrix_map)))
    return f


class Raster:
    """A rasteriser of cols x rows cell frames (asciichat_raster_*): run() turns the frames a Plan.render left in device memory
    into RGBA images, one font-cell rectangle per character; run_yuv420() into YUV 4:2:0 planes for an encoder instead.  Not a
    parity path where DESIGN.md 7 says so."""

    def __init__(self, font, cols, rows, max_frames):
        self.L = raster_lib()
        self._font = font
        self._h = C.c_void_p()
        rc = self.L.asciichat_raster_create(C.byref(self._h), C.byref(font), cols, rows, max_frames)
        if rc != 0:
            raise RuntimeError(f"asciichat_raster_create failed ({rc}): {self.last_error()}")
        self.width = self.L.asciichat_raster_width_px(self._h)
        self.height = self.L.asciichat_raster_height_px(self._h)
        self.pitch = int(self.L.asciichat_raster_image_pitch(self._h))
        self.yuv_pitch = int(self.L.asciichat_raster_yuv420_pitch(self._h))  # width * height * 3 / 2; 0 when either is odd

    def last_error(self):
        return self.L.asciichat_raster_last_error().decode("utf-8", "replace")

    def run(self, frames_ptr, frame_stride, len_ptr, n, pixels_ptr, status_ptr, image_pitch=None, stream=0):
        """frame i at frames_ptr + i * frame_stride, len_ptr[i] bytes -> image i at pixels_ptr + i * image_pitch; asynchronous"""
        rc = self.L.asciichat_raster_run(self._h, frames_ptr, frame_stride, len_ptr, n, pixels_ptr,
                                         self.pitch if image_pitch is None else image_pitch, status_ptr, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_raster_run failed ({rc}): {self.last_error()}")

    def parse(self, frames_ptr, frame_stride, len_ptr, n, status_ptr, stream=0):
        rc = self.L.asciichat_raster_parse(self._h, frames_ptr, frame_stride, len_ptr, n, status_ptr, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_raster_parse failed ({rc}): {self.last_error()}")

    def draw(self, n, pixels_ptr, image_pitch=None, stream=0):
        rc = self.L.asciichat_raster_draw(self._h, n, pixels_ptr, self.pitch if image_pitch is None else image_pitch, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_raster_draw failed ({rc}): {self.last_error()}")

    def run_yuv420(self, frames_ptr, frame_stride, len_ptr, n, yuv_ptr, status_ptr, layout, image_pitch=None, stream=0):
        """run(), but image i is the YUV 4:2:0 planes (layout RASTER_YUV_I420 | RASTER_YUV_NV12) at yuv_ptr + i * image_pitch, a
        multiple of 4 and at least yuv_pitch (default: yuv_pitch rounded up to 4); width and height must be even"""
        rc = self.L.asciichat_raster_run_yuv420(self._h, frames_ptr, frame_stride, len_ptr, n, yuv_ptr, self._yuv_pitch(image_pitch),
                                                layout, status_ptr, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_raster_run_yuv420 failed ({rc}): {self.last_error()}")

    def draw_yuv420(self, n, yuv_ptr, layout, image_pitch=None, stream=0):
        """the cells the last parse() left, as run_yuv420() draws them"""
        rc = self.L.asciichat_raster_draw_yuv420(self._h, n, yuv_ptr, self._yuv_pitch(image_pitch), layout, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_raster_draw_yuv420 failed ({rc}): {self.last_error()}")

    def set_images(self, mode, palette, frames, stream=0):
        """the frames the *_images methods work on: mode MODE_* 0..8, the renderers' palette, a list (or ctypes array) of
        binding.Frame with device-visible sources; checked on the host, copied asynchronously on `stream` (the handle's one
        stream).  No composites (set_images_composites takes those), no dithered mode (set_images_dithered takes that)"""
        from .binding import Frame
        arr = frames if isinstance(frames, C.Array) else (Frame * max(1, len(frames)))(*frames)
        p = palette.encode("utf-8") if isinstance(palette, str) else palette
        rc = self.L.asciichat_raster_images_set(self._h, mode, p, C.cast(arr, C.c_void_p), len(frames), stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_raster_images_set failed ({rc}): {self.last_error()}")

    def set_images_composites(self, mode, palette, frames, stream=0):
        """set_images for grid composites: a frame may carry comp, a device-visible composite descriptor as a Plan takes it
        (asciichat_hip_composite_upload, asciichat_hip_grid_composite_dev); its src is not read.  Plain and composite frames mix;
        replaces the last set of any kind.  The dithered mode is refused here too: set_images_dithered takes it"""
        from .binding import Frame
        arr = frames if isinstance(frames, C.Array) else (Frame * max(1, len(frames)))(*frames)
        p = palette.encode("utf-8") if isinstance(palette, str) else palette
        rc = self.L.asciichat_raster_images_set_composites(self._h, mode, p, C.cast(arr, C.c_void_p), len(frames), stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_raster_images_set_composites failed ({rc}): {self.last_error()}")

    def set_images_dithered(self, palette, frames, stream=0):
        """set_images for the Floyd-Steinberg renderer (MODE_16_DITHER_BG, implied): plain and composite frames, each in the
        style its ops carry (achip_frame_set_dither_style: background, foreground, foreground with the ramp glyph), out_w up to
        1024; replaces the last set of any kind"""
        from .binding import Frame
        arr = frames if isinstance(frames, C.Array) else (Frame * max(1, len(frames)))(*frames)
        p = palette.encode("utf-8") if isinstance(palette, str) else palette
        rc = self.L.asciichat_raster_images_set_dithered(self._h, p, C.cast(arr, C.c_void_p), len(frames), stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_raster_images_set_dithered failed ({rc}): {self.last_error()}")

    def cells_from_images(self, n, status_ptr, stream=0):
        """parse()'s counterpart: the cells of frames 0..n-1 of the last set_images, straight from their pixels"""
        rc = self.L.asciichat_raster_cells_from_images(self._h, n, status_ptr, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_raster_cells_from_images failed ({rc}): {self.last_error()}")

    def run_images(self, n, pixels_ptr, status_ptr, image_pitch=None, stream=0):
        """cells_from_images + draw: image i at pixels_ptr + i * image_pitch, what run() gives for Plan.render's text of the same
        descriptors; asynchronous"""
        rc = self.L.asciichat_raster_run_images(self._h, n, pixels_ptr, self.pitch if image_pitch is None else image_pitch, status_ptr,
                                                stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_raster_run_images failed ({rc}): {self.last_error()}")

    def run_images_yuv420(self, n, yuv_ptr, status_ptr, layout, image_pitch=None, stream=0):
        """cells_from_images + draw_yuv420, with run_yuv420()'s output arguments"""
        rc = self.L.asciichat_raster_run_images_yuv420(self._h, n, yuv_ptr, self._yuv_pitch(image_pitch), layout, status_ptr, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_raster_run_images_yuv420 failed ({rc}): {self.last_error()}")

    def _yuv_pitch(self, image_pitch):
        return (self.yuv_pitch + 3) // 4 * 4 if image_pitch is None else image_pitch

    def close(self):
        if self._h:
            self.L.asciichat_raster_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
