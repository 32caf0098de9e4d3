"""ctypes binding of libasciichat_pixgrid.so (include/asciichat_pixgrid.h): packed RGB camera frames -- RGB24, RGBA, BGR24, BGRA --
as the tiles of grid composites, on the device: one launch leaves the pixels the composite samplers read of every packed source
(PixGrid.run), or the box average of its whole conversion at the tile's size (PixGrid.run_box: opt-in and not a parity mode, as
the box pass is not), and PixGrid.composites hands back the descriptors rewritten onto those tiles."""
import ctypes as C
import os

from .pix import PixSource

__all__ = ["PixGrid", "pixgrid_lib", "PIXGRID_LIB_PATH"]

HERE = os.path.dirname(os.path.abspath(__file__))
PIXGRID_LIB_PATH = os.path.join(HERE, "libasciichat_pixgrid.so")
SLOTS = 9

_lib = None


def pixgrid_lib(path=None):
    """Load libasciichat_pixgrid.so (never a substitute: raises if it has not been built).  path: another build of it -- one at
    another segment width, for scripts/pixgrid_timing.py --, loaded beside the package's own and not kept."""
    global _lib
    if path is not None:
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing")
        return _bound(C.CDLL(path))
    if _lib is not None:
        return _lib
    try:
        import torch  # noqa: F401  (its libamdhip64 first, as binding.lib() does)
    except ImportError:
        pass
    if not os.path.exists(PIXGRID_LIB_PATH):
        raise RuntimeError(f"{PIXGRID_LIB_PATH} is missing: run __graft_entry__.build() (hipcc, gfx950) first")
    _lib = _bound(C.CDLL(PIXGRID_LIB_PATH))
    return _lib


def _bound(L):
    vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
    for name, res, args in (("asciichat_pixgrid_device_count", ci, []),
                            ("asciichat_pixgrid_last_error", C.c_char_p, []),
                            ("asciichat_pixgrid_create", ci, [C.POINTER(vp), ci]),
                            ("asciichat_pixgrid_set", ci, [vp, vp, vp, ci, vp]),
                            ("asciichat_pixgrid_tiles_bytes", sz, [vp]),
                            ("asciichat_pixgrid_run", ci, [vp, vp, vp]),
                            ("asciichat_pixgrid_run_box", ci, [vp, vp, vp]),
                            ("asciichat_pixgrid_composites", ci, [vp, vp, vp]),
                            ("asciichat_pixgrid_destroy", None, [vp])):
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    return L


class PixGrid:
    """A handle for up to max_tiles packed slots per tick (asciichat_pixgrid_*): set() takes the tick's host composite descriptors
    and, beside the nine slots of each, the packed sources; run() leaves the sampled tiles, run_box() the averaged ones;
    composites() the descriptors rewritten onto them, to upload with asciichat_hip_composite_upload once per geometry, to hand to
    Box(frames, comps=...), or to give to YuvGrid.set / YuvBoxGrid.set for the YUV slots of the same tick (and the other way
    round: what their composites() return is a set for this one)."""

    def __init__(self, max_tiles, lib=None):
        self.L = lib or pixgrid_lib()
        self._h = C.c_void_p()
        rc = self.L.asciichat_pixgrid_create(C.byref(self._h), max_tiles)
        if rc != 0:
            raise RuntimeError(f"asciichat_pixgrid_create failed ({rc}): {self.last_error()}")
        self.n_comps = 0

    def last_error(self):
        return self.L.asciichat_pixgrid_last_error().decode("utf-8", "replace")

    def set(self, comps, sources, stream=0):
        """comps: a list of binding.Composite (host descriptors); sources: per composite a list of up to nine PixSource or None
        (None, or a source without pixels: the slot is left as it stands).  Checked on the host, copied asynchronously on
        `stream` (the handle's one stream)"""
        n = len(comps)
        if len(sources) != n:
            raise ValueError("as many source lists as composites")
        nines = []
        for per in sources:
            if len(per) > SLOTS:
                raise ValueError("at most nine sources per composite")
            arr = (PixSource * SLOTS)()
            for k, s in enumerate(per):
                if s is not None:
                    arr[k] = s
            nines.append(arr)
        cp = (C.c_void_p * max(1, n))(*[C.addressof(c) for c in comps])
        sp = (C.c_void_p * max(1, n))(*[C.addressof(a) for a in nines])
        rc = self.L.asciichat_pixgrid_set(self._h, C.cast(cp, C.c_void_p), C.cast(sp, C.c_void_p), n, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_pixgrid_set failed ({rc}): {self.last_error()}")
        self.n_comps = n

    def tiles_bytes(self):
        """the bytes of the tile slab the set needs (0 without packed slots)"""
        return int(self.L.asciichat_pixgrid_tiles_bytes(self._h))

    def run(self, tiles_ptr, stream=0):
        """every sampled tile of every composite of the set into the slab at tiles_ptr (16-aligned), one launch; asynchronous"""
        rc = self.L.asciichat_pixgrid_run(self._h, tiles_ptr, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_pixgrid_run failed ({rc}): {self.last_error()}")

    def run_box(self, tiles_ptr, stream=0):
        """every averaged tile of every composite of the set into the slab at tiles_ptr (16-aligned), one launch; asynchronous"""
        rc = self.L.asciichat_pixgrid_run_box(self._h, tiles_ptr, stream)
        if rc != 0:
            raise RuntimeError(f"asciichat_pixgrid_run_box failed ({rc}): {self.last_error()}")

    def composites(self, tiles_ptr):
        """-> the set's descriptors with every packed slot rewritten onto its tile (a list of binding.Composite)"""
        from .binding import Composite
        out = (Composite * max(1, self.n_comps))()
        rc = self.L.asciichat_pixgrid_composites(self._h, tiles_ptr, C.cast(out, C.c_void_p))
        if rc != 0:
            raise RuntimeError(f"asciichat_pixgrid_composites failed ({rc}): {self.last_error()}")
        return [out[i] for i in range(self.n_comps)]

    def close(self):
        if self._h:
            self.L.asciichat_pixgrid_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
