"""Digital rain test support: the sequential C restatement (tests/cabi/rain_restatement.c), the kernel under the CPU
emulator (tests/hipemu/rain_emu_driver.cpp), and the ctypes mirror of the context they share with the product. TESTS ONLY."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ascii-chat_amd", "csrc")
INC = os.path.join(ROOT, "include")
EMU_DIR = os.path.join(ROOT, "tests", "hipemu")
OUT_DIR = os.path.join(EMU_DIR, "_build")
GOLDEN = os.path.join(ROOT, "tests", "golden", "digital_rain.json")
GOLDEN_EDGES = os.path.join(ROOT, "tests", "golden", "digital_rain_edges.json")
TABLE_MAX = 12288
LEN_OVERFLOW = 0xFFFFFFFF


class Column(C.Structure):
    _fields_ = [("time_offset", C.c_float), ("speed_multiplier", C.c_float), ("phase_offset", C.c_float)]


class RainT(C.Structure):  # digital_rain_t
    _fields_ = [("columns", C.POINTER(Column)), ("num_columns", C.c_int), ("num_rows", C.c_int), ("time", C.c_float),
                ("fall_speed", C.c_float), ("raindrop_length", C.c_float), ("brightness_decay", C.c_float),
                ("animation_speed", C.c_float), ("color_r", C.c_uint8), ("color_g", C.c_uint8), ("color_b", C.c_uint8),
                ("cursor_brightness", C.c_float), ("rainbow_mode", C.c_bool), ("first_frame", C.c_bool),
                ("previous_brightness", C.POINTER(C.c_float))]


class Desc(C.Structure):  # achip_rain_desc_t (csrc/rain.h)
    _fields_ = [("state", C.c_void_p), ("cols", C.c_void_p), ("t", C.c_float), ("fall_speed", C.c_float),
                ("raindrop_length", C.c_float), ("decay", C.c_float), ("color", C.c_uint32), ("num_columns", C.c_int32),
                ("num_rows", C.c_int32), ("backup", C.c_uint32)]


def _fresh(out, srcs):
    return os.path.exists(out) and all(os.path.getmtime(s) <= os.path.getmtime(out) for s in srcs)


def _build(out, srcs, cmd):
    if _fresh(out, srcs):
        return out
    os.makedirs(OUT_DIR, exist_ok=True)
    tmp = out + ".%d.tmp" % os.getpid()
    subprocess.check_call(cmd + ["-o", tmp])
    os.replace(tmp, out)
    return out


_restate = None
_emu = None


def restatement():
    global _restate
    if _restate is None:
        src = os.path.join(ROOT, "tests", "cabi", "rain_restatement.c")
        host = os.path.join(CSRC, "achip_host.c")  # color_filter_calculate_rainbow's walk (achip_rainbow_color): plain C
        so = _build(os.path.join(OUT_DIR, "librain_restatement.so"), [src, host],
                    ["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I" + INC, src, host, "-lm"])
        L = C.CDLL(so)
        L.rs_init.restype = C.POINTER(RainT)
        L.rs_init.argtypes = [C.c_int, C.c_int]
        L.rs_destroy.argtypes = [C.POINTER(RainT)]
        L.rs_reset.argtypes = [C.POINTER(RainT)]
        L.rs_apply.restype = C.c_void_p
        L.rs_apply.argtypes = [C.POINTER(RainT), C.c_char_p, C.c_float, C.POINTER(C.c_size_t)]
        L.rs_set_color_from_filter.argtypes = [C.POINTER(RainT), C.c_int]
        L.free = C.CDLL(None).free
        L.free.argtypes = [C.c_void_p]
        _restate = L
    return _restate


def emulator():
    global _emu
    if _emu is None:
        drv = os.path.join(EMU_DIR, "rain_emu_driver.cpp")
        srcs = [drv, os.path.join(EMU_DIR, "hip_emu.h"), os.path.join(EMU_DIR, "gfx950_ops.hpp"),
                os.path.join(CSRC, "rain_kernels.hpp"), os.path.join(CSRC, "rain.h"), os.path.join(INC, "achip_types.h")]
        so = _build(os.path.join(OUT_DIR, "librain_emu.so"), srcs,
                    ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I" + EMU_DIR, "-I" + CSRC,
                     "-I" + INC, drv])
        L = C.CDLL(so)
        L.emu_rain.restype = None
        L.emu_rain.argtypes = [C.POINTER(Desc), C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                               C.c_uint64, C.c_void_p]
        _emu = L
    return _emu


class Restated:
    """One restatement context; apply() returns the output bytes."""

    def __init__(self, cols, rows):
        L = restatement()
        self.p = L.rs_init(cols, rows)
        assert self.p
        self.r = self.p.contents
        self.cols, self.rows = cols, rows

    def apply(self, frame, dt):
        L = restatement()
        n = C.c_size_t()
        ptr = L.rs_apply(self.p, frame, C.c_float(dt), C.byref(n))
        out = C.string_at(ptr, n.value)
        L.free(ptr)
        return out

    def state(self):
        return [self.r.previous_brightness[i] for i in range(self.cols * self.rows)]

    def reset(self):
        restatement().rs_reset(self.p)

    def set_color_from_filter(self, f):
        restatement().rs_set_color_from_filter(self.p, f)

    def set_color(self, r, g, b):
        self.r.color_r, self.r.color_g, self.r.color_b = r, g, b

    def set_fall_speed(self, v):
        self.r.fall_speed = v

    def set_raindrop_length(self, v):
        self.r.raindrop_length = v

    def set_field(self, name, v):
        setattr(self.r, name, v)

    def close(self):
        if self.p:
            restatement().rs_destroy(self.p)
            self.p = None



def rainbow(t):
    """color_filter_calculate_rainbow(t) by the product's host helper (linked into the restatement library)."""
    L = restatement()
    r, g, b = C.c_uint8(), C.c_uint8(), C.c_uint8()
    L.achip_rainbow_color(C.c_float(t), C.byref(r), C.byref(g), C.byref(b))
    return r.value, g.value, b.value


class Emulated:
    """A context whose device state lives in numpy arrays; batches go through the kernel under the emulator.  Its public
    fields are a digital_rain_t (held by a restatement context, whose own grid stays unused), advanced as rain.c
    advances them when a call is issued."""

    def __init__(self, cols, rows):
        import numpy as np
        self.h = Restated(cols, rows)
        self.s = self.h.r
        self.cols, self.rows = cols, rows
        self.colv = np.array([[self.s.columns[c].time_offset, self.s.columns[c].speed_multiplier] for c in range(cols)],
                             dtype=np.float32).ravel()
        self.state = np.zeros(2 * cols * rows, dtype=np.float32)
        self.backup = cols * rows  # as rain.c fills the descriptor; 0 is the kernel's default, behind the grid as written

    def __getattr__(self, name):  # the setters: set_color_from_filter, set_color, set_fall_speed, ...
        return getattr(self.h, name)

    def reset(self):
        self.h.reset()
        self.state[:self.cols * self.rows] = 0

    def desc(self, dt):
        import numpy as np
        f = np.float32
        s = self.s
        s.time = float(f(f(s.time) + f(f(dt) * f(s.animation_speed))))
        if s.rainbow_mode:
            s.color_r, s.color_g, s.color_b = rainbow(s.time)
        d = Desc(self.state.ctypes.data, self.colv.ctypes.data, s.time, s.fall_speed, s.raindrop_length, s.brightness_decay,
                 s.color_r | s.color_g << 8 | s.color_b << 16 | (1 << 24 if s.first_frame else 0), s.num_columns, s.num_rows, self.backup)
        s.first_frame = False
        return d

    def grid(self):
        return [float(v) for v in self.state[:self.cols * self.rows]]

    def close(self):
        self.h.close()


def emu_batch(items, dst_stride=None, src_stride=None, src_lens=None):
    """items: [(Emulated, frame bytes, dt)]; returns [bytes, or LEN_OVERFLOW / the error code that travelled through].
    src_lens: the lengths the kernel is told, where they are not the frames' own."""
    import numpy as np
    n = len(items)
    if src_stride is None:
        src_stride = max(16, (max(len(f) for _, f, _ in items) + 15) // 16 * 16)
    if dst_stride is None:
        dst_stride = (20 * src_stride + 1 + 15) // 16 * 16
    src = np.zeros(n * src_stride + 64, dtype=np.uint8)
    for i, (_, f, _) in enumerate(items):
        src[i * src_stride:i * src_stride + len(f)] = np.frombuffer(f, dtype=np.uint8)
    src_len = np.array(src_lens if src_lens is not None else [len(f) for _, f, _ in items], dtype=np.uint32)
    dst = np.full(n * dst_stride + 64, 0xEE, dtype=np.uint8)
    dst_len = np.zeros(n, dtype=np.uint32)
    descs = (Desc * n)(*[ctx.desc(dt) for ctx, _, dt in items])
    table = max([c.s.num_columns * (c.s.num_rows + 1) for c, _, _ in items if c.s.num_columns * (c.s.num_rows + 1) <= TABLE_MAX],
                default=0)
    emulator().emu_rain(descs, n, table, src.ctypes.data, src_stride, src_len.ctypes.data, dst.ctypes.data, dst_stride,
                        dst_len.ctypes.data)
    assert (dst[n * dst_stride:] == 0xEE).all(), "a store past the last slot"
    out = []
    for i in range(n):
        ln = int(dst_len[i])
        if ln >= 0xFFFFFFF0:
            out.append(ln)
        else:
            assert ln < dst_stride and dst[i * dst_stride + ln] == 0
            out.append(bytes(dst[i * dst_stride:i * dst_stride + ln]))
    return out


def apply_ops(ctx, ops):
    """a fixture step's calls and direct field writes, on a Restated / Emulated / product Rain context"""
    for op in ops:
        if op[0] == "filter":
            ctx.set_color_from_filter(op[1])
        elif op[0] == "color":
            ctx.set_color(*op[1:])
        elif op[0] == "reset":
            ctx.reset()
        elif op[0] == "fall_speed_call":
            ctx.set_fall_speed(op[1])
        elif op[0] == "raindrop_length_call":
            ctx.set_raindrop_length(op[1])
        else:
            ctx.set_field(op[0], op[1])
