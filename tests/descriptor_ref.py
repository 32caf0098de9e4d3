"""A plain reference for the frame descriptor's sampling rule (include/achip_types.h, achip_frame_t), and the guarded
descriptor cases the kernel forms are judged on.  TESTS ONLY.

The rule: sx = min((x * x_ratio) >> 16, src_w - 1), sy likewise, computed here in Python integers (no wrap), then the flips
of `ops`, then the colour filter; pixel (sx, sy) sits at src + sy * stride + 3 * sx (stride 0 = 3 * src_w).  `expected`
emits the sampled image through the oracle at scale 1 and pads it as ascii_convert_with_capabilities does (width first,
then height).  Sources live inside a larger buffer whose row padding and guard zones hold a sentinel colour the image does
not contain: a sampler that reads the wrong pixel shows up as wrong bytes, not as a fault."""
import ctypes as C
from collections import namedtuple

import numpy as np

import emu
import orc
from achip_ctypes import MODE_CAPS, MODE_TRUE_BG, Frame

SENTINEL = (255, 0, 255)
FLIP_X, FLIP_Y = 1, 2
PRE = 48  # guard bytes in front of the source (a multiple of 3 and 16: the sentinel stays in phase with the pixels)

_filter_of_ops = None
_host = None  # (library exporting achip_frame_set_display_ops, its Frame structure); None: the emulator's


def use_host(lib, frame_cls):
    """build descriptors with another library's host helpers (the package's own on a GPU machine: no emulator build)"""
    global _host
    _host = (lib, frame_cls)


def host():
    return _host if _host is not None else (emu.lib(), Frame)


def filter_of_ops(ops):
    """the reference's colour filter (0 none, 1..11) that achip_frame_set_display_ops folds into `ops`"""
    global _filter_of_ops
    if _filter_of_ops is None:
        _filter_of_ops = {}
        lib, cls = host()
        for flt in range(12):
            f = cls()
            assert lib.achip_frame_set_display_ops(C.byref(f), False, False, flt) == 0
            _filter_of_ops[int(f.ops)] = flt
    return _filter_of_ops[int(ops) & ~(FLIP_X | FLIP_Y)]


def sample(desc, buf, base_offset=None):
    """-> out_h x out_w x 3: the pixels the descriptor addresses inside `buf` (a flat uint8 array holding the source)"""
    if base_offset is None:
        base_offset = int(desc.src) - buf.ctypes.data
    w, h = int(desc.src_w), int(desc.src_h)
    stride = int(desc.src_stride) or 3 * w
    xs = np.array([min((x * int(desc.x_ratio)) >> 16, w - 1) for x in range(int(desc.out_w))], dtype=np.int64)
    ys = np.array([min((y * int(desc.y_ratio)) >> 16, h - 1) for y in range(int(desc.out_h))], dtype=np.int64)
    if desc.ops & FLIP_X:
        xs = w - 1 - xs
    if desc.ops & FLIP_Y:
        ys = h - 1 - ys
    idx = base_offset + ys[:, None] * stride + 3 * xs[None, :]
    img = np.ascontiguousarray(np.stack([buf[idx], buf[idx + 1], buf[idx + 2]], axis=-1), dtype=np.uint8)
    flt = filter_of_ops(desc.ops)
    return orc.color_filter(img, flt) if flt else img


def expected(mode, desc, buf, palette=orc.PALETTE_STANDARD, base_offset=None):
    """the bytes the reference emits for what the descriptor samples, padded by its pad_left / pad_top"""
    img = sample(desc, buf, base_offset)
    if mode == MODE_TRUE_BG:
        s = orc.print_truecolor_bg(img, palette)
    else:
        cl, rm = MODE_CAPS[mode]
        s = orc.print_with_caps(img, cl, rm, palette)
    assert s, "the oracle emitted nothing"
    return orc.pad_height(orc.pad_width(s, int(desc.pad_left)), int(desc.pad_top))


def nn_ratio(src, out):
    return ((src << 16) // out) + 1


def source_image(w, h, seed):
    """noise without the sentinel colour"""
    img = orc.frame_hash_noise(w, h, seed).copy()
    hit = (img[..., 0] == SENTINEL[0]) & (img[..., 1] == SENTINEL[1]) & (img[..., 2] == SENTINEL[2])
    img[hit, 1] = 1
    return np.ascontiguousarray(img)


class Guarded:
    """a source inside a sentinel-filled buffer: PRE guard bytes, src_h rows of `stride` bytes (row padding = sentinel), then
    a guard as long as the furthest byte an unclamped sampler could reach, (out_h - 1) * stride + 3 * out_w + 4"""

    def __init__(self, img, stride, out_w, out_h):
        h, w = img.shape[:2]
        self.stride = stride or 3 * w
        after = (max(out_h, 1) - 1) * self.stride + 3 * out_w + 4 + 16
        n = PRE + (h - 1) * self.stride + 3 * w + after
        self.buf = np.resize(np.array(SENTINEL, dtype=np.uint8), n)
        for y in range(h):
            self.buf[PRE + y * self.stride:PRE + y * self.stride + 3 * w] = img[y].reshape(-1)
        self.base = PRE

    @property
    def src(self):
        return self.buf.ctypes.data + self.base


Case = namedtuple("Case", "name sw sh ow oh xr yr stride ops flt pl pt")


def case(name, sw, sh, ow, oh, xr=None, yr=None, stride=0, ops=0, flt=0, pl=0, pt=0):
    return Case(name, sw, sh, ow, oh, nn_ratio(sw, ow) if xr is None else xr, nn_ratio(sh, oh) if yr is None else yr,
                stride, ops, flt, pl, pt)


def ratio_ok(c):
    return (c.ow - 1) * c.xr < (1 << 32) and (c.oh - 1) * c.yr < (1 << 32)


def _named():
    top = (1 << 32) - 1
    base = [  # the ratio axis
        case("derived_down", 40, 24, 20, 10),
        case("derived_up", 9, 5, 30, 14),
        case("one16_same", 30, 14, 30, 14, 1 << 16, 1 << 16),
        case("one16_src_larger", 40, 20, 30, 14, 1 << 16, 1 << 16),
        case("one16_src_smaller", 12, 8, 30, 14, 1 << 16, 1 << 16),
        case("r65537_same", 30, 14, 30, 14, 65537, 65537),
        case("r65537_small_x", 20, 14, 30, 14, 65537, 65537),
        case("r65537_small_y", 30, 9, 30, 14, 65537, 65537),
        case("r65537_small_xy", 20, 9, 30, 14, 65537, 65537),
        case("r65537_large_x", 40, 14, 30, 14, 65537, 65537),
        case("r65537_large_y", 30, 20, 30, 14, 65537, 65537),
        case("r65537_large_xy", 40, 20, 30, 14, 65537, 65537),
        case("up_8000", 16, 10, 30, 14, 0x8000, 0x8000),
        case("up_C000", 16, 10, 30, 14, 0xC000, 0xC000),
        case("up_FFFF", 16, 10, 30, 14, 0xFFFF, 0xFFFF),
        case("odd_down", 64, 40, 20, 10, 0x12345, 0x20001),
        case("odd_down_clamped", 64, 40, 20, 10, 0x37FFF, 0x4FFFF),
        case("largest_ratio", 50, 30, 16, 4, top // 15, top // 3),
    ]
    out = []
    for i, c in enumerate(base):
        c = c._replace(pl=i % 6, pt=i % 4)
        out.append(c)
        for ops, tag in ((FLIP_X, "fx"), (FLIP_Y, "fy"), (FLIP_X | FLIP_Y, "fxy")):
            out.append(c._replace(name=f"{c.name}_{tag}", ops=ops, pl=(i + ops) % 6, pt=(i + ops) % 4))
        out.append(c._replace(name=c.name + "_fxy_filter", ops=FLIP_X | FLIP_Y, flt=1 + i % 11))
    for j, c in enumerate((base[0], base[8], base[13])):  # the stride axis
        w3 = 3 * c.sw
        for k, s in enumerate((3 * c.sw, w3 + 1, w3 + 2, w3 + 5, (w3 + 127) // 128 * 128 + 128)):
            out.append(c._replace(name=f"{c.name}_stride{s}", stride=s, ops=(j + k) % 4, pl=k % 6, pt=j % 4))
    near = (1 << 24) - 13
    out += [case("stride_near_2^24", 23, 2, 17, 2, stride=near, pl=1),
            case("stride_near_2^24_fxy", 23, 2, 17, 2, stride=near, ops=FLIP_X | FLIP_Y, flt=4)]
    out += [  # the shape axis
        case("out_1x1", 37, 21, 1, 1, pl=3, pt=1),
        case("out_1xN", 37, 21, 1, 13, ops=FLIP_Y),
        case("out_Nx1", 37, 21, 29, 1, ops=FLIP_X, pl=5),
        case("src_1xN", 1, 17, 12, 9, pt=3),
        case("src_1xN_fxy", 1, 17, 12, 9, ops=FLIP_X | FLIP_Y, pl=2),
        case("src_Nx1", 17, 1, 12, 9, ops=FLIP_X),
        case("src_2x1", 2, 1, 7, 4, ops=FLIP_X, pl=1, pt=2),
        case("src_2x1_65537", 2, 1, 7, 4, 65537, 65537),
        case("big_pads", 24, 12, 19, 6, pl=5, pt=3, ops=FLIP_Y, flt=11),
    ]
    return out


NAMED = _named()
ONE_BY_ONE = [case("src_1x1", 1, 1, 9, 5, pl=2, pt=1), case("src_1x1_fx_filter", 1, 1, 4, 3, ops=FLIP_X, flt=6)]
# The flipped ratio-1.0 cases with a source smaller than the output: an unclamped sampler would address memory about 4 GB
# away from them (a negative offset as 32 bits), so they run on the emulator only
FLIP_UNCLAMPED = frozenset(c.name for c in NAMED if c.name.startswith("r65537_small") and c.ops)


def random_cases(seed, n):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        sw, sh = int(rng.integers(1, 70)), int(rng.integers(1, 40))
        if sw * sh == 1:
            sw = 2
        ow, oh = int(rng.integers(1, 48)), int(rng.integers(1, 20))
        kind = int(rng.integers(0, 5))
        if kind == 0:
            xr, yr = nn_ratio(sw, ow), nn_ratio(sh, oh)
        elif kind == 1:
            xr, yr = 1 << 16, 1 << 16
        elif kind == 2:  # ratio 1.0 on equal sizes only (the mismatched sizes are named cases)
            sw = ow = max(ow, 2)
            sh = oh
            xr, yr = 65537, 65537
        elif kind == 3:
            xr, yr = int(rng.integers(0x4000, 0x10000)), int(rng.integers(0x4000, 0x10000))
        else:
            xr, yr = int(rng.integers(0x10001, 0x60000)), int(rng.integers(0x10001, 0x60000))
        stride = [0, 3 * sw, 3 * sw + int(rng.integers(1, 9)), (3 * sw + 127) // 128 * 128][int(rng.integers(0, 4))]
        out.append(Case(f"random{seed}_{i}", sw, sh, ow, oh, xr, yr, stride, int(rng.integers(0, 4)),
                        int(rng.integers(0, 12)) if rng.integers(0, 3) == 0 else 0, int(rng.integers(0, 6)),
                        int(rng.integers(0, 4))))
    return out


def make_frame(c, src_ptr):
    lib, cls = host()
    f = cls()
    f.src, f.comp = src_ptr, None
    f.src_w, f.src_h, f.out_w, f.out_h = c.sw, c.sh, c.ow, c.oh
    f.pad_left, f.pad_top = c.pl, c.pt
    f.x_ratio, f.y_ratio = c.xr, c.yr
    f.src_stride = c.stride
    assert lib.achip_frame_set_display_ops(C.byref(f), bool(c.ops & FLIP_X), bool(c.ops & FLIP_Y), c.flt) == 0
    return f


def as_frame(cls, f):
    """the same descriptor as another binding's Frame structure (the package's own, for plans)"""
    g = cls()
    for name, _ in Frame._fields_:
        setattr(g, name, getattr(f, name))
    return g


def build(cases, seed=1):
    """-> [(case, Guarded, Frame)] with every source in a guarded buffer of its own"""
    out = []
    for i, c in enumerate(cases):
        g = Guarded(source_image(c.sw, c.sh, seed + i), c.stride, c.ow, c.oh)
        out.append((c, g, make_frame(c, g.src)))
    return out


def forced_geometries(pkg, mode, frames, geometries):
    """-> the geometries of `geometries` (built into pkg's library) that a plan forced to them takes, as the host's policy
    decides (achip_choose_geometry with the plan's caps); asserts that set_variant agrees: it succeeds on exactly those"""
    L = pkg.lib()
    L.achip_variant_block.restype = L.achip_variant_cap.restype = C.c_int
    L.achip_variant_block.argtypes = L.achip_variant_cap.argtypes = [C.c_int]
    L.achip_choose_geometry.restype = C.c_int
    L.achip_choose_geometry.argtypes = [C.c_int, C.POINTER(pkg.Frame), C.c_int, C.c_bool, C.POINTER(C.c_int), C.c_int, C.c_int,
                                        C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    caps = (C.c_int * 5)(*[L.achip_variant_cap(v) for v in range(5)])
    arr = (pkg.Frame * len(frames))(*frames)
    taken = []
    for v in geometries:
        if L.achip_variant_block(v) <= 0:
            continue
        got, parts, rpp = C.c_int(-1), C.c_int(0), C.c_int(0)
        applies = L.achip_choose_geometry(mode, arr, len(frames), True, caps, 256, -1, v, C.byref(got), C.byref(parts),
                                          C.byref(rpp)) == 0 and got.value == v
        plan = pkg.Plan(mode, orc.PALETTE_STANDARD, frames)
        try:
            if applies:
                plan.set_variant(v)  # must take it
                taken.append(v)
            else:
                try:
                    plan.set_variant(v)
                except RuntimeError:
                    continue
                raise AssertionError(f"mode {mode}: set_variant({v}) took frames its policy refuses")
        finally:
            plan.close()
    return taken
