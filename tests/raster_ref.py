"""The rasteriser restated in Python (asciichat_raster.h): an ANSI frame to a cell grid, the cell grid to RGBA pixels, painted
literally in the order of the reference's compositor.  Line numbers are those of the reference's
lib/media/render/terminal.c.  TESTS ONLY: the kernels implement the per-pixel "last writer" rule instead, their agreement with
this loop is the test."""
import numpy as np

NO_FRAME, BAD_UTF8, UNKNOWN, OVERFLOW_COLS, OVERFLOW_ROWS = 1, 2, 4, 8, 16
INDEXED_FLAT, INDEXED_XTERM = 1, 2
LEN_OVERFLOW = 0xFFFFFFFF
SATURATE = 65535  # a decimal parameter stops growing here

# get_16color_rgb of this project (ascii-chat_amd/csrc/hostutil.c)
ANSI16 = [(0, 0, 0), (128, 0, 0), (0, 128, 0), (128, 128, 0), (0, 0, 128), (128, 0, 128), (0, 128, 128), (192, 192, 192),
          (128, 128, 128), (255, 0, 0), (0, 255, 0), (255, 255, 0), (0, 0, 255), (255, 0, 255), (0, 255, 255), (255, 255, 255)]
CUBE = [0, 95, 135, 175, 215, 255]


class Glyph:
    def __init__(self, codepoint, left, top, width, rows, pitch, offset):
        self.codepoint, self.left, self.top, self.width, self.rows, self.pitch, self.offset = (codepoint, left, top, width, rows,
                                                                                              pitch, offset)


class Font:
    """asciichat_raster_font_t"""

    def __init__(self, cell_w, cell_h, baseline, glyphs, coverage, default_fg=0xCCCCCC, default_bg=0x000000, indexed=INDEXED_FLAT,
                 flat_fg=0xCCCCCC, flat_bg=0x000000, matrix_map=False):
        self.cell_w, self.cell_h, self.baseline = cell_w, cell_h, baseline
        self.glyphs = list(glyphs)
        self.coverage = np.asarray(coverage, dtype=np.uint8)
        self.default_fg, self.default_bg, self.indexed = default_fg, default_bg, indexed
        self.flat_fg, self.flat_bg, self.matrix_map = flat_fg, flat_bg, matrix_map

    def replace(self, **kw):
        f = Font(self.cell_w, self.cell_h, self.baseline, self.glyphs, self.coverage, self.default_fg, self.default_bg, self.indexed,
                 self.flat_fg, self.flat_bg, self.matrix_map)
        for k, v in kw.items():
            setattr(f, k, v)
        return f


def xterm_rgb(n):
    if n < 16:
        r, g, b = ANSI16[n]
    elif n < 232:
        n -= 16
        r, g, b = CUBE[n // 36], CUBE[n // 6 % 6], CUBE[n % 6]
    else:
        r = g = b = 8 + 10 * (n - 232)
    return r << 16 | g << 8 | b


def indexed_rgb(font, n, is_fg):
    """FLAT: what the reference draws for a colour that is not VTERM_COLOR_IS_RGB (:474-488)"""
    if font.indexed == INDEXED_FLAT:
        return font.flat_fg if is_fg else font.flat_bg
    return xterm_rgb(n)


def matrix_char_map(cp):
    """:146-165"""
    if 0xE900 <= cp <= 0xE91A:
        return cp
    if 32 <= cp <= 126:
        return 0xE900 + (cp - 32) % 27
    return cp


def find_glyph(font, cp):
    """the glyph a cell of codepoint cp draws, or None: 0 and ' ' draw nothing (:507), nor does a codepoint the face lacks
    (:94-96) or an empty bitmap (:513)"""
    if cp == 0 or cp == 0x20:
        return None
    if font.matrix_map:
        cp = matrix_char_map(cp)  # :509
    for g in font.glyphs:
        if g.codepoint == cp:
            return g if g.width > 0 and g.rows > 0 else None
    return None


def _params(body):
    """the ';'-separated decimal parameters of a CSI: a list of values (empty = None), or None when a byte is no digit"""
    out = []
    for part in body.split(b";"):
        if not part:
            out.append(None)
        elif part.isdigit():
            out.append(min(int(part), SATURATE))
        else:
            return None
    return out


def parse(frame, cols, rows, font):
    """-> (cells[rows][cols] of (codepoint, fg, bg), status).  frame None: the ACHIP_LEN_OVERFLOW sentinel."""
    blank = (0, font.default_fg, font.default_bg)
    cells = [[blank] * cols for _ in range(rows)]
    if frame is None:
        return cells, NO_FRAME
    status = 0
    fg, bg = font.default_fg, font.default_bg  # a fresh pen per frame (the reference's survives from the frame before)
    row = col = 0
    last = None  # the last character of this row
    n = len(frame)

    def put(cp, times=1):
        nonlocal col, last, status
        for _ in range(times):
            if row >= rows:
                status |= OVERFLOW_ROWS  # (the reference would scroll)
            elif col >= cols:
                status |= OVERFLOW_COLS  # (the reference would wrap)
            else:
                cells[row][col] = (cp, fg, bg)
            if col < cols:
                col += 1
        last = cp

    i = 0
    while i < n:
        b = frame[i]
        if b == 0x0A:
            row, col, last = row + 1, 0, None
            i += 1
        elif b == 0x0D:
            col = 0
            i += 1
        elif b == 0x1B:
            if i + 1 >= n or frame[i + 1] != 0x5B:
                status |= UNKNOWN
                i += 1
                continue
            j = i + 2
            while j < n and 0x30 <= frame[j] <= 0x3F:
                j += 1
            p_end = j
            while j < n and 0x20 <= frame[j] <= 0x2F:
                j += 1
            if j >= n or not 0x40 <= frame[j] <= 0x7E:
                status |= UNKNOWN  # not a control sequence: dropped up to the byte that broke it, which counts for itself
                i = j
                continue
            final, interm = frame[j], j > p_end
            par = _params(frame[i + 2:p_end])
            i = j + 1
            if final == 0x6D and not interm and par is not None:  # SGR
                k = 0
                while k < len(par):
                    p = par[k] or 0
                    if p == 0:
                        fg, bg = font.default_fg, font.default_bg
                    elif p in (38, 48):
                        sel = (par[k + 1] or 0) if k + 1 < len(par) else None
                        if sel == 2:
                            if k + 4 < len(par):
                                r, g, bl = (par[k + 2] or 0), (par[k + 3] or 0), (par[k + 4] or 0)
                                if max(r, g, bl) <= 255:
                                    if p == 38:
                                        fg = r << 16 | g << 8 | bl
                                    else:
                                        bg = r << 16 | g << 8 | bl
                                else:
                                    status |= UNKNOWN
                            else:
                                status |= UNKNOWN
                            k += 4
                        elif sel == 5:
                            if k + 2 < len(par) and (par[k + 2] or 0) <= 255:
                                if p == 38:
                                    fg = indexed_rgb(font, par[k + 2] or 0, True)
                                else:
                                    bg = indexed_rgb(font, par[k + 2] or 0, False)
                            else:
                                status |= UNKNOWN
                            k += 2
                        else:
                            status |= UNKNOWN
                            k += 1
                    elif 30 <= p <= 37 or 90 <= p <= 97:
                        fg = indexed_rgb(font, p - 30 if p < 90 else p - 90 + 8, True)
                    elif 40 <= p <= 47 or 100 <= p <= 107:
                        bg = indexed_rgb(font, p - 40 if p < 100 else p - 100 + 8, False)
                    elif p == 39:
                        fg = font.default_fg
                    elif p == 49:
                        bg = font.default_bg
                    else:
                        status |= UNKNOWN
                    k += 1
            elif final == 0x62 and not interm and par is not None and len(par) == 1:  # REP
                if last is None:
                    status |= UNKNOWN
                else:
                    put(last, par[0] or 1)
            else:
                status |= UNKNOWN
        elif b < 0x20 or b == 0x7F:
            status |= UNKNOWN
            i += 1
        elif b < 0x80:
            put(b)
            i += 1
        else:
            need = 1 if 0xC2 <= b <= 0xDF else 2 if 0xE0 <= b <= 0xEF else 3 if 0xF0 <= b <= 0xF4 else 0
            if need == 0:
                status |= BAD_UTF8
                put(0xFFFD)
                i += 1
                continue
            cp = b & (0x1F if need == 1 else 0x0F if need == 2 else 0x07)
            j = i + 1
            while j < n and j - i <= need and 0x80 <= frame[j] <= 0xBF:
                cp = cp << 6 | (frame[j] & 0x3F)
                j += 1
            ok = j - i == need + 1
            if ok and (cp < (0x80, 0x800, 0x10000)[need - 1] or 0xD800 <= cp <= 0xDFFF or cp > 0x10FFFF):
                ok = False
            if not ok:
                status |= BAD_UTF8
                cp = 0xFFFD
            put(cp)
            i = j
    return cells, status


def rasterise(cells, cols, rows, font):
    """the loop of term_renderer_feed, :468-525 -> uint8[rows * cell_h][cols * cell_w][4]"""
    cw, ch = font.cell_w, font.cell_h
    W, H = cols * cw, rows * ch
    img = np.zeros((H, W, 4), dtype=np.uint8)
    cov = font.coverage
    for row in range(rows):
        for col in range(cols):
            cp, fg, bg = cells[row][col]
            f = (fg >> 16 & 255, fg >> 8 & 255, fg & 255)
            b = (bg >> 16 & 255, bg >> 8 & 255, bg & 255)
            px, py = col * cw, row * ch
            img[py:py + ch, px:px + cw] = (b[0], b[1], b[2], 255)  # :490-505
            g = find_glyph(font, cp)
            if g is None:
                continue
            gx, gy = px + g.left, py + font.baseline - g.top  # :518
            for r in range(g.rows):  # blit_glyph, :170-193
                dy = gy + r
                if dy < 0 or dy >= H:
                    continue
                for c in range(g.width):
                    dx = gx + c
                    if dx < 0 or dx >= W:
                        continue
                    a = int(cov[g.offset + r * g.pitch + c])
                    img[dy, dx] = ((f[0] * a + b[0] * (255 - a)) // 255, (f[1] * a + b[1] * (255 - a)) // 255,
                                   (f[2] * a + b[2] * (255 - a)) // 255, 255)  # :183-190
    return img


def render(frame, cols, rows, font):
    """-> (image, status)"""
    cells, status = parse(frame, cols, rows, font)
    return rasterise(cells, cols, rows, font), status
