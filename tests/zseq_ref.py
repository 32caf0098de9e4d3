"""The "zseq" wire form restated in Python (sequence form): the zstd frame of tests/zwide_ref.py cut every
PIECE bytes, every block's bytes parsed greedily into matches of a 64-byte window, the unmatched bytes sent as the wide form's
literals section (or raw literals) and the matches as a sequences section under zstd's predefined FSE tables.  encode() /
wire() are what the device must produce byte for byte; decode() is a decoder of exactly this subset written from the format
(decoding tables, backward bitstream, sequence execution) and not by inverting the encoder; libzstd's ZSTD_decompress is the
judge (zhuf_ref.zstd_decompress).  TESTS ONLY."""
import struct

import numpy as np

import zhuf_ref as Z
import zwide_ref as W

PIECE = 8192
WINDOW = 64  # distances tried
MAX_MATCH = 130
MIN_MATCH = 4

LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DIST = [4, 3] + [2] * 11 + [1] * 3 + [2] * 9 + [3, 2] + [1] * 5 + [-1] * 4
ML_DIST = [1, 4, 3] + [2] * 6 + [1] * 37 + [-1] * 7
OF_DIST = [1] * 6 + [2] * 3 + [1] * 15 + [-1] * 5
LL_LOG, ML_LOG, OF_LOG = 6, 6, 5
assert len(LL_BASE) == len(LL_BITS) == len(LL_DIST) == 36 and len(ML_BASE) == len(ML_BITS) == len(ML_DIST) == 53 and len(OF_DIST) == 29
assert sum(abs(x) for x in LL_DIST) == 64 and sum(abs(x) for x in ML_DIST) == 64 and sum(abs(x) for x in OF_DIST) == 32


# ---- matches ---------------------------------------------------------------------------------------------------------------
def best_matches(f, a, b):
    """-> (m[b - a], d[b - a]): at every position of block [a, b) of frame f the longest match among distances 1 .. min(64, i)
    capped at min(130, b - i), the smallest distance among equals; m = 0 where b - i < 4 or nothing matches"""
    n = b - a
    arr = np.frombuffer(f, dtype=np.uint8)
    lens = np.zeros((WINDOW, n), dtype=np.int32)
    idx = np.arange(n + 1)
    for d in range(1, WINDOW + 1):
        lo = max(a, d)  # i - d >= 0
        if lo >= b:
            break
        eq = np.zeros(n + 1, dtype=bool)  # (a False behind the block's end)
        eq[lo - a:n] = arr[lo:b] == arr[lo - d:b - d]
        stop = np.where(eq, n + 1, idx)  # the next position that differs, by a running minimum from the back
        stop = np.minimum.accumulate(stop[::-1])[::-1]
        lens[d - 1] = (stop - idx)[:n]
    lens = np.minimum(lens, MAX_MATCH)
    d = np.argmax(lens, axis=0)  # the first of the largest: the smallest distance
    m = lens[d, np.arange(n)]
    m[max(0, n - MIN_MATCH + 1):] = 0
    return m, d + 1


def parse(f, a, b):
    """greedy from a -> (sequences [(LL, ML, OFF)], literal bytes)"""
    m, d = best_matches(f, a, b)
    seqs, lits, i, start = [], bytearray(), a, a
    while i < b:
        if m[i - a] >= MIN_MATCH:
            seqs.append((i - start, int(m[i - a]), int(d[i - a])))
            lits += f[start:i]
            i += int(m[i - a])
            start = i
        else:
            i += 1
    lits += f[start:b]
    return seqs, bytes(lits)


# ---- codes -----------------------------------------------------------------------------------------------------------------
def _code(base, v):
    c = 0
    while c + 1 < len(base) and base[c + 1] <= v:
        c += 1
    return c


def ll_code(ll):
    return ll if ll < 16 else _code(LL_BASE, ll)


def ml_code(ml):
    return ml - 3 if ml <= 34 else _code(ML_BASE, ml)


def of_code(off):
    return (off + 3).bit_length() - 1


# ---- the coding table of a predefined distribution -------------------------------------------------------------------------
def coding_table(dist, log):
    """-> (stateTable[size], deltaNbBits[symbols], deltaFindState[symbols])"""
    size = 1 << log
    cells, high = [None] * size, size - 1
    for s, p in enumerate(dist):  # "less than 1": one cell each from the top down
        if p == -1:
            cells[high] = s
            high -= 1
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, p in enumerate(dist):
        for _ in range(max(p, 0)):
            cells[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0 and None not in cells
    cumul, total = [], 0
    for p in dist:
        cumul.append(total)
        total += abs(p)
    state = [0] * size
    nxt = list(cumul)
    for u in range(size):
        state[nxt[cells[u]]] = size + u
        nxt[cells[u]] += 1
    dnb, dfs = [], []
    for s, p in enumerate(dist):
        n = abs(p)
        if n == 1:
            dnb.append((log << 16) - size)
            dfs.append(cumul[s] - 1)
        else:
            b = log - ((n - 1).bit_length() - 1)
            dnb.append((b << 16) - (n << b))
            dfs.append(cumul[s] - n)
    return state, dnb, dfs


class _Coder:
    def __init__(self, dist, log, out):
        self.st, self.dnb, self.dfs = coding_table(dist, log)
        self.log, self.out, self.state = log, out, None

    def init(self, x):
        nb = (self.dnb[x] + 32768) >> 16
        self.state = self.st[(((nb << 16) - self.dnb[x]) >> nb) + self.dfs[x]]

    def put(self, x):
        nb = (self.state + self.dnb[x]) >> 16
        self.out.put(self.state & ((1 << nb) - 1), nb)
        self.state = self.st[(self.state >> nb) + self.dfs[x]]

    def flush(self):
        self.out.put(self.state - (1 << self.log), self.log)


def sequences_section(seqs):
    n = len(seqs)
    if n == 0:
        return b"\x00"
    assert n < 0x7F00
    head = bytes([n]) if n < 128 else bytes([(n >> 8) + 0x80, n & 255])
    out = W._Bits()
    ll, ml, of = _Coder(LL_DIST, LL_LOG, out), _Coder(ML_DIST, ML_LOG, out), _Coder(OF_DIST, OF_LOG, out)

    def extras(s):
        L, M, O = s
        out.put(L - LL_BASE[ll_code(L)], LL_BITS[ll_code(L)])
        out.put(M - ML_BASE[ml_code(M)], ML_BITS[ml_code(M)])
        out.put((O + 3) - (1 << of_code(O)), of_code(O))

    L, M, O = seqs[-1]
    ml.init(ml_code(M))
    of.init(of_code(O))
    ll.init(ll_code(L))
    extras(seqs[-1])
    for s in reversed(seqs[:-1]):
        L, M, O = s
        of.put(of_code(O))
        ml.put(ml_code(M))
        ll.put(ll_code(L))
        extras(s)
    ml.flush()
    of.flush()
    ll.flush()
    out.put(1, 1)
    return head + b"\x00" + out.bytes()


def literals_section(lits):
    n = len(lits)
    if n:
        cand = W.huf_block_candidate(lits)
    else:
        cand = None
    raw = (bytes([n << 3]) if n < 32 else ((n << 4) | 4).to_bytes(2, "little") if n < 4096 else ((n << 4) | 12).to_bytes(3, "little")) + lits
    if cand is not None and len(cand) - 1 < len(raw):
        return cand[:-1]
    return raw


def block_body(f, a, b, info=None):
    """the compressed block of bytes [a, b) of frame f whether it gains or not"""
    seqs, lits = parse(f, a, b)
    lit = literals_section(lits)
    if info is not None:
        info.update(seqs=seqs, lits=lits, lit_section=lit, huf=lit[0] & 3 == 2, tail=(b - a) - sum(s[0] + s[1] for s in seqs))
    return lit + sequences_section(seqs)


_frames = {}


def encode(frame, piece=PIECE, infos=None):
    """the zseq frame of `frame`; infos: a list that receives a dict per block (kind, and the parse of a non-RLE block)"""
    frame = bytes(frame)
    if infos is None and (frame, piece) in _frames:
        return _frames[frame, piece]
    out = [Z.MAGIC, bytes([Z.FHD]), struct.pack("<I", len(frame))]
    cuts = list(range(0, len(frame), piece)) or [0]
    for k, a in enumerate(cuts):
        b = min(len(frame), a + piece)
        last, n = k == len(cuts) - 1, b - a
        info = {}
        if n and frame.count(frame[a:a + 1], a, b) == n:
            out += [Z._block_header(last, 1, n), frame[a:a + 1]]
            info["kind"] = 1
        else:
            body = block_body(frame, a, b, info) if n else b"\x00\x00"
            if len(body) < n:
                out += [Z._block_header(last, 2, len(body)), body]
                info["kind"] = 2
            else:
                out += [Z._block_header(last, 0, n), frame[a:b]]
                info["kind"] = 0
            info["body"] = len(body)
        if infos is not None:
            infos.append(info)
    z = b"".join(out)
    _frames[frame, piece] = z
    return z


def wire(frame, piece=PIECE):
    """the frame rule of the sender: -> (payload as sent, compressed_size, flags)"""
    frame = bytes(frame)
    z = encode(frame, piece)
    if len(frame) <= Z.MIN_SIZE or Z.RATIO_DEN * len(z) >= Z.RATIO_NUM * len(frame):
        return frame, 0, 0
    return z, len(z), Z.FLAG_COMPRESSED


# ---- decoder, from the format ----------------------------------------------------------------------------------------------
def _decoding_table(dist, log):
    """-> [(symbol, bits to read, baseline of the next state)] per state"""
    size = 1 << log
    cells, high = [None] * size, size - 1
    for s, p in enumerate(dist):
        if p == -1:
            cells[high] = s
            high -= 1
    pos = 0
    for s, p in enumerate(dist):
        for _ in range(max(p, 0)):
            cells[pos] = s
            while True:
                pos = (pos + (size >> 1) + (size >> 3) + 3) & (size - 1)
                if pos <= high:
                    break
    Z._need(pos == 0 and None not in cells, "the spread does not fill the table")
    nxt = [abs(p) for p in dist]
    table = []
    for s in cells:
        x = nxt[s]
        nxt[s] += 1
        nb = log - (x.bit_length() - 1)
        table.append((s, nb, (x << nb) - size))
    return table


_TABLES = None


def _tables():
    global _TABLES
    if _TABLES is None:
        _TABLES = (_decoding_table(LL_DIST, LL_LOG), _decoding_table(OF_DIST, OF_LOG), _decoding_table(ML_DIST, ML_LOG))
    return _TABLES


def _decode_literals_section(body):
    """-> (literals, bytes of the section)"""
    Z._need(len(body) >= 1, "no literals section")
    kind = body[0] & 3
    if kind == 0:
        fmt = (body[0] >> 2) & 3
        if fmt in (0, 2):
            n, h = body[0] >> 3, 1
        elif fmt == 1:
            n, h = int.from_bytes(body[:2], "little") >> 4, 2
        else:
            n, h = int.from_bytes(body[:3], "little") >> 4, 3
        Z._need(h + n <= len(body), "raw literals beyond the block")
        return body[h:h + n], h + n
    Z._need(kind == 2, "RLE and treeless literals are outside the subset")
    fmt = (body[0] >> 2) & 3
    Z._need(fmt != 0, "single-stream literals are outside the subset")
    bits = {1: 10, 2: 14, 3: 18}[fmt]
    hlen = 2 + fmt
    csize = (int.from_bytes(body[:hlen], "little") >> 4) >> bits
    Z._need(hlen + csize <= len(body), "literals section beyond the block")
    return W._decode_literals(body[:hlen + csize] + b"\x00"), hlen + csize


def _decode_block(body, history):
    """a compressed block -> its bytes; history: the frame's bytes in front of it"""
    lits, at = _decode_literals_section(body)
    Z._need(at < len(body), "no sequences section")
    n = body[at]
    at += 1
    if n == 0:
        Z._need(at == len(body), "bytes behind a zero sequence count")
        return lits
    if n >= 128:
        Z._need(n < 255 and at < len(body), "the three-byte sequence count is outside the subset")
        n = ((n - 128) << 8) + body[at]
        at += 1
    Z._need(at < len(body) and body[at] == 0, "only Predefined_Mode tables are in the subset")
    at += 1
    stream = body[at:]
    Z._need(len(stream) >= 1 and stream[-1] != 0, "bitstream without an end mark")
    v = int.from_bytes(stream, "little")
    left = v.bit_length() - 1

    def take(nb):
        nonlocal left
        left -= nb
        Z._need(left >= 0, "the bitstream runs out")
        return (v >> left) & ((1 << nb) - 1)

    llt, oft, mlt = _tables()
    sl, so, sm = take(LL_LOG), take(OF_LOG), take(ML_LOG)
    out = bytearray(history)
    base = len(out)
    lit_at = 0
    for k in range(n):
        oc, lc, mc = oft[so][0], llt[sl][0], mlt[sm][0]
        Z._need(oc >= 2, "repeat offsets are outside the subset")
        value = (1 << oc) + take(oc)
        ml = ML_BASE[mc] + take(ML_BITS[mc])
        ll = LL_BASE[lc] + take(LL_BITS[lc])
        off = value - 3
        Z._need(off >= 1, "repeat offsets are outside the subset")
        if k + 1 < n:
            sl = llt[sl][2] + take(llt[sl][1])
            sm = mlt[sm][2] + take(mlt[sm][1])
            so = oft[so][2] + take(oft[so][1])
        Z._need(lit_at + ll <= len(lits), "more literals than the section holds")
        out += lits[lit_at:lit_at + ll]
        lit_at += ll
        Z._need(off <= len(out), "offset beyond the frame's start")
        for _ in range(ml):
            out.append(out[-off])
    Z._need(left == 0, "bits left over")
    out += lits[lit_at:]
    return bytes(out[base:])


def decode(payload, piece=PIECE):
    payload = bytes(payload)
    Z._need(payload[:4] == Z.MAGIC and len(payload) >= 9 and payload[4] == Z.FHD, "frame header")
    size = struct.unpack("<I", payload[5:9])[0]
    at, out, last = 9, bytearray(), False
    while not last:
        Z._need(at + 3 <= len(payload), "block header cut short")
        h = int.from_bytes(payload[at:at + 3], "little")
        at += 3
        last, kind, bsize = bool(h & 1), (h >> 1) & 3, h >> 3
        Z._need(kind != 3, "reserved block type")
        take = 1 if kind == 1 else bsize
        Z._need(at + take <= len(payload) and bsize <= piece, "block beyond the frame")
        body = payload[at:at + take]
        at += take
        part = body if kind == 0 else body * bsize if kind == 1 else _decode_block(body, bytes(out))
        Z._need(len(part) <= piece, "block regenerates more than a piece")
        out += part
    Z._need(at == len(payload), "bytes behind the last block")
    Z._need(len(out) == size, "Frame_Content_Size")
    return bytes(out)


def roundtrip(frame, piece=PIECE):
    """encode -> decode and encode -> libzstd give the frame back; -> the zseq frame"""
    frame = bytes(frame)
    z = encode(frame, piece)
    assert decode(z, piece) == frame
    if Z.libzstd() is not None:
        assert Z.zstd_decompress(z, len(frame)) == frame
    return z


def device_tables():
    """the three coding tables as csrc/zseq_kernels.hpp holds them: words of stateTable, deltaNbBits, deltaFindState for LL, ML, OF"""
    out = []
    for dist, log in ((LL_DIST, LL_LOG), (ML_DIST, ML_LOG), (OF_DIST, OF_LOG)):
        st, dnb, dfs = coding_table(dist, log)
        out.append((st, dnb, dfs))
    return out
