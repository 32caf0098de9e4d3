"""The "zhuf" wire form restated in Python: a zstd frame built only from raw, RLE and Huffman-literals
blocks with zero sequences.  encode() is what the device must produce byte for byte (the length algorithm included);
decode() is a decoder of exactly this subset, written from the format and not by inverting encode(); zstd_decompress() is
libzstd's own decoder where libzstd.so.1 loads.  encode(), decode() and wire() take the piece size (the product's by default:
the tests' second emulator library has a smaller one); a piece of 1 KB or more is coded once and its block decoded once,
however many frames hold it.  TESTS ONLY."""
import ctypes as C
import struct

PIECE = 131072
MAX_BITS = 11
MAGIC = b"\x28\xb5\x2f\xfd"
FHD = 0xA0  # Single_Segment, 4-byte Frame_Content_Size, no checksum, no dictionary
MIN_HUF_PIECE = 17  # no compressed block is below 16 bytes (3 + 2 + 6 + 4 + 1): shorter pieces never gain
FLAG_COMPRESSED = 0x02
RATIO_NUM, RATIO_DEN, MIN_SIZE = 4, 5, 1024  # COMPRESSION_RATIO_THRESHOLD 0.8, COMPRESSION_MIN_SIZE


# ---- code lengths ------------------------------------------------------------------------------------------------------
def code_lengths(hist, steps=None):
    """hist: 129 counts (symbols 0..128), at least two of them non-zero -> 129 code lengths (0: symbol absent), every
    length <= MAX_BITS, Kraft sum exactly 1.  Integer only, deterministic.  steps: a dict that receives how often the
    limiter demoted and promoted ("demoted", "promoted": 0 where the tree was no deeper than MAX_BITS)."""
    leaves = sorted((c, s) for s, c in enumerate(hist) if c)  # count ascending, then symbol ascending
    m = len(leaves)
    assert m >= 2
    # two-queue merge: leaves in sorted order, internal nodes in creation order; on a tie the leaf goes first
    weight = [c for c, _ in leaves]
    parent = [0] * (2 * m - 1)
    li, ii = 0, m
    for k in range(m, 2 * m - 1):
        picked = []
        for _ in range(2):
            if li < m and (ii >= k or weight[li] <= weight[ii]):
                picked.append(li)
                li += 1
            else:
                picked.append(ii)
                ii += 1
        weight.append(weight[picked[0]] + weight[picked[1]])
        parent[picked[0]] = parent[picked[1]] = k
    depth = [0] * (2 * m - 1)
    for k in range(2 * m - 3, -1, -1):
        depth[k] = depth[parent[k]] + 1
    lens = depth[:m]
    demoted = promoted = 0
    if max(lens) > MAX_BITS:
        lens = [min(d, MAX_BITS) for d in lens]
        full = 1 << MAX_BITS
        kraft = sum(full >> d for d in lens)
        while kraft > full:  # demote: the longest code below the limit, the least frequent of those
            best = -1
            for j in range(m):
                if lens[j] < MAX_BITS and (best < 0 or lens[j] > lens[best]):
                    best = j
            lens[best] += 1
            kraft -= full >> lens[best]
            demoted += 1
        while kraft < full:  # promote: the most frequent symbol whose step fits what is missing
            for j in range(m - 1, -1, -1):
                if (full >> lens[j]) <= full - kraft:
                    kraft += full >> lens[j]
                    lens[j] -= 1
                    promoted += 1
                    break
    if steps is not None:
        steps["demoted"], steps["promoted"] = demoted, promoted
    out = [0] * 129
    for (_, s), d in zip(leaves, lens):
        out[s] = d
    return out


def canonical_codes(lens):
    """-> (codes[129], maxBits): weight ascending (longest first), then value ascending; the first gets 0, +1 within a
    weight, (code + count) >> 1 on the way up."""
    max_bits = max(lens)
    count = [0] * (max_bits + 2)
    for d in lens:
        if d:
            count[d] += 1
    start = [0] * (max_bits + 2)
    code = 0
    for d in range(max_bits, 0, -1):
        start[d] = code
        code = (code + count[d]) >> 1
    codes = [0] * len(lens)
    nxt = list(start)
    for s, d in enumerate(lens):
        if d:
            codes[s] = nxt[d]
            nxt[d] += 1
    return codes, max_bits


def check_table(lens):
    """the pins of the issue: maxBits <= 11, Kraft sum exactly 1"""
    assert max(lens) <= MAX_BITS
    assert sum((1 << MAX_BITS) >> d for d in lens if d) == 1 << MAX_BITS


# ---- encoder -----------------------------------------------------------------------------------------------------------
def _stream(sym, codes, lens):
    acc, pos = 0, 0
    for b in reversed(sym):  # last symbol first, LSB-first accumulator
        acc |= codes[b] << pos
        pos += lens[b]
    acc |= 1 << pos  # the end mark
    return acc.to_bytes(pos // 8 + 1, "little")


def _block_header(last, kind, size):
    return struct.pack("<I", (1 if last else 0) | (kind << 1) | (size << 3))[:3]


def huf_block_body(piece, tables=None):
    """the compressed block of a piece (literals section + the zero sequence count), or None when the piece is not coded"""
    body = huf_block_candidate(piece, tables)
    return body if body is not None and len(body) < len(piece) else None


def huf_block_candidate(piece, tables=None):
    """the compressed block of a piece whether it gains or not; None where no table is built at all"""
    n = len(piece)
    if n < MIN_HUF_PIECE or max(piece) > 0x80 or piece.count(piece[0]) == n:
        return None
    hist = [0] * 129
    for b in piece:
        hist[b] += 1
    lens = code_lengths(hist)
    check_table(lens)
    if tables is not None:
        tables.append(lens)
    codes, max_bits = canonical_codes(lens)
    top = max(piece)  # S: its weight is implied
    weights = [(max_bits + 1 - lens[s]) if lens[s] else 0 for s in range(top)]
    if len(weights) & 1:
        weights.append(0)
    tree = bytes([127 + top]) + bytes((weights[k] << 4) | weights[k + 1] for k in range(0, len(weights), 2))
    seg = (n + 3) // 4
    streams = [_stream(piece[k * seg:min(n, (k + 1) * seg)], codes, lens) for k in range(4)]
    csize = len(tree) + 6 + sum(len(s) for s in streams)
    for fmt, bits in ((1, 10), (2, 14), (3, 18)):
        if n < (1 << bits) and csize < (1 << bits):
            break
    head = (2 | (fmt << 2) | (n << 4) | (csize << (4 + bits))).to_bytes(2 + fmt, "little")
    return head + tree + struct.pack("<HHH", *(len(s) for s in streams[:3])) + b"".join(streams) + b"\x00"


_bodies = {}  # piece -> (its compressed block or None, its code lengths or None): long pieces are coded once


def _body_of(piece, tables):
    if len(piece) < 1024:
        return huf_block_body(piece, tables)
    if piece not in _bodies:
        t = []
        body = huf_block_body(piece, t)
        _bodies[piece] = (body, t[0] if t else None)
    body, lens = _bodies[piece]
    if tables is not None and lens is not None:
        tables.append(lens)
    return body


def encode(frame, tables=None, piece=PIECE):
    """the zhuf frame of `frame` (any length), one block per `piece` bytes; tables: a list that receives the code lengths
    of every coded piece"""
    frame = bytes(frame)
    out = [MAGIC, bytes([FHD]), struct.pack("<I", len(frame))]
    pieces = [frame[k:k + piece] for k in range(0, len(frame), piece)] or [b""]
    for k, part in enumerate(pieces):
        last = k == len(pieces) - 1
        n = len(part)
        if n and part.count(part[0]) == n:
            out += [_block_header(last, 1, n), part[:1]]
            continue
        body = _body_of(part, tables)
        if body is None:
            out += [_block_header(last, 0, n), part]
        else:
            out += [_block_header(last, 2, len(body)), body]
    return b"".join(out)


def blocks(z):
    """[(type, size, offset of the block's header in the frame)] of a zhuf frame"""
    at, out, last = 9, [], False
    while not last:
        h = int.from_bytes(z[at:at + 3], "little")
        last, kind, size = bool(h & 1), (h >> 1) & 3, h >> 3
        out.append((kind, size, at))
        at += 3 + (1 if kind == 1 else size)
    assert at == len(z)
    return out


def wire(frame, piece=PIECE):
    """the frame rule of the sender: -> (payload as sent, compressed_size, flags)"""
    frame = bytes(frame)
    z = encode(frame, piece=piece)
    if len(frame) <= MIN_SIZE or RATIO_DEN * len(z) >= RATIO_NUM * len(frame):
        return frame, 0, 0
    return z, len(z), FLAG_COMPRESSED


def packet_header(width, height, original, compressed, checksum, flags):
    """ascii_frame_packet_t, network byte order"""
    return struct.pack(">6I", width, height, original, compressed, checksum, flags)


# ---- decoder of the subset ---------------------------------------------------------------------------------------------
class FormatError(Exception):
    pass


def _need(cond, what):
    if not cond:
        raise FormatError(what)


def _decode_stream(data, n_sym, table, max_bits):
    """one Huffman bitstream read backwards from its end mark; table: 2^max_bits entries of (symbol, length)"""
    _need(len(data) >= 1 and data[-1] != 0, "stream without an end mark")
    digits = bin(int.from_bytes(data, "little"))[3:]  # behind "0b" and the end mark: the codes, the first symbol's first
    pos = len(digits)  # bits left
    digits += "0" * max_bits
    at = 0
    out = bytearray()
    for _ in range(n_sym):
        sym, ln = table[int(digits[at:at + max_bits], 2)]
        _need(ln <= pos, "stream runs out of bits")
        pos -= ln
        at += ln
        out.append(sym)
    _need(pos == 0, "stream has bits left over")
    return bytes(out)


def _decode_literals(body):
    _need(len(body) >= 3, "literals header cut short")
    _need(body[0] & 3 == 2, "only Compressed_Literals_Block is in the subset")
    fmt = (body[0] >> 2) & 3
    _need(fmt != 0, "single-stream literals are outside the subset")
    bits = {1: 10, 2: 14, 3: 18}[fmt]
    hlen = 2 + fmt
    v = int.from_bytes(body[:hlen], "little") >> 4
    regen, csize = v & ((1 << bits) - 1), v >> bits
    _need(regen >= 6, "four streams need at least six literals")
    _need(hlen + csize + 1 == len(body) and body[-1] == 0, "literals section + a zero sequence count must fill the block")
    sec = body[hlen:hlen + csize]
    _need(len(sec) >= 1 and sec[0] >= 128, "only the direct weight form is in the subset")
    listed = sec[0] - 127
    nbytes = (listed + 1) // 2
    _need(len(sec) >= 1 + nbytes + 6, "tree description cut short")
    weights = []
    for k in range(listed):
        byte = sec[1 + k // 2]
        weights.append(byte >> 4 if k % 2 == 0 else byte & 15)
    total = sum((1 << (w - 1)) for w in weights if w)
    _need(total > 0, "no weights")
    max_bits = total.bit_length()
    _need(max_bits <= MAX_BITS, "table log above 11")
    rest = (1 << max_bits) - total
    _need(rest & (rest - 1) == 0, "the implied weight is no power of two")
    weights.append(rest.bit_length())
    table = []
    for w in range(1, max_bits + 1):  # weight ascending, value ascending: consecutive ranges of the decoding table
        for s, ws in enumerate(weights):
            if ws == w:
                table += [(s, max_bits + 1 - w)] * (1 << (w - 1))
    _need(len(table) == 1 << max_bits, "incomplete code")
    at = 1 + nbytes
    sizes = list(struct.unpack("<HHH", sec[at:at + 6]))
    at += 6
    _need(sum(sizes) < len(sec) - at + 1 and len(sec) - at - sum(sizes) >= 1, "jump table beyond the section")
    sizes.append(len(sec) - at - sum(sizes))
    seg = (regen + 3) // 4
    counts = [seg, seg, seg, regen - 3 * seg]
    _need(counts[3] >= 1, "an empty fourth stream")
    out = b""
    for size, cnt in zip(sizes, counts):
        out += _decode_stream(sec[at:at + size], cnt, table, max_bits)
        at += size
    return out


_literals = {}  # compressed block -> its literals: long blocks are decoded once


def _literals_of(body):
    if len(body) < 1024:
        return _decode_literals(body)
    if body not in _literals:
        _literals[body] = _decode_literals(body)
    return _literals[body]


def decode(payload, piece=PIECE):
    payload = bytes(payload)
    _need(payload[:4] == MAGIC and len(payload) >= 9 and payload[4] == FHD, "frame header")
    size = struct.unpack("<I", payload[5:9])[0]
    at, out, last = 9, [], False
    while not last:
        _need(at + 3 <= len(payload), "block header cut short")
        h = int.from_bytes(payload[at:at + 3], "little")
        at += 3
        last, kind, bsize = bool(h & 1), (h >> 1) & 3, h >> 3
        _need(kind != 3, "reserved block type")
        take = 1 if kind == 1 else bsize
        _need(at + take <= len(payload) and bsize <= piece, "block beyond the frame")
        body = payload[at:at + take]
        at += take
        out.append(body if kind == 0 else body * bsize if kind == 1 else _literals_of(body))
        _need(len(out[-1]) <= piece, "block regenerates more than a piece")
    _need(at == len(payload), "bytes behind the last block")
    res = b"".join(out)
    _need(len(res) == size, "Frame_Content_Size")
    return res


# ---- libzstd -----------------------------------------------------------------------------------------------------------
_zstd = False


def libzstd():
    """libzstd.so.1, or None where it does not load"""
    global _zstd
    if _zstd is False:
        try:
            L = C.CDLL("libzstd.so.1")
            L.ZSTD_decompress.restype = C.c_size_t
            L.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
            L.ZSTD_isError.restype = C.c_uint
            L.ZSTD_isError.argtypes = [C.c_size_t]
            L.ZSTD_getErrorName.restype = C.c_char_p
            L.ZSTD_getErrorName.argtypes = [C.c_size_t]
            L.ZSTD_compress.restype = C.c_size_t
            L.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int]
            L.ZSTD_compressBound.restype = C.c_size_t
            L.ZSTD_compressBound.argtypes = [C.c_size_t]
            _zstd = L
        except OSError:
            _zstd = None
    return _zstd


def zstd_decompress(payload, size):
    """ZSTD_decompress of a frame whose content is `size` bytes; raises FormatError with libzstd's message"""
    L = libzstd()
    buf = C.create_string_buffer(max(size, 1))
    r = L.ZSTD_decompress(buf, size, bytes(payload), len(payload))
    if L.ZSTD_isError(r):
        raise FormatError("libzstd: " + L.ZSTD_getErrorName(r).decode())
    return buf.raw[:r]


def zstd_compress(data, level=1):
    L = libzstd()
    cap = L.ZSTD_compressBound(len(data))
    buf = C.create_string_buffer(cap)
    r = L.ZSTD_compress(buf, cap, bytes(data), len(data), level)
    assert not L.ZSTD_isError(r)
    return buf.raw[:r]


def roundtrip(frame):
    """encode -> decode and encode -> libzstd (where it loads) give the frame back; -> the zhuf frame"""
    frame = bytes(frame)
    z = encode(frame)
    assert decode(z) == frame
    if libzstd() is not None:
        assert zstd_decompress(z, len(frame)) == frame
    return z
