"""The wide zhuf form restated in Python: the zhuf frame of tests/zhuf_ref.py over all 256 byte values, the
Huffman tree in zstd's direct form where the largest symbol is at most 128 and in its FSE-compressed form above that.
encode() / wire() are what the device must produce byte for byte; decode() is a decoder of exactly this subset whose FSE
part (table description, decoding table, two-state bitstream) is written from the format and not by inverting the encoder,
direct-form blocks go to zhuf_ref's; libzstd's ZSTD_decompress is the judge (zhuf_ref.zstd_decompress).  TESTS ONLY."""
import struct

import zhuf_ref as Z

PIECE = Z.PIECE
MAX_BITS = Z.MAX_BITS
ACC_LOG = 6  # Accuracy_Log of the weights' FSE table, always
CELLS = 1 << ACC_LOG
MAX_TREE = 127  # bytes of table description + bitstream a tree may take (its header byte says < 128)


# ---- code lengths over 256 symbols ---------------------------------------------------------------------------------------
def code_lengths(hist):
    """zhuf_ref.code_lengths' algorithm over 256 counts -> 256 lengths"""
    leaves = sorted((c, s) for s, c in enumerate(hist) if c)
    m = len(leaves)
    assert m >= 2 and len(hist) == 256
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
    if max(lens) > MAX_BITS:
        lens = [min(d, MAX_BITS) for d in lens]
        full = 1 << MAX_BITS
        kraft = sum(full >> d for d in lens)
        while kraft > full:
            best = -1
            for j in range(m):
                if lens[j] < MAX_BITS and (best < 0 or lens[j] > lens[best]):
                    best = j
            lens[best] += 1
            kraft -= full >> lens[best]
        while kraft < full:
            for j in range(m - 1, -1, -1):
                if (full >> lens[j]) <= full - kraft:
                    kraft += full >> lens[j]
                    lens[j] -= 1
                    break
    out = [0] * 256
    for (_, s), d in zip(leaves, lens):
        out[s] = d
    return out


# ---- the FSE form of the weights: encoder ---------------------------------------------------------------------------------
def normalise(weights, steps=None):
    """the counts of the weight values among `weights`, scaled to a sum of 64 -> n[12]; steps receives how often the rule
    decremented ("dec") and how much it added ("add")"""
    top = len(weights)
    c = [0] * 12
    for w in weights:
        c[w] += 1
    n = [max(1, CELLS * c[w] // top) if c[w] else 0 for w in range(12)]

    def largest():
        return max(range(12), key=lambda w: (n[w], -w))  # ties: the smallest w

    dec = 0
    while sum(n) > CELLS:
        n[largest()] -= 1
        dec += 1
    add = CELLS - sum(n)
    if add:
        n[largest()] += add
    if steps is not None:
        steps["dec"], steps["add"] = dec, add
    assert sum(n) == CELLS and all(n[w] >= 1 for w in range(12) if c[w])
    return n


class _Bits:
    """an LSB-first forward bit stream"""

    def __init__(self):
        self.acc, self.pos = 0, 0

    def put(self, v, nb):
        assert 0 <= v < (1 << nb) or nb == 0
        self.acc |= v << self.pos
        self.pos += nb

    def bytes(self):
        return self.acc.to_bytes((self.pos + 7) // 8, "little")


def describe(n, runs=None):
    """the FSE table description of n[12] (sum 64); runs receives every r of a zero run (further zeros behind a zero)"""
    out = _Bits()
    out.put(ACC_LOG - 5, 4)
    remaining, threshold, nb = CELLS + 1, CELLS, ACC_LOG + 1
    w = 0
    while remaining > 1:
        mx = 2 * threshold - 1 - remaining
        v = n[w] + 1
        remaining -= n[w]
        if v >= threshold:
            v += mx
        out.put(v, nb - 1 if v < mx else nb)
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
        if n[w] == 0:
            nxt = w + 1
            while n[nxt] == 0:
                nxt += 1
            r = nxt - w - 1
            if runs is not None:
                runs.append(r)
            for _ in range(r // 3):
                out.put(3, 2)
            out.put(r % 3, 2)
            w = nxt
        else:
            w += 1
    return out.bytes()


def coding_table(n):
    """-> (stateTable[64], deltaNbBits[12], deltaFindState[12])"""
    cells, pos = [0] * CELLS, 0
    for w in range(12):
        for _ in range(n[w]):
            cells[pos] = w
            pos = (pos + 43) & (CELLS - 1)
    assert pos == 0
    cumul, total = [0] * 12, 0
    for w in range(12):
        cumul[w] = total
        total += n[w]
    state = [0] * CELLS
    for u in range(CELLS):
        state[cumul[cells[u]]] = CELLS + u
        cumul[cells[u]] += 1
    dnb, dfs, total = [0] * 12, [0] * 12, 0
    for w in range(12):
        if n[w] == 1:
            dnb[w], dfs[w] = (ACC_LOG << 16) - CELLS, total - 1
        elif n[w] > 1:
            b = ACC_LOG - ((n[w] - 1).bit_length() - 1)
            dnb[w], dfs[w] = (b << 16) - (n[w] << b), total - n[w]
        total += n[w]
    return state, dnb, dfs


def fse_bitstream(x, n, info=None):
    """the two-state bitstream of the weights x under n[12]; info receives "bits": the bit count before the end mark"""
    state, dnb, dfs = coding_table(n)
    out = _Bits()

    def init(w):
        nb = (dnb[w] + 32768) >> 16
        return state[(((nb << 16) - dnb[w]) >> nb) + dfs[w]]

    def put(s, w):
        nb = (s + dnb[w]) >> 16
        out.put(s & ((1 << nb) - 1), nb)
        return state[(s >> nb) + dfs[w]]

    k = len(x)
    assert k >= 2
    if k & 1:
        s1, s2 = init(x[k - 1]), init(x[k - 2])
        s1 = put(s1, x[k - 3])
        at = k - 3
    else:
        s2, s1 = init(x[k - 1]), init(x[k - 2])
        at = k - 2
    while at > 0:  # an even count remains: x[0] goes through s1
        s2 = put(s2, x[at - 1])
        s1 = put(s1, x[at - 2])
        at -= 2
    out.put(s2 - CELLS, ACC_LOG)
    out.put(s1 - CELLS, ACC_LOG)
    if info is not None:
        info["bits"] = out.pos
    out.put(1, 1)
    return out.bytes()


def fse_tree(weights, info=None):
    """header byte + description + bitstream of the weights of symbols 0 .. top - 1, or None where the form does not apply
    (one weight value only; more than 127 bytes).  info receives "dec", "add", "runs", "bits", "tree" (bytes behind the
    header byte, also where None is returned for the size)."""
    info = {} if info is None else info
    if len(set(weights)) == 1:
        return None
    n = normalise(weights, info)
    info["runs"] = []
    body = describe(n, info["runs"]) + fse_bitstream(weights, n, info)
    info["tree"] = len(body)
    if len(body) > MAX_TREE:
        return None
    return bytes([len(body)]) + body


# ---- encoder ------------------------------------------------------------------------------------------------------------
def huf_block_candidate(piece, tables=None, info=None):
    """the compressed block of a piece whether it gains or not; None where no tree is sent at all"""
    n = len(piece)
    if n < Z.MIN_HUF_PIECE or piece.count(piece[0]) == n:
        return None
    hist = [0] * 256
    for b in piece:
        hist[b] += 1
    lens = code_lengths(hist)
    Z.check_table(lens)
    codes, max_bits = Z.canonical_codes(lens)
    top = max(piece)
    weights = [(max_bits + 1 - lens[s]) if lens[s] else 0 for s in range(top)]
    if top <= 128:
        if info is not None:
            info["form"] = "direct"
        padded = weights + [0] * (len(weights) & 1)
        tree = bytes([127 + top]) + bytes((padded[k] << 4) | padded[k + 1] for k in range(0, len(padded), 2))
    else:
        if info is not None:
            info["form"] = "fse"
        tree = fse_tree(weights, info)
        if tree is None:
            return None
    if tables is not None:
        tables.append(lens)
    seg = (n + 3) // 4
    streams = [Z._stream(piece[k * seg:min(n, (k + 1) * seg)], codes, lens) for k in range(4)]
    csize = len(tree) + 6 + sum(len(s) for s in streams)
    for fmt, bits in ((1, 10), (2, 14), (3, 18)):
        if n < (1 << bits) and csize < (1 << bits):
            break
    head = (2 | (fmt << 2) | (n << 4) | (csize << (4 + bits))).to_bytes(2 + fmt, "little")
    return head + tree + struct.pack("<HHH", *(len(s) for s in streams[:3])) + b"".join(streams) + b"\x00"


def huf_block_body(piece, tables=None, info=None):
    t = []
    body = huf_block_candidate(piece, t, info)
    if body is None or len(body) >= len(piece):
        return None
    if tables is not None:
        tables += t
    return body


_bodies = {}


def _body_of(part, tables):
    if part not in _bodies:
        t = []
        _bodies[part] = (huf_block_body(part, t), t[0] if t else None)
    body, lens = _bodies[part]
    if tables is not None and lens is not None:
        tables.append(lens)
    return body


def encode(frame, tables=None, piece=PIECE):
    """the wide zhuf frame of `frame`; tables: a list that receives the 256 code lengths of every coded piece"""
    frame = bytes(frame)
    out = [Z.MAGIC, bytes([Z.FHD]), struct.pack("<I", len(frame))]
    pieces = [frame[k:k + piece] for k in range(0, len(frame), piece)] or [b""]
    for k, part in enumerate(pieces):
        last = k == len(pieces) - 1
        n = len(part)
        if n and part.count(part[0]) == n:
            out += [Z._block_header(last, 1, n), part[:1]]
            continue
        body = _body_of(part, tables)
        if body is None:
            out += [Z._block_header(last, 0, n), part]
        else:
            out += [Z._block_header(last, 2, len(body)), body]
    return b"".join(out)


def wire(frame, piece=PIECE):
    """the frame rule of the sender: -> (payload as sent, compressed_size, flags)"""
    frame = bytes(frame)
    z = encode(frame, piece=piece)
    if len(frame) <= Z.MIN_SIZE or Z.RATIO_DEN * len(z) >= Z.RATIO_NUM * len(frame):
        return frame, 0, 0
    return z, len(z), Z.FLAG_COMPRESSED


# ---- decoder: the FSE form, from the format ---------------------------------------------------------------------------------
def _read_distribution(data):
    """FSE table description -> (probabilities, accuracy log, bytes used)"""
    v = int.from_bytes(data, "little")
    at = 0

    def take(nb):
        nonlocal at
        Z._need(at + nb <= 8 * len(data), "table description cut short")
        r = (v >> at) & ((1 << nb) - 1)
        at += nb
        return r

    log = take(4) + 5
    Z._need(log <= 6, "Accuracy_Log above 6 in a weight table")
    left, probs = 1 << log, []
    while left > 0:
        Z._need(len(probs) < 12, "more than 12 weight values")
        # a value in 0 .. left + 1: the low ones in one bit less
        nb = (left + 1).bit_length()
        low = take(nb - 1)
        cut = (1 << nb) - 1 - (left + 1)
        if low < cut:
            val = low
        else:
            val = low + (take(1) << (nb - 1))
            if val >= 1 << (nb - 1):
                val -= cut
        Z._need(val != 0, '"less than 1" probabilities are outside the subset')
        p = val - 1
        probs.append(p)
        left -= p
        Z._need(left >= 0, "probabilities above the table size")
        if p == 0:
            while True:
                rep = take(2)
                probs += [0] * rep
                if rep != 3:
                    break
    return probs, log, (at + 7) // 8


def _decoding_table(probs, log):
    size = 1 << log
    cells, pos = [None] * size, 0
    for s, p in enumerate(probs):
        for _ in range(p):
            cells[pos] = s
            pos = (pos + (size >> 1) + (size >> 3) + 3) & (size - 1)
    Z._need(pos == 0 and None not in cells, "the spread does not fill the table")
    nxt = list(probs)
    table = []
    for s in cells:
        x = nxt[s]
        nxt[s] += 1
        nb = log - (x.bit_length() - 1)
        table.append((s, nb, (x << nb) - size))
    return table


def _fse_weights(data):
    """table description + bitstream -> the weights"""
    probs, log, used = _read_distribution(data)
    table = _decoding_table(probs, log)
    stream = data[used:]
    Z._need(len(stream) >= 1 and stream[-1] != 0, "bitstream without an end mark")
    v = int.from_bytes(stream, "little")
    left = v.bit_length() - 1  # bits in front of the end mark, read from the top down

    def take(nb):
        nonlocal left
        left -= nb
        if left >= 0:
            return (v >> left) & ((1 << nb) - 1)
        return ((v << -left) & ((1 << nb) - 1)) if nb + left > 0 else 0  # past the start: zeros

    s1 = take(log)
    s2 = take(log)
    Z._need(left >= 0, "bitstream shorter than its two states")
    out = []
    while True:
        sym, nb, base = table[s1]
        out.append(sym)
        s1 = base + take(nb)
        if left < 0:
            out.append(table[s2][0])
            break
        sym, nb, base = table[s2]
        out.append(sym)
        s2 = base + take(nb)
        if left < 0:
            out.append(table[s1][0])
            break
        Z._need(len(out) <= 255, "more than 255 weights")
    return out


def _decode_literals(body):
    Z._need(len(body) >= 3 and body[0] & 3 == 2, "only Compressed_Literals_Block is in the subset")
    fmt = (body[0] >> 2) & 3
    Z._need(fmt != 0, "single-stream literals are outside the subset")
    bits = {1: 10, 2: 14, 3: 18}[fmt]
    hlen = 2 + fmt
    v = int.from_bytes(body[:hlen], "little") >> 4
    regen, csize = v & ((1 << bits) - 1), v >> bits
    Z._need(hlen + csize + 1 == len(body) and body[-1] == 0, "literals section + a zero sequence count must fill the block")
    sec = body[hlen:hlen + csize]
    Z._need(len(sec) >= 1, "no tree")
    if sec[0] >= 128:
        return Z._decode_literals(body)
    h = sec[0]
    Z._need(h >= 2 and len(sec) >= 1 + h + 6, "tree description cut short")
    weights = _fse_weights(sec[1:1 + h])
    Z._need(len(weights) <= 255 and all(w <= MAX_BITS for w in weights), "weights")
    total = sum((1 << (w - 1)) for w in weights if w)
    Z._need(total > 0, "no weights")
    max_bits = total.bit_length()
    Z._need(max_bits <= MAX_BITS, "table log above 11")
    rest = (1 << max_bits) - total
    Z._need(rest & (rest - 1) == 0, "the implied weight is no power of two")
    weights.append(rest.bit_length())
    table = []
    for w in range(1, max_bits + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                table += [(s, max_bits + 1 - w)] * (1 << (w - 1))
    Z._need(len(table) == 1 << max_bits, "incomplete code")
    at = 1 + h
    sizes = list(struct.unpack("<HHH", sec[at:at + 6]))
    at += 6
    Z._need(len(sec) - at - sum(sizes) >= 1, "jump table beyond the section")
    sizes.append(len(sec) - at - sum(sizes))
    seg = (regen + 3) // 4
    counts = [seg, seg, seg, regen - 3 * seg]
    Z._need(counts[3] >= 1, "an empty fourth stream")
    out = b""
    for size, cnt in zip(sizes, counts):
        out += Z._decode_stream(sec[at:at + size], cnt, table, max_bits)
        at += size
    return out


_literals = {}


def decode(payload, piece=PIECE):
    payload = bytes(payload)
    Z._need(payload[:4] == Z.MAGIC and len(payload) >= 9 and payload[4] == Z.FHD, "frame header")
    size = struct.unpack("<I", payload[5:9])[0]
    at, out, last = 9, [], False
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
        if kind == 2:
            if body not in _literals:
                _literals[body] = _decode_literals(body)
            out.append(_literals[body])
        else:
            out.append(body if kind == 0 else body * bsize)
        Z._need(len(out[-1]) <= piece, "block regenerates more than a piece")
    Z._need(at == len(payload), "bytes behind the last block")
    res = b"".join(out)
    Z._need(len(res) == size, "Frame_Content_Size")
    return res


def roundtrip(frame, piece=PIECE):
    """encode -> decode and encode -> libzstd give the frame back; -> the wide zhuf frame"""
    frame = bytes(frame)
    z = encode(frame, piece=piece)
    assert decode(z, piece) == frame
    if Z.libzstd() is not None:
        assert Z.zstd_decompress(z, len(frame)) == frame
    return z
