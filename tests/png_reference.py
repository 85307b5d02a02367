"""What the PNG encoder (csrc/png_encode.hip) is checked against, restated in numpy / plain Python from RFC 2083 (PNG) and RFC 1951
(deflate): the scanline filter rule, a chunk parser, the cost of an optimal Huffman code, and a bit reader that walks a deflate
stream of stored and literal-only dynamic blocks."""
import heapq
import struct
import zlib

import numpy as np

S = 16384                      # CLSLAM_PNG_BLOCK: filtered bytes per deflate block
HEADER_BITS = 17 + 19 * 3 + 258 * 4
CLC_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
SIGNATURE = b'\x89PNG\r\n\x1a\n'


# ---- filter ----------------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(image, fixed=None):
    """image (H,W) or (H,W,3) uint8 -> (filtered stream (H * (1 + W * bpp),) uint8, the H filter types).  fixed=None: per row the
    type with the smallest sum of min(b, 256 - b) over the filtered bytes, ties to the lowest type."""
    image = np.asarray(image)
    H, W = image.shape[:2]
    bpp = 1 if image.ndim == 2 else image.shape[2]
    rows = image.reshape(H, W * bpp).astype(np.int64)
    out = np.zeros((H, 1 + W * bpp), np.uint8)
    types = []
    for y in range(H):
        x = rows[y]
        a = np.concatenate([np.zeros(bpp, np.int64), x[:-bpp]]) if W * bpp > bpp else np.zeros_like(x)
        b = rows[y - 1] if y else np.zeros_like(x)
        c = (np.concatenate([np.zeros(bpp, np.int64), b[:-bpp]]) if W * bpp > bpp else np.zeros_like(x)) if y else np.zeros_like(x)
        cand = [x, x - a, x - b, x - (a + b) // 2, x - _paeth(a, b, c)]
        cand = [v & 255 for v in cand]
        if fixed is None:
            scores = [int(np.minimum(v, 256 - v).sum()) for v in cand]
            t = scores.index(min(scores))                               # the first of equals: the lowest type
        else:
            t = fixed
        types.append(t)
        out[y, 0] = t
        out[y, 1:] = cand[t]
    return out.reshape(-1), types


# ---- container -------------------------------------------------------------------------------------------------------------
def chunks(data: bytes):
    """-> [(type, data, stored crc)]; asserts the signature and that the chunks fill the file exactly"""
    assert data[:8] == SIGNATURE
    out, p = [], 8
    while p < len(data):
        n, = struct.unpack('>I', data[p:p + 4])
        typ, body = data[p + 4:p + 8], data[p + 8:p + 8 + n]
        crc, = struct.unpack('>I', data[p + 8 + n:p + 12 + n])
        out.append((typ, body, crc))
        p += 12 + n
    assert p == len(data)
    return out


def check_file(data: bytes, filtered: bytes, h: int, w: int, channels: int) -> bytes:
    """every container check of one file; -> the zlib stream (the concatenated IDAT payload)"""
    cs = chunks(data)
    assert [c[0] for c in cs][0] == b'IHDR' and cs[-1][0] == b'IEND' and all(c[0] == b'IDAT' for c in cs[1:-1]) and len(cs) >= 3
    for typ, body, crc in cs:
        assert crc == zlib.crc32(typ + body), typ
    assert cs[0][1] == struct.pack('>IIBBBBB', w, h, 8, 2 if channels == 3 else 0, 0, 0, 0)
    assert cs[-1][1] == b''
    z = b''.join(c[1] for c in cs[1:-1])
    assert zlib.decompress(z) == filtered
    assert struct.unpack('>I', z[-4:])[0] == zlib.adler32(filtered)
    return z


# ---- Huffman -----------------------------------------------------------------------------------------------------------------
def huffman(hist):
    """hist {symbol: count > 0} -> (cost sum(count * length) of an optimal prefix code, the depth of the optimal tree of least
    depth).  The cost is the same for every optimal code."""
    if len(hist) == 1:
        return sum(hist.values()), 1
    heap = [(f, 0, i) for i, f in enumerate(hist.values())]             # (weight, depth below, tie-break)
    heapq.heapify(heap)
    cost, n = 0, len(heap)
    while len(heap) > 1:
        f1, d1, _ = heapq.heappop(heap)
        f2, d2, _ = heapq.heappop(heap)
        cost += f1 + f2
        heapq.heappush(heap, (f1 + f2, max(d1, d2) + 1, n))
        n += 1
    return cost, heap[0][1]


# ---- deflate ---------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, data: bytes):
        self.data, self.pos = data, 0

    def take(self, n: int) -> int:
        v = 0
        for i in range(n):
            v |= ((self.data[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v


def _decoder(lengths):
    """canonical code of RFC 1951 3.2.2: {(length, code): symbol}"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    table = {}
    for sym, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = sym
            nxt[l] += 1
    return table


def _symbol(bits: _Bits, table) -> int:
    code, l = 0, 0
    while True:
        code = (code << 1) | bits.take(1)                               # Huffman codes are packed from their most significant bit
        l += 1
        if (l, code) in table:
            return table[(l, code)]
        assert l < 16, 'no code matches'


def blocks(z: bytes):
    """Walk the deflate stream of a zlib stream made of stored and literal-only dynamic blocks -> [{'final', 'type' ('stored' |
    'dynamic'), 'data' (bytes), and for dynamic blocks 'lengths' (the 257+ literal/length code lengths), 'dist_lengths',
    'payload_bits' (the bits of the literals and end-of-block)}]"""
    assert (z[0] << 8 | z[1]) % 31 == 0 and z[0] & 15 == 8
    bits, out = _Bits(z[2:-4]), []
    while True:
        blk = {'final': bits.take(1)}
        btype = bits.take(2)
        if btype == 0:
            bits.pos = (bits.pos + 7) & ~7
            n, nn = bits.take(16), bits.take(16)
            assert n ^ nn == 0xffff
            blk.update(type='stored', data=bytes(bits.data[bits.pos >> 3:(bits.pos >> 3) + n]))
            bits.pos += 8 * n
        else:
            assert btype == 2, 'only stored and dynamic blocks are written'
            hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
            cl = [0] * 19
            for i in range(hclen):
                cl[CLC_ORDER[i]] = bits.take(3)
            assert sum(2.0 ** -l for l in cl if l) == 1.0               # inflate requires a complete code-length code
            table, lengths = _decoder(cl), []
            while len(lengths) < hlit + hdist:
                s = _symbol(bits, table)
                if s < 16:
                    lengths.append(s)
                elif s == 16:
                    lengths += [lengths[-1]] * (3 + bits.take(2))
                else:
                    lengths += [0] * ((3 + bits.take(3)) if s == 17 else (11 + bits.take(7)))
            assert len(lengths) == hlit + hdist
            lit, dist = lengths[:hlit], lengths[hlit:]
            table, data, p0 = _decoder(lit), bytearray(), bits.pos
            while True:
                s = _symbol(bits, table)
                assert s <= 256, 'a length code: this encoder writes literals only'
                if s == 256:
                    break
                data.append(s)
            blk.update(type='dynamic', data=bytes(data), lengths=lit, dist_lengths=dist, payload_bits=bits.pos - p0)
        out.append(blk)
        if blk['final']:
            break
    assert (bits.pos + 7) >> 3 == len(bits.data)
    return out


def check_blocks(z: bytes, filtered: bytes):
    """the block structure every stream must have: ceil(F / S) blocks of S bytes (the last one shorter), BFINAL on the last only,
    complete literal codes of at most 15 bits with the one unused distance code, optimal whenever an optimal code of depth <= 15
    exists, and no block longer than its stored form -> the blocks"""
    bl = blocks(z)
    assert len(bl) == -(-len(filtered) // S)
    assert [b['final'] for b in bl] == [0] * (len(bl) - 1) + [1]
    for i, b in enumerate(bl):
        assert b['data'] == filtered[i * S:(i + 1) * S]
        if b['type'] == 'stored':
            continue
        used = [l for l in b['lengths'] if l]
        assert max(used) <= 15 and sum(2 ** (15 - l) for l in used) == 2 ** 15          # Kraft sum exactly 1
        assert b['dist_lengths'] == [0]
        hist = {s: c for s, c in enumerate(np.bincount(np.frombuffer(b['data'], np.uint8), minlength=256).tolist()) if c}
        hist[256] = 1
        assert all(b['lengths'][s] for s in hist) and len(used) == len(hist)
        cost, depth = huffman(hist)
        assert b['payload_bits'] == sum(c * b['lengths'][s] for s, c in hist.items())
        if depth <= 15:
            assert b['payload_bits'] == cost
        else:
            assert b['payload_bits'] >= cost
        assert HEADER_BITS + b['payload_bits'] < 3 + 7 + 32 + 8 * len(b['data'])
    return bl


def bound(h: int, w: int, channels: int) -> int:
    F = h * (1 + w * channels)
    return F + 5 * -(-F // S) + 63
