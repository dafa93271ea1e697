"""A PNG reader in numpy, independent of the encoder under test: the chunk walk with zlib.crc32 on every chunk,
zlib.decompress of the IDAT data (which also checks Adler-32) and the five unfilters of the PNG specification (§9.2).
8 bits per sample, colour types 0 (gray) and 6 (RGBA), no interlace: what libaptgpu's encoder writes.  Also the walk over
the deflate blocks of a zlib stream (their types and BFINAL bits) and the size of a file made of stored blocks."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def chunks(data):
    """[(type, payload)] of a PNG file; asserts the signature, every CRC and that nothing follows IEND."""
    assert data[:8] == SIGNATURE, "signature"
    out, p = [], 8
    while p < len(data):
        assert p + 12 <= len(data), "truncated chunk"
        (n,) = struct.unpack(">I", data[p:p + 4])
        kind = data[p + 4:p + 8]
        assert p + 12 + n <= len(data), "chunk runs past the file"
        payload = data[p + 8:p + 8 + n]
        (crc,) = struct.unpack(">I", data[p + 8 + n:p + 12 + n])
        assert crc == zlib.crc32(kind + payload), f"CRC of {kind!r}"
        out.append((kind, payload))
        p += 12 + n
        if kind == b"IEND":
            break
    assert p == len(data), "bytes behind IEND"
    return out


def header(data):
    """(width, height, bit_depth, colour_type, compression, filter_method, interlace) of IHDR."""
    kind, payload = chunks(data)[0]
    assert kind == b"IHDR" and len(payload) == 13
    return struct.unpack(">IIBBBBB", payload)


def idat(data):
    """The concatenated IDAT payloads (the zlib stream)."""
    return b"".join(p for k, p in chunks(data) if k == b"IDAT")


def filtered(data):
    """The filtered scanlines: the inflated zlib stream (zlib verifies Adler-32), as (height, 1 + width * bpp) u8."""
    width, height, depth, ctype, comp, filt, lace = header(data)
    assert depth == 8 and ctype in (0, 6) and comp == 0 and filt == 0 and lace == 0, (depth, ctype, comp, filt, lace)
    bpp = 4 if ctype == 6 else 1
    raw = zlib.decompress(idat(data))
    assert len(raw) == height * (1 + width * bpp), (len(raw), height, width, bpp)
    return np.frombuffer(raw, np.uint8).reshape(height, 1 + width * bpp), bpp


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def unfilter(rows, bpp):
    """Undo the per-row filters (None, Sub, Up, Average, Paeth): (height, 1 + n) u8 -> (height, n) u8."""
    height, n = rows.shape[0], rows.shape[1] - 1
    out = np.zeros((height, n), np.uint8)
    prev = np.zeros(n, np.int64)
    for r in range(height):
        f = int(rows[r, 0])
        x = rows[r, 1:].astype(np.int64)
        assert 0 <= f <= 4, f"filter type {f}"
        if f == 0:
            cur = x
        elif f == 2:
            cur = (x + prev) & 255
        elif f == 1:
            # Recon(x) = Filt(x) + Recon(a): a running sum per byte lane of the pixel
            cur = np.zeros(n, np.int64)
            for k in range(bpp):
                cur[k::bpp] = np.cumsum(x[k::bpp]) & 255
        else:
            # Average and Paeth depend on the reconstructed left neighbour: pixel by pixel, the bpp lanes at once
            cur = np.zeros(n, np.int64)
            left = np.zeros(bpp, np.int64)
            upleft = np.zeros(bpp, np.int64)
            for i in range(0, n, bpp):
                up = prev[i:i + bpp]
                if f == 3:
                    v = (x[i:i + bpp] + ((left + up) >> 1)) & 255
                else:
                    v = (x[i:i + bpp] + _paeth(left, up, upleft)) & 255
                cur[i:i + bpp] = v
                left, upleft = v, up
        out[r] = cur
        prev = cur
    return out


def read(data):
    """The pixels of a PNG file: (height, width) u8 for colour type 0, (height, width, 4) for colour type 6."""
    rows, bpp = filtered(data)
    width, height = header(data)[:2]
    px = unfilter(rows, bpp)
    return px.reshape(height, width, 4) if bpp == 4 else px.reshape(height, width)


def filter_types(data):
    return filtered(data)[0][:, 0].copy()


# ------------------------------------------------------------------ deflate block walk
class _Bits:
    def __init__(self, data):
        self.d, self.p = data, 0

    def get(self, n):
        v = 0
        for k in range(n):
            v |= ((self.d[self.p >> 3] >> (self.p & 7)) & 1) << k
            self.p += 1
        return v


def _huffman(lengths):
    """{(length, code): symbol} of the canonical code (RFC 1951 §3.2.2); asserts it is complete or a single code."""
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
    kraft = sum(2.0 ** -l for l in lengths if l)
    assert kraft == 1.0 or sum(1 for l in lengths if l) <= 1, f"incomplete or oversubscribed code ({kraft})"
    return table


def _decode(bits, table):
    code = 0
    for l in range(1, 16):
        code = (code << 1) | bits.get(1)
        if (l, code) in table:
            return table[(l, code)]
    raise AssertionError("bad Huffman code")


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
          6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
_CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def deflate_blocks(zstream):
    """Walks a zlib stream's deflate blocks: [(bfinal, btype, bytes_out, max_distance)], and the bytes it inflates
    to.  A slow bit-by-bit inflater of its own; use on small streams."""
    assert (zstream[0] * 256 + zstream[1]) % 31 == 0 and zstream[0] & 15 == 8 and not zstream[1] & 32, "zlib header"
    bits = _Bits(zstream[2:])
    out = bytearray()
    blocks = []
    while True:
        final, btype = bits.get(1), bits.get(2)
        start, far = len(out), 0
        assert btype != 3
        if btype == 0:
            bits.p = (bits.p + 7) & ~7
            n, nn = bits.get(16), bits.get(16)
            assert n == (~nn & 0xffff), "LEN / NLEN"
            q = bits.p >> 3
            out += bits.d[q:q + n]
            bits.p += 8 * n
        else:
            if btype == 1:
                lit = _huffman([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
                dist = _huffman([5] * 30)
            else:
                hlit, hdist, hclen = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[_CLORDER[k]] = bits.get(3)
                clt = _huffman(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    s = _decode(bits, clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits.get(2))
                    elif s == 17:
                        lens += [0] * (3 + bits.get(3))
                    else:
                        lens += [0] * (11 + bits.get(7))
                assert len(lens) == hlit + hdist, "code lengths run over"
                lit, dist = _huffman(lens[:hlit]), _huffman(lens[hlit:])
            while True:
                s = _decode(bits, lit)
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    n = _LBASE[s - 257] + bits.get(_LEXT[s - 257])
                    ds = _decode(bits, dist)
                    d = _DBASE[ds] + bits.get(_DEXT[ds])
                    assert d <= len(out), "distance before the start"
                    far = max(far, d)
                    for _ in range(n):
                        out.append(out[-d])
        blocks.append((final, btype, len(out) - start, far))
        if final:
            break
    bits.p = (bits.p + 7) & ~7
    tail = bits.d[bits.p >> 3:]
    assert len(tail) == 4 and struct.unpack(">I", tail)[0] == zlib.adler32(bytes(out)), "Adler-32 / trailing bytes"
    return blocks, bytes(out)


def stored_file_size(width, height, channels):
    """Bytes of a PNG of that shape whose zlib stream holds only stored blocks of up to 65535 bytes."""
    raw = height * (1 + width * channels)
    blocks = max(1, -(-raw // 65535))
    return 8 + (12 + 13) + (12 + 2 + raw + 5 * blocks + 4) + 12
