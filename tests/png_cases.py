"""PNG streams for the decoder tests, built from seeded numpy arrays: a writer that takes explicit scanlines (forced filter
types, any zlib.compressobj setting, full flushes mid-stream, IDAT split anywhere), a numpy unfilter as the oracle beside
zlib.decompress, a bit writer with DEFLATE's fixed code for hand-made streams, and the fixed table of corrupt streams with the
status each must get (the enum of include/mmhand_hip.h)."""
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
(OK, E_HEADER, E_DICT, E_TRUNCATED, E_BLOCK_TYPE, E_STORED_LEN, E_CODE_OVER, E_CODE_INCOMPLETE, E_REPEAT, E_CODE_COUNT, E_NO_EOB,
 E_SYMBOL, E_BAD_CODE, E_DISTANCE, E_OUTPUT_LONG, E_OUTPUT_SHORT, E_TRAILING, E_ADLER, E_FILTER, E_STEPS, E_RANGE) = range(21)

COMPRESSORS = ("stored", "fixed", "l1", "l9", "rle", "default")


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def filter_rows(img, filters):
    """img uint8 [H,W,3] RGB, filters[r] in 0..4 -> the H * (1 + 3 W) filtered scanline bytes"""
    H, W, _ = img.shape
    flat = img.reshape(H, W * 3).astype(np.int32)
    out = np.zeros((H, 1 + 3 * W), dtype=np.uint8)
    for r in range(H):
        ft = filters[r]
        cur = flat[r]
        up = flat[r - 1] if r else np.zeros_like(cur)
        left = np.concatenate([np.zeros(3, np.int32), cur[:-3]])
        ul = np.concatenate([np.zeros(3, np.int32), up[:-3]])
        if ft == 0:
            pred = 0
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (left + up) // 2
        else:
            p = left + up - ul
            pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
        out[r, 0] = ft
        out[r, 1:] = (cur - pred) & 255
    return out.tobytes()


def unfilter(raw, H, W):
    """the oracle: filtered scanlines -> uint8 [H,W,3] RGB (PNG 9.2), byte by byte"""
    stride = 1 + 3 * W
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, stride)
    out = np.zeros((H, 3 * W), dtype=np.int32)
    for r in range(H):
        ft, x = int(rows[r, 0]), rows[r, 1:].astype(np.int32)
        up = out[r - 1] if r else np.zeros(3 * W, np.int32)
        if ft == 0:
            out[r] = x
        elif ft == 2:
            out[r] = (x + up) & 255
        else:
            cur = out[r]
            for i in range(3 * W):
                a = cur[i - 3] if i >= 3 else 0
                b = up[i]
                c = up[i - 3] if i >= 3 else 0
                pred = a if ft == 1 else ((a + b) >> 1 if ft == 3 else _paeth(int(a), int(b), int(c)))
                cur[i] = (x[i] + pred) & 255
    return out.astype(np.uint8).reshape(H, W, 3)


def deflate(raw, how="default", flush_every=None):
    """zlib stream of raw under one of COMPRESSORS; flush_every: a Z_FULL_FLUSH after every that many input bytes"""
    level, strategy = {"stored": (0, zlib.Z_DEFAULT_STRATEGY), "fixed": (6, zlib.Z_FIXED), "l1": (1, zlib.Z_DEFAULT_STRATEGY),
                       "l9": (9, zlib.Z_DEFAULT_STRATEGY), "rle": (6, zlib.Z_RLE), "default": (6, zlib.Z_DEFAULT_STRATEGY)}[how]
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    if not flush_every:
        return co.compress(raw) + co.flush()
    out = []
    for i in range(0, len(raw), flush_every):
        out.append(co.compress(raw[i:i + flush_every]))
        out.append(co.flush(zlib.Z_FULL_FLUSH))
    out.append(co.flush())
    return b"".join(out)


def chunk(typ, body):
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))


def write_png(W, H, idat, split=None, depth=8, colour=2, interlace=0):
    """the file around a zlib stream; split: IDAT chunks of that many bytes"""
    parts = [idat] if not split else [idat[i:i + split] for i in range(0, len(idat), split)]
    return (SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, colour, 0, 0, interlace))
            + b"".join(chunk(b"IDAT", p) for p in parts) + chunk(b"IEND", b""))


def content(kind, H, W, seed=0):
    rs = np.random.RandomState(seed)
    if kind == "noise":
        return rs.randint(0, 256, size=(H, W, 3), dtype=np.uint8)
    if kind == "const":
        return np.full((H, W, 3), 173, dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    g = np.stack([xx * 255 // max(1, W - 1), yy * 255 // max(1, H - 1), (xx + yy) * 255 // max(1, H + W - 2)], -1)
    return ((g + rs.randint(-6, 7, size=g.shape)) & 255).astype(np.uint8)


def far_match_raw(H, W, pitch=32500, seed=5):
    """filtered scanlines (filter 0 everywhere) whose bytes repeat at `pitch`: with level 9 the matches reach almost the whole
    32 KiB window (zlib itself never goes past 32768 - 262)"""
    stride = 1 + 3 * W
    block = np.random.RandomState(seed).randint(0, 256, size=pitch, dtype=np.uint8)
    raw = np.tile(block, H * stride // pitch + 1)[:H * stride].copy()
    raw[::stride] = 0
    return raw.tobytes()


# ---------------------------------------------------------------------------------------------- hand-made DEFLATE
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):                    # n bits of v, least significant first (header fields, extra bits)
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):                   # a Huffman code, most significant bit first
        self.put(int(format(c, f"0{n}b")[::-1], 2), n)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def fixed_lit(self, s):                 # literal / length symbol 0 .. 287 in the fixed code
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def fixed_match(self, length, dist):
        for s in range(28, -1, -1):
            base, extra = _len_code(s)
            if length >= base:
                break
        self.fixed_lit(257 + s)
        self.put(length - base, extra)
        for d in range(29, -1, -1):
            base, extra = _dist_code(d)
            if dist >= base:
                break
        self.code(d, 5)
        self.put(dist - base, extra)

    def bytes(self):
        b = Bits()
        b.acc, b.n, b.out = self.acc, self.n, bytearray(self.out)
        b.align()
        return bytes(b.out)


def _len_code(s):
    if s < 8:
        return 3 + s, 0
    if s == 28:
        return 258, 0
    e = (s - 4) >> 2
    return 3 + ((4 + (s & 3)) << e), e


def _dist_code(d):
    if d < 4:
        return 1 + d, 0
    e = (d >> 1) - 1
    return 1 + ((2 + (d & 1)) << e), e


def zwrap(body, raw):
    return b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(raw))


def fixed_stream(ops, final=True):
    """ops: ints (literals) and (length, dist) pairs -> (one fixed block's bytes, the bytes it inflates to)"""
    b, raw = Bits(), bytearray()
    b.put(1 if final else 0, 1)
    b.put(1, 2)
    for o in ops:
        if isinstance(o, tuple):
            b.fixed_match(*o)
            for _ in range(o[0]):
                raw.append(raw[-o[1]])
        else:
            b.fixed_lit(o)
            raw.append(o)
    b.fixed_lit(256)
    return b.bytes(), bytes(raw)


def window_edge_case():
    """(W, H, zlib stream, raw) of a 129 x 85 image whose hand-made fixed-code stream holds a match of distance exactly 32768
    (zlib's own matches stop 262 short of it), an overlapping match of distance 1 and one of distance 2 with an odd length"""
    W, H = 129, 85
    stride, total = 1 + 3 * W, (1 + 3 * W) * H                        # 388 * 85 = 32980
    rs = np.random.RandomState(11)
    ops = [int(v) for v in rs.randint(0, 256, size=32768)]
    for r in range(H):
        if r * stride < 32768:
            ops[r * stride] = 0
    # rows start every 388 bytes, the last one at 32592: every filter byte is one of the literals above
    ops += [(100, 32768), 7, (60, 1), 9, 4, (total - 32868 - 63, 2)]
    body, raw = fixed_stream(ops)
    assert len(raw) == total and zlib.decompress(zwrap(body, raw)) == raw
    return W, H, zwrap(body, raw), raw


def dynamic_header(hlit, hdist, cl_lens, symbols):
    """a final dynamic block's header: HLIT, HDIST, the 19 code-length code lengths in RFC order (trailing
    zeros trimmed to HCLEN >= 4), then `symbols`: (code-length symbol, extra value) pairs written with the canonical
    code-length code.  Returns a Bits to go on writing into."""
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    seq = [cl_lens.get(s, 0) for s in order]
    n = 19
    while n > 4 and seq[n - 1] == 0:
        n -= 1
    b = Bits()
    b.put(1, 1)
    b.put(2, 2)
    b.put(hlit - 257, 5)
    b.put(hdist - 1, 5)
    b.put(n - 4, 4)
    for v in seq[:n]:
        b.put(v, 3)
    codes, code = {}, 0                                                # canonical codes of the code-length code
    for ln in range(1, 8):
        for s in range(19):
            if cl_lens.get(s, 0) == ln:
                codes[s] = (code, ln)
                code += 1
        code <<= 1
    for s, extra in symbols:
        b.code(*codes[s])
        if s >= 16:
            b.put(extra, {16: 2, 17: 3, 18: 7}[s])
    return b


def corrupt_table(W=5, H=7):
    """[(name, zlib stream, expected status)] for images of W x H; every stream is small"""
    img = content("gradient", H, W, seed=2)
    raw = filter_rows(img, [r % 5 for r in range(H)])
    stride = 1 + 3 * W
    good = deflate(raw, "default")
    stored = deflate(raw, "stored")
    fixed = deflate(raw, "fixed")
    t = [("truncated after the zlib header", good[:2], E_TRUNCATED),
         ("truncated mid-block", good[:len(good) // 2], E_TRUNCATED),
         ("truncated mid-block (stored)", stored[:len(stored) // 2], E_TRUNCATED),
         ("truncated inside the trailer", good[:-2], E_TRUNCATED),
         ("one byte too many", good + b"\x00", E_TRAILING),
         ("raw short by one row", deflate(raw[:-stride], "default"), E_OUTPUT_SHORT),
         ("raw long by one row", deflate(raw + raw[:stride], "default"), E_OUTPUT_LONG),
         ("raw long by one row (stored)", deflate(raw + raw[:stride], "stored"), E_OUTPUT_LONG),
         ("block type 3", b"\x78\x9c" + bytes([0b111]) + b"\x00" * 8, E_BLOCK_TYPE),
         ("stored LEN != ~NLEN", stored[:5] + bytes([stored[5] ^ 1]) + stored[6:], E_STORED_LEN),
         ("wrong Adler-32", good[:-1] + bytes([good[-1] ^ 0x40]), E_ADLER),
         ("preset dictionary flag", bytes([0x78, 0xbb]) + good[2:], E_DICT),
         ("zlib CM != 8", bytes([0x79, (31 - 0x7900 % 31) % 31]) + good[2:], E_HEADER),
         ("filter byte 5", deflate(raw[:stride * 3] + b"\x05" + raw[stride * 3 + 1:], "default"), E_FILTER)]
    # over-subscribed code-length code: three codes of length 1
    b = dynamic_header(257, 1, {0: 1, 1: 1, 2: 1}, [])
    t.append(("over-subscribed code lengths", b"\x78\x9c" + b.bytes() + b"\x00" * 8, E_CODE_OVER))
    # incomplete code-length code: one code of length 2 and one of length 1
    b = dynamic_header(257, 1, {0: 1, 1: 2}, [])
    t.append(("incomplete code lengths", b"\x78\x9c" + b.bytes() + b"\x00" * 8, E_CODE_INCOMPLETE))
    # complete code-length code {16: 1, 0: 1}; the first length symbol is a repeat
    b = dynamic_header(257, 1, {16: 1, 0: 1}, [(16, 0)])
    t.append(("repeat with no previous length", b"\x78\x9c" + b.bytes() + b"\x00" * 8, E_REPEAT))
    # literal/length lengths over-subscribed: 258 lengths, all 1 (code-length code {1: 1, 18: 1})
    b = dynamic_header(257, 1, {1: 1, 18: 1}, [(1, 0)] * 258)
    t.append(("over-subscribed literal code", b"\x78\x9c" + b.bytes() + b"\x00" * 8, E_CODE_OVER))
    # literal/length lengths incomplete: symbols 0 and 256 with lengths 2 and 2 only (zeros between them by symbol 18)
    b = dynamic_header(257, 1, {2: 1, 18: 2, 0: 2}, [(2, 0), (18, 127), (18, 106), (2, 0), (0, 0)])
    t.append(("incomplete literal code", b"\x78\x9c" + b.bytes() + b"\x00" * 8, E_CODE_INCOMPLETE))
    # fixed-code streams
    fb = Bits()
    fb.put(1, 1); fb.put(1, 2); fb.fixed_lit(0); fb.fixed_lit(1); fb.fixed_match(3, 3)       # noqa: E702
    t.append(("distance before the start", b"\x78\x9c" + fb.bytes() + b"\x00" * 8, E_DISTANCE))
    fb = Bits()
    fb.put(1, 1); fb.put(1, 2); fb.fixed_lit(0); fb.fixed_lit(286)                            # noqa: E702
    t.append(("length symbol 286", b"\x78\x9c" + fb.bytes() + b"\x00" * 8, E_SYMBOL))
    fb = Bits()
    fb.put(1, 1); fb.put(1, 2); fb.fixed_lit(0); fb.fixed_lit(257); fb.code(30, 5)            # noqa: E702
    t.append(("distance symbol 30", b"\x78\x9c" + fb.bytes() + b"\x00" * 8, E_SYMBOL))
    assert zlib.decompress(good) == raw and zlib.decompress(fixed) == raw
    return img, raw, good, t
