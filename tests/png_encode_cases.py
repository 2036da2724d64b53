"""Images and oracles for the PNG encoder tests (tests/test_png_encode_cpu.py through the host build, tests/test_png_encode_gpu.py
on the device): the size x content matrix, the row-filter heuristic restated in numpy, a DEFLATE block-header walker, and the
host build's entry point with canaries round every buffer."""
import ctypes as C
import io
import os
import subprocess

import numpy as np

from tests import png_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "mmhand_amd", "libmmhand_png_host.so")

SIZES = ((1, 1), (5, 7), (16, 16), (129, 65), (256, 256))          # (W, H), from the decoder's matrix
KINDS = ("gradient", "noise", "const", "photo", "stripes")
OK, E_ROOM = 0, 1
CANARY = 64


def photo(H, W, seed=0):
    """low-pass noise: a 5-tap box filter, twice, over uniform noise, stretched to the full range - smooth like a photograph,
    with the last bits still noisy"""
    rs = np.random.RandomState(seed)
    x = rs.rand(H + 8, W + 8, 3)
    for _ in range(2):
        x = sum(np.roll(x, s, 0) for s in range(-2, 3)) / 5
        x = sum(np.roll(x, s, 1) for s in range(-2, 3)) / 5
    x = x[4:4 + H, 4:4 + W]
    x = (x - x.min()) / max(1e-9, x.max() - x.min())
    return np.clip(x * 255 + rs.randn(H, W, 3) * 1.5, 0, 255).round().astype(np.uint8)


def content(kind, H, W, seed=0, seg_rows=16):
    if kind == "photo":
        return photo(H, W, seed)
    if kind == "stripes":                       # segments alternate flat and noise: neighbouring blocks need different codes
        img = P.content("noise", H, W, seed)
        for r0 in range(0, H, 2 * seg_rows):
            img[r0:r0 + seg_rows] = 90
        return img
    return P.content(kind, H, W, seed)


def batch(kind, H, W, n, seed=0):
    return np.stack([content(kind, H, W, seed + 7 * i) for i in range(n)])


def fibonacci_image(W=30000):
    """a single row whose FILTERED bytes have a Fibonacci-like histogram (symbol k + 1 about 3 fib(k) times, 22 symbols;
    the factor keeps the partial sums strictly below the next weight with the filter byte and end-of-block counted in):
    Huffman's tree for it is a chain deeper than 15, so the length limiter must act.  The pixels are the running sums of the
    wanted residues, so the Sub filter gives the residues back; on a first row Paeth predicts what Sub does and the tie goes
    to Sub, and every other type leaves bytes spread over the whole range.  The test asserts the filter byte and the 15-bit
    maximum it reads from the stream, not what this function hoped for."""
    fib = [1, 1]
    while 3 * sum(fib) < 3 * W:
        fib.append(fib[-1] + fib[-2])
    syms = np.concatenate([np.full(3 * c, k + 1, np.uint8) for k, c in enumerate(fib)])[:3 * W]
    np.random.RandomState(3).shuffle(syms)
    res = syms.reshape(1, W, 3).astype(np.int64)
    return (np.cumsum(res, axis=1) & 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ oracles
def choose_filters(img):
    """the heuristic of csrc/png_deflate.h in numpy: per row the filter type with the smallest sum of |signed byte| over the
    row's 3 W filtered bytes, ties to the lower type -> ([H] types, the H (1 + 3 W) filtered bytes)"""
    H, W, _ = img.shape
    cand = [np.frombuffer(P.filter_rows(img, [ft] * H), dtype=np.uint8).reshape(H, 1 + 3 * W) for ft in range(5)]
    cost = np.stack([np.minimum(c[:, 1:].astype(np.int64), 256 - c[:, 1:].astype(np.int64)).sum(1) for c in cand])
    types = np.argmin(cost, axis=0)              # argmin takes the first of equals: the lower type
    rows = np.stack([cand[types[r]][r] for r in range(H)])
    return types, rows.tobytes()


class BitReader:
    def __init__(self, data):
        self.d, self.pos = data, 0

    def bits(self, n):
        v = 0
        for i in range(n):
            v |= ((self.d[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v


def _decoder(lens):
    """canonical code of `lens` -> {(length, code): symbol}"""
    table, code = {}, 0
    for ln in range(1, 16):
        for s, v in enumerate(lens):
            if v == ln:
                table[(ln, code)] = s
                code += 1
        code <<= 1
    return table


def _sym(br, table):
    code = 0
    for ln in range(1, 16):
        code = (code << 1) | br.bits(1)
        if (ln, code) in table:
            return table[(ln, code)]
    raise AssertionError("no code of <= 15 bits matches")


def kraft(lens):
    from fractions import Fraction
    return sum(Fraction(1, 2 ** v) for v in lens if v)


def walk_blocks(stream):
    """every DEFLATE block of a zlib stream made of dynamic literal-only blocks -> [dict(final, btype, lit_lens, dist_lens,
    cl_lens, n_literals)], and the decoded bytes; asserts the stream ends exactly at its trailer"""
    assert stream[0] == 0x78 and (stream[0] * 256 + stream[1]) % 31 == 0 and not stream[1] & 0x20
    br = BitReader(stream)
    br.pos = 16
    blocks, out = [], bytearray()
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    while True:
        final, btype = br.bits(1), br.bits(2)
        blk = dict(final=final, btype=btype)
        blocks.append(blk)
        if btype != 2:
            return blocks, bytes(out)
        hlit, hdist, hclen = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
        cl = [0] * 19
        for i in range(hclen):
            cl[order[i]] = br.bits(3)
        tab, lens = _decoder(cl), []
        while len(lens) < hlit + hdist:
            s = _sym(br, tab)
            if s < 16:
                lens.append(s)
            elif s == 16:
                lens += [lens[-1]] * (3 + br.bits(2))
            elif s == 17:
                lens += [0] * (3 + br.bits(3))
            else:
                lens += [0] * (11 + br.bits(7))
        assert len(lens) == hlit + hdist
        blk.update(cl_lens=cl, lit_lens=lens[:hlit], dist_lens=lens[hlit:])
        lit, n = _decoder(lens[:hlit]), 0
        while True:
            s = _sym(br, lit)
            if s == 256:
                break
            assert s < 256, "a length symbol in a literal-only block"
            out.append(s)
            n += 1
        blk["n_literals"] = n
        if final:
            break
    assert (br.pos + 7) // 8 + 4 == len(stream)
    return blocks, bytes(out)


def pil_png_size(img):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="PNG")
    return len(b.getvalue())


# --------------------------------------------------------------------------------------------------------------- host build
def host_lib():
    if not os.path.exists(HOST_LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mmhand_amd", "csrc"), "../libmmhand_png_host.so"])
    lib = C.CDLL(HOST_LIB)
    lib.mmh_png_encode_batch_host.restype = C.c_int
    lib.mmh_png_encode_batch_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mmh_png_encode_host_slot_bytes.restype = lib.mmh_png_encode_host_scratch_bytes.restype = C.c_int64
    lib.mmh_png_encode_host_slot_bytes.argtypes = [C.c_int, C.c_int]
    lib.mmh_png_encode_host_scratch_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.mmh_png_encode_host_seg_rows.restype = C.c_int
    return lib


def host_encode(lib, imgs, bgr=False, slot_bytes=None):
    """imgs uint8 [N,H,W,3] -> (status [N], lengths [N], slots uint8 [N, slot_bytes]); the slots start out as 0xC3 and the
    canaries round scratch, the slots, lengths and status are asserted"""
    imgs = np.ascontiguousarray(imgs)
    n, H, W, _ = imgs.shape
    slot = int(slot_bytes if slot_bytes is not None else lib.mmh_png_encode_host_slot_bytes(H, W))
    nscr = int(lib.mmh_png_encode_host_scratch_bytes(n, H, W))
    scr = np.full(nscr + 2 * CANARY, 0xA5, dtype=np.uint8)
    out = np.full(n * slot + 2 * CANARY, 0xC3, dtype=np.uint8)
    lens = np.full(n + 2, -7, dtype=np.int64)
    st = np.full(n + 2, -9, dtype=np.int32)
    assert scr[CANARY:].ctypes.data % 16 == 0
    rc = lib.mmh_png_encode_batch_host(imgs.ctypes.data, n, H, W, int(bgr), scr[CANARY:].ctypes.data, out[CANARY:].ctypes.data,
                                       slot, lens[1:].ctypes.data, st[1:].ctypes.data, None)
    assert rc == 0
    assert (scr[:CANARY] == 0xA5).all() and (scr[-CANARY:] == 0xA5).all(), "scratch canary"
    assert (out[:CANARY] == 0xC3).all() and (out[-CANARY:] == 0xC3).all(), "stream canary"
    assert lens[0] == -7 and lens[-1] == -7 and st[0] == -9 and st[-1] == -9, "lengths / status canary"
    slots = out[CANARY:CANARY + n * slot].reshape(n, slot)
    for i in range(n):                          # nothing past the stream's end, nothing at all for an image without room
        k = int(lens[1 + i]) if st[1 + i] == OK else 0
        assert (slots[i, k:] == 0xC3).all(), f"slot {i} written past its stream"
    return st[1:-1].copy(), lens[1:-1].copy(), slots
