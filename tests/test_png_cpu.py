"""The PNG decoder without a GPU: png.parse_png, and the decoder core of csrc/png_inflate.h through its host build
(libmmhand_png_host.so, one lane) - bit-exact against zlib.decompress + a numpy unfilter and against PIL on the whole file,
the fixed table of corrupt streams with the status each must get, and a seeded mutation run with canaries around the scratch
and output buffers.  The same header runs on the device with 64 lanes (tests/test_png_gpu.py)."""
import ctypes as C
import io
import os
import subprocess
import zlib

import numpy as np
import pytest

from tests import png_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "mmhand_amd", "libmmhand_png_host.so")


@pytest.fixture(scope="module")
def host():
    if not os.path.exists(HOST_LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mmhand_amd", "csrc"), "../libmmhand_png_host.so"])
    lib = C.CDLL(HOST_LIB)
    lib.mmh_png_decode_batch_host.restype = C.c_int
    lib.mmh_png_decode_batch_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.mmh_png_host_step_bound.restype = lib.mmh_png_host_last_steps.restype = C.c_uint64
    lib.mmh_png_host_step_bound.argtypes = [C.c_uint64, C.c_uint64]
    return lib


CANARY = 64


def host_decode(lib, streams, H, W, bgr=False):
    """-> (status [N], out [N,H,W,3]); asserts the canaries around scratch and out"""
    n, raw = len(streams), H * (1 + 3 * W)
    buf = np.frombuffer(b"".join(streams), dtype=np.uint8).copy() if sum(map(len, streams)) else np.zeros(1, np.uint8)
    off = np.cumsum([0] + [len(s) for s in streams]).astype(np.int64)
    scr = np.full(n * raw + 2 * CANARY, 0xA5, dtype=np.uint8)
    out = np.full(n * H * W * 3 + 2 * CANARY, 0x5A, dtype=np.uint8)
    st = np.full(n, -1, dtype=np.int32)
    rc = lib.mmh_png_decode_batch_host(buf.ctypes.data, int(off[-1]), off.ctypes.data, n, H, W, scr[CANARY:].ctypes.data,
                                       out[CANARY:].ctypes.data, st.ctypes.data, int(bgr), None)
    assert rc == 0
    assert (scr[:CANARY] == 0xA5).all() and (scr[-CANARY:] == 0xA5).all(), "scratch canary"
    assert (out[:CANARY] == 0x5A).all() and (out[-CANARY:] == 0x5A).all(), "output canary"
    return st, out[CANARY:-CANARY].reshape(n, H, W, 3)


def pil_rgb(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------ parse_png
def test_parse_png_fields_and_errors():
    from mmhand_amd.png import parse_png
    img = P.content("gradient", 7, 5)
    idat = P.deflate(P.filter_rows(img, [0] * 7))
    for split in (None, 1, 7):
        assert parse_png(P.write_png(5, 7, idat, split=split)) == (5, 7, 8, 2, 0, idat)
    assert parse_png(P.write_png(5, 7, idat, depth=16, colour=6, interlace=1))[2:5] == (16, 6, 1)
    good = P.write_png(5, 7, idat, split=7)
    bad_crc = bytearray(good)
    bad_crc[40] ^= 1
    for bad in (b"\x89PNX" + good[4:], bytes(bad_crc), good[:-5], good[:60], good[:8], b"", good[:-12]):
        with pytest.raises(ValueError):
            parse_png(bad)


# ------------------------------------------------------------------------------------------------- valid streams
SIZES = [(1, 1), (5, 7), (16, 16), (129, 65), (128, 128)]          # (W, H)


def valid_matrix():
    """[(name, W, H, file bytes)]: every content x compressor at every size with mixed filters; every filter type forced on
    every row; full flushes; IDAT splits; the far-match cases"""
    cases = []
    for W, H in SIZES:
        for ci, kind in enumerate(("noise", "const", "gradient")):
            img = P.content(kind, H, W, seed=W + ci)
            mixed = P.filter_rows(img, [(r * 7 + ci) % 5 for r in range(H)])
            for how in P.COMPRESSORS:
                if (W, H) in ((129, 65), (128, 128)) and kind != "gradient" and how in ("l1", "rle", "default"):
                    continue                                        # the large sizes: every setting on one content
                cases.append((f"{W}x{H}-{kind}-{how}", W, H, P.write_png(W, H, P.deflate(mixed, how))))
    for W, H in ((5, 7), (16, 16), (129, 65)):
        img = P.content("gradient", H, W, seed=9)
        for ft in range(5):
            cases.append((f"{W}x{H}-filter{ft}", W, H, P.write_png(W, H, P.deflate(P.filter_rows(img, [ft] * H), "l9"))))
    img = P.content("gradient", 65, 129, seed=4)
    raw = P.filter_rows(img, [r % 5 for r in range(65)])
    for how in ("stored", "fixed", "default"):
        cases.append((f"129x65-flush-{how}", 129, 65, P.write_png(129, 65, P.deflate(raw, how, flush_every=1000))))
    for split in (1, 7, 4096):
        cases.append((f"129x65-split{split}", 129, 65, P.write_png(129, 65, P.deflate(raw, "default"), split=split)))
    cases.append(("128x128-far-l9", 128, 128, P.write_png(128, 128, P.deflate(P.far_match_raw(128, 128), "l9"))))
    W, H, z, _ = P.window_edge_case()
    cases.append(("129x85-window-edge", W, H, P.write_png(W, H, z)))
    return cases


def test_host_decode_equals_oracles(host):
    from mmhand_amd.png import parse_png
    cases = valid_matrix()
    assert len(cases) > 60
    by_size = {}
    for name, W, H, data in cases:
        by_size.setdefault((W, H), []).append((name, data))
    for (W, H), group in by_size.items():
        idats = [parse_png(d)[5] for _, d in group]
        for bgr in (False, True):
            st, out = host_decode(host, idats, H, W, bgr=bgr)
            for i, (name, data) in enumerate(group):
                assert st[i] == 0, (name, st[i])
                want = P.unfilter(zlib.decompress(idats[i]), H, W)
                assert np.array_equal(pil_rgb(data), want), name
                assert np.array_equal(out[i], want[:, :, ::-1] if bgr else want), (name, bgr)
            assert host.mmh_png_host_last_steps() <= host.mmh_png_host_step_bound(max(map(len, idats)), H * (1 + 3 * W))


def test_far_match_case_reaches_the_window():
    """the level-9 stream of far_match_raw is far smaller than its input: the 32500-byte period was found"""
    raw = P.far_match_raw(128, 128)
    assert len(P.deflate(raw, "l9")) < 0.75 * len(raw)


# ------------------------------------------------------------------------------------------------- corrupt streams
def test_corrupt_table_statuses(host):
    img, raw, good, table = P.corrupt_table()
    H, W = img.shape[:2]
    assert len(table) >= 20
    streams = [good] + [z for _, z, _ in table] + [good]
    st, out = host_decode(host, streams, H, W)
    assert st[0] == 0 and st[-1] == 0 and np.array_equal(out[0], img) and np.array_equal(out[-1], img)
    for (name, z, want), got in zip(table, st[1:-1]):
        assert got == want, (name, int(got), want)
        if want not in (P.E_FILTER, P.E_OUTPUT_SHORT, P.E_OUTPUT_LONG, P.E_TRAILING):     # those four are PNG's rules, not zlib's
            with pytest.raises(zlib.error):
                zlib.decompress(z)
    # a range outside the buffer
    off = np.array([0, 5, 3], dtype=np.int64)
    buf, scr, o, s2 = np.zeros(8, np.uint8), np.zeros(2 * H * (1 + 3 * W), np.uint8), np.zeros(2 * H * W * 3, np.uint8), np.zeros(2, np.int32)
    assert host.mmh_png_decode_batch_host(buf.ctypes.data, 4, off.ctypes.data, 2, H, W, scr.ctypes.data, o.ctypes.data,
                                          s2.ctypes.data, 0, None) == 0
    assert list(s2) == [P.E_RANGE, P.E_RANGE]


def test_mutations_are_contained(host):
    """2,000 seeded single-byte and truncation mutations of three valid streams: a status every time, canaries intact, steps
    within the bound, and status 0 only with the bytes zlib.decompress gives"""
    W, H = 16, 16
    raw_len = H * (1 + 3 * W)
    img = P.content("gradient", H, W, seed=21)
    raw = P.filter_rows(img, [r % 5 for r in range(H)])
    seeds = [P.deflate(raw, "default"), P.deflate(raw, "fixed"), P.deflate(P.filter_rows(P.content("noise", H, W, 3), [0] * H), "stored")]
    rs = np.random.RandomState(1234)
    muts = []
    for k in range(2000):
        z = bytearray(seeds[k % 3])
        if k % 4 == 3:
            z = z[:rs.randint(0, len(z))]
        else:
            z[rs.randint(0, len(z))] ^= 1 << rs.randint(0, 8)
        muts.append(bytes(z))
    ok = 0
    for i in range(0, len(muts), 100):
        group = muts[i:i + 100]
        st, out = host_decode(host, group, H, W)
        assert host.mmh_png_host_last_steps() <= host.mmh_png_host_step_bound(max(map(len, group)), raw_len)
        for z, s, o in zip(group, st, out):
            assert 0 <= s <= 20
            if s == 0:
                ok += 1
                assert np.array_equal(o, P.unfilter(zlib.decompress(z), H, W))
    assert ok < len(muts) // 2
