"""The PNG encoder without a GPU: the core of csrc/png_deflate.h through its host build (libmmhand_png_host.so, one lane) -
every stream inflates under zlib (which verifies the Adler-32) to exactly the scanlines the numpy restatement of the row
heuristic picks, unfilters to the input pixels, and opens in PIL as the input; every block header is walked bit by bit; the
no-room status leaves the neighbours and every canary alone; the slot bound holds on the worst cases; and the size of the
output is held against PIL's.  The same header runs on the device with 256 lanes (tests/test_png_encode_gpu.py)."""
import ctypes as C
import io
import os
import re
import zlib

import numpy as np
import pytest

from tests import png_cases as P
from tests import png_encode_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    return E.host_lib()


def pil_rgb(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def check_stream(stream, rgb, seg_rows, full=True):
    """one image's zlib stream against every oracle; returns its blocks.  full=False leaves out the two byte-by-byte Python
    walks (the numpy unfilter and the bit reader), which take seconds at 256 x 256: zlib, the filter heuristic and PIL remain"""
    from mmhand_amd.png import write_png
    H, W, _ = rgb.shape
    raw = zlib.decompress(stream)                                   # raises on a wrong Adler-32 or any malformed block
    assert len(raw) == H * (1 + 3 * W)
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert rows[:, 0].max() <= 4
    assert not full or np.array_equal(P.unfilter(raw, H, W), rgb)
    types, want = E.choose_filters(rgb)
    assert list(rows[:, 0]) == list(types) and raw == want
    assert np.array_equal(pil_rgb(write_png(W, H, stream)), rgb)
    if not full:
        return None
    blocks, literals = E.walk_blocks(stream)
    assert literals == raw
    assert len(blocks) == -(-H // seg_rows)
    for k, b in enumerate(blocks):
        assert b["btype"] == 2 and b["final"] == (k == len(blocks) - 1)
        assert b["n_literals"] == min(seg_rows, H - k * seg_rows) * (1 + 3 * W)
        assert E.kraft(b["lit_lens"]) == 1 and max(b["lit_lens"]) <= 15 and len(b["lit_lens"]) == 257
        assert E.kraft(b["cl_lens"]) == 1 and max(b["cl_lens"]) <= 7
        assert b["dist_lens"] == [1]                                # one distance code of one bit, never used
    return blocks


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("W,H", E.SIZES)
def test_streams_are_valid_and_exact(host, W, H, n):
    seg_rows = host.mmh_png_encode_host_seg_rows()
    for kind in E.KINDS:
        imgs = E.batch(kind, H, W, n, seed=11)
        for bgr in (False, True):
            if bgr and n == 5 and (W, H) == (256, 256):
                continue                                            # the pixel order at the real size is covered by n = 1
            st, ln, slots = E.host_encode(host, imgs, bgr=bgr)
            assert (st == E.OK).all()
            for i in range(n):
                full = W * H < 256 * 256 or (i == 0 and not bgr)    # at the real size: the first image of each kind
                blocks = check_stream(slots[i, :ln[i]].tobytes(), imgs[i][:, :, ::-1] if bgr else imgs[i], seg_rows, full)
                if full and kind == "const" and H > seg_rows:       # two symbols per block: 1-bit codes
                    assert sorted(v for v in blocks[-1]["lit_lens"] if v) in ([1, 1], [1, 2, 2])
            if kind == "stripes" and H > 2 * seg_rows:              # neighbouring blocks carry different codes
                b = E.walk_blocks(slots[0, :ln[0]].tobytes())[0]
                assert b[0]["lit_lens"] != b[1]["lit_lens"] and max(b[0]["lit_lens"]) <= 4 and max(b[1]["lit_lens"]) >= 8


def test_no_room_is_a_status_and_neighbours_are_untouched(host):
    """slot_bytes that holds the flat and gradient images but not the noise ones: those get E_ROOM and the size they need, their
    slots are not written at all, the others equal a run with room byte for byte, and the canaries round scratch, the slots,
    lengths and status stay intact (asserted inside host_encode)"""
    H, W = 65, 129
    imgs = np.stack([E.content(k, H, W, seed=i) for i, k in enumerate(("const", "noise", "gradient", "noise", "const"))])
    s0, full, fslots = E.host_encode(host, imgs)
    assert (s0 == E.OK).all()
    slot = int(full[2]) + 3
    assert full[1] > slot and full[3] > slot and full[0] <= slot
    st, ln, slots = E.host_encode(host, imgs, slot_bytes=slot)
    assert list(st) == [E.OK, E.E_ROOM, E.OK, E.E_ROOM, E.OK]
    assert ln[1] == full[1] and ln[3] == full[3]
    for i in (0, 2, 4):
        assert ln[i] == full[i] and np.array_equal(slots[i, :ln[i]], fslots[i, :full[i]])
    for i in (1, 3):
        assert (slots[i] == 0xC3).all()
    exact = int(full[2])
    st, ln, _ = E.host_encode(host, imgs[2:3], slot_bytes=exact)
    assert st[0] == E.OK and ln[0] == exact
    st, ln, _ = E.host_encode(host, imgs[2:3], slot_bytes=exact - 1)
    assert st[0] == E.E_ROOM and ln[0] == exact
    st, ln, _ = E.host_encode(host, imgs[2:3], slot_bytes=8)
    assert st[0] == E.E_ROOM


def test_slot_bound_holds_on_the_worst_cases(host):
    """lengths[i] <= mmh_png_encode_slot_bytes(H, W) - the library's own, host-only entry point - on uniform noise (no code
    beats 8 bits per byte) and on the Fibonacci-like histogram, where Huffman's tree is deeper than 15 and the limiter acts:
    the stream must show a 15-bit code, a Kraft sum of exactly 1, and still fit"""
    from mmhand_amd import lib as L
    lib = L.load()
    seg_rows = host.mmh_png_encode_host_seg_rows()
    for W, H in E.SIZES:
        assert lib.mmh_png_encode_slot_bytes(H, W) == host.mmh_png_encode_host_slot_bytes(H, W) >= 8
        assert lib.mmh_png_encode_scratch_bytes(3, H, W) == host.mmh_png_encode_host_scratch_bytes(3, H, W)
        st, ln, _ = E.host_encode(host, E.batch("noise", H, W, 2, seed=5))
        assert (st == E.OK).all() and (ln <= lib.mmh_png_encode_slot_bytes(H, W)).all()
        assert (ln > H * 3 * W * 0.9).all() or W * H < 64         # noise does not compress: the bound is not idle
    img = E.fibonacci_image()
    st, ln, slots = E.host_encode(host, img[None])
    assert st[0] == E.OK and ln[0] <= lib.mmh_png_encode_slot_bytes(1, img.shape[1])
    stream = slots[0, :ln[0]].tobytes()
    blocks = check_stream(stream, img, seg_rows)
    assert zlib.decompress(stream)[0] == 1                          # the row took the Sub filter: the histogram is the planned one
    assert max(blocks[0]["lit_lens"]) == 15 and sum(v == 15 for v in blocks[0]["lit_lens"]) >= 4
    assert lib.mmh_png_encode_slot_bytes(0, 4) < 0 and lib.mmh_png_encode_slot_bytes(1 << 20, 1 << 20) < 0


def test_argument_errors_return_non_zero(host):
    """the host build and the library refuse the same calls, the library before any launch (no GPU here)"""
    from mmhand_amd import lib as L
    lib = L.load()
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    ln, st = np.zeros(4, np.int64), np.zeros(4, np.int32)
    good = dict(px=p, N=1, H=2, W=2, scr=p, out=p, slot=64, ln=ln.ctypes.data, st=st.ctypes.data)
    bad = [dict(N=-1), dict(H=0), dict(W=0), dict(H=1 << 15, W=1 << 15), dict(px=None), dict(scr=None), dict(out=None),
           dict(ln=None), dict(st=None), dict(slot=7), dict(scr=p + 4)]
    for fn in (host.mmh_png_encode_batch_host, lib.mmh_png_encode_batch):
        for change in bad:
            a = dict(good, **change)
            rc = fn(a["px"], a["N"], a["H"], a["W"], 0, a["scr"], a["out"], a["slot"], a["ln"], a["st"], None)
            assert rc != 0, change
        assert fn(None, 0, 2, 2, 0, None, None, 64, None, None, None) == 0         # an empty batch needs no buffers
    assert b"mmh_png_encode_batch" in lib.mmh_last_error()


def test_abi_declares_and_exports_the_encoder():
    """the three entry points are in the header, in lib.SIGNATURES and in the library's dynamic symbol table (the header and
    the symbol table are diffed as a whole by tests/test_host_cpu.py)"""
    from mmhand_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "mmhand_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = {"mmh_png_encode_slot_bytes", "mmh_png_encode_scratch_bytes", "mmh_png_encode_batch"}
    assert names <= set(re.findall(r"\b(mmh_[a-z0-9_]+)\s*\(", hdr))
    assert names <= set(L.SIGNATURES)
    cdll = C.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(cdll, n), n
    assert re.search(r"MMH_PNGENC_OK\s*=\s*0", hdr) and re.search(r"MMH_PNGENC_E_ROOM\s*=\s*1", hdr)
    assert sum(1 for s in L.SIGNATURES if s.startswith("mmh_png_")) == 4


def test_write_png_container():
    from mmhand_amd.png import parse_png, write_png
    img = P.content("gradient", 7, 5)
    idat = P.deflate(P.filter_rows(img, [0] * 7))
    data = write_png(5, 7, idat)
    assert data == P.write_png(5, 7, idat)
    assert parse_png(data) == (5, 7, 8, 2, 0, idat)
    assert np.array_equal(pil_rgb(data), img)


def test_size_against_pil_on_photo_like_images(host):
    """SIZE BAR: over the photo-like fixture images (low-pass noise, 256 x 256 and 129 x 65, 4 seeds each) the encoder's files -
    Huffman only, one code per 16 rows - may take at most 1.03 x the bytes of PIL.Image.save at its default (zlib level 6 with
    matches).  Measured on this set: 1.0024 (535,394 against 534,136 bytes).  The margin is what 16 block headers per
    256 rows can cost (up to about 100 bytes each: 1.3 % of a 120 KB file) plus as much again for the spread between image
    sets; matches buy PIL next to nothing on such content.  Flat and synthetic contents are exempt (Huffman-only cannot go below one bit per
    byte) and checked for validity only, above."""
    from mmhand_amd.png import write_png
    ours = pil = 0
    for W, H in ((256, 256), (129, 65)):
        imgs = E.batch("photo", H, W, 4, seed=21)
        st, ln, slots = E.host_encode(host, imgs)
        assert (st == E.OK).all()
        for i in range(len(imgs)):
            ours += len(write_png(W, H, slots[i, :ln[i]].tobytes()))
            pil += E.pil_png_size(imgs[i])
    print(f"encoder {ours} bytes, PIL {pil} bytes, ratio {ours / pil:.4f}")
    assert ours <= 1.03 * pil, (ours, pil, ours / pil)
