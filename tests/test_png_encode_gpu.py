"""mmh_png_encode_batch on the device: the size x content x N matrix of tests/test_png_encode_cpu.py byte for byte against the
host build of the same header (csrc/png_deflate.h with one lane), the round trip through the project's own device decoder and
through PIL, the no-room status with canaries round every device buffer, buffer reuse across batches, and `aug --device_png`
against the PIL-written run."""
import ctypes as C
import io
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

from tests import png_encode_cases as E

pytestmark = pytest.mark.gpu
CANARY = 256


@pytest.fixture(scope="module")
def host():
    return E.host_lib()


def device_encode(dev, imgs, bgr=False, slot_bytes=None):
    """raw C-ABI call with canaries round scratch, the slots, lengths and status -> (status, lengths, slots [N, slot]) as
    numpy; the slots start out as 0xC3, and an image's slot must still hold that past its stream (everywhere, without room)"""
    from mmhand_amd import lib as L
    lib = L.load()
    imgs = np.ascontiguousarray(imgs)
    n, H, W, _ = imgs.shape
    slot = int(slot_bytes if slot_bytes is not None else lib.mmh_png_encode_slot_bytes(H, W))
    nscr = int(lib.mmh_png_encode_scratch_bytes(n, H, W))
    px = torch.from_numpy(imgs).to(dev)
    scr = torch.full((nscr + 2 * CANARY,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((n * slot + 2 * CANARY,), 0xC3, dtype=torch.uint8, device=dev)
    ln = torch.full((n + 2,), -7, dtype=torch.int64, device=dev)
    st = torch.full((n + 2,), -9, dtype=torch.int32, device=dev)
    L.call("mmh_png_encode_batch", C.c_void_p(px.data_ptr()), n, H, W, int(bgr), C.c_void_p(scr.data_ptr() + CANARY),
           C.c_void_p(out.data_ptr() + CANARY), slot, C.c_void_p(ln.data_ptr() + 8), C.c_void_p(st.data_ptr() + 4),
           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    scr, out, ln, st = scr.cpu().numpy(), out.cpu().numpy(), ln.cpu().numpy(), st.cpu().numpy()
    assert (scr[:CANARY] == 0xA5).all() and (scr[-CANARY:] == 0xA5).all(), "scratch canary"
    assert (out[:CANARY] == 0xC3).all() and (out[-CANARY:] == 0xC3).all(), "stream canary"
    assert ln[0] == -7 and ln[-1] == -7 and st[0] == -9 and st[-1] == -9, "lengths / status canary"
    slots = out[CANARY:CANARY + n * slot].reshape(n, slot)
    for i in range(n):
        k = int(ln[1 + i]) if st[1 + i] == E.OK else 0
        assert (slots[i, k:] == 0xC3).all(), f"slot {i} written past its stream"
    return st[1:-1].copy(), ln[1:-1].copy(), slots


def pil_rgb(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("W,H", E.SIZES)
def test_device_streams_equal_the_host_build(dev, host, W, H, n):
    """every content kind, both pixel orders: status all 0, lengths and the whole slots (0xC3 past each stream on both sides)
    equal the host build's; PIL decodes every file to the exact pixels"""
    from mmhand_amd.png import write_png
    for kind in E.KINDS:
        imgs = E.batch(kind, H, W, n, seed=11)
        for bgr in (False, True):
            hs, hl, hslots = E.host_encode(host, imgs, bgr=bgr)
            ds, dl, dslots = device_encode(dev, imgs, bgr=bgr)
            assert (ds == 0).all() and (hs == 0).all(), (kind, bgr, ds)
            assert np.array_equal(dl, hl), (kind, bgr, dl, hl)
            assert np.array_equal(dslots, hslots), (kind, bgr)
            for i in range(n):
                got = pil_rgb(write_png(W, H, dslots[i, :dl[i]].tobytes()))
                assert np.array_equal(got, imgs[i][:, :, ::-1] if bgr else imgs[i]), (kind, bgr, i)


@pytest.mark.parametrize("W,H", E.SIZES)
def test_own_decoder_accepts_own_encoder(dev, W, H):
    """decode_png_batch(encode_png_batch(x)) == x with empty fallback reports on both sides, in both pixel orders"""
    from mmhand_amd.png import decode_png_batch, encode_png_batch
    imgs = np.stack([E.content(k, H, W, seed=3 + i) for i, k in enumerate(E.KINDS)])
    x = torch.from_numpy(imgs).to(dev)
    for bgr in (False, True):
        files, report = encode_png_batch(x, bgr=bgr)
        assert report == [] and len(files) == len(imgs)
        back, fallback = decode_png_batch(files, dev, bgr=bgr)
        assert fallback == []
        assert torch.equal(back, x), bgr


def test_no_room_is_a_status_and_neighbours_are_untouched(dev, host):
    """slot_bytes between the flat images' streams and the noise images': the noise images get E_ROOM and the size they need,
    their slots stay as they were, the flat images' slots equal a run with room byte for byte, every canary is intact (checked
    in device_encode after the copy back) - and the host build does the same.  The kernel tests the room itself; nothing
    here faults."""
    H, W = 65, 129
    imgs = np.stack([E.content(k, H, W, seed=i) for i, k in enumerate(("const", "noise", "gradient", "noise", "const"))])
    _, full, fslots = device_encode(dev, imgs)
    slot = int(full[2]) + 3                                         # the gradient image fits with 3 bytes to spare
    assert full[1] > slot and full[3] > slot and full[0] <= slot
    ds, dl, dslots = device_encode(dev, imgs, slot_bytes=slot)
    hs, hl, hslots = E.host_encode(host, imgs, slot_bytes=slot)
    assert list(ds) == [E.OK, E.E_ROOM, E.OK, E.E_ROOM, E.OK] and list(hs) == list(ds)
    assert np.array_equal(dl, hl) and np.array_equal(dslots, hslots)
    assert dl[1] == full[1] and dl[3] == full[3]
    for i in (0, 2, 4):
        assert dl[i] == full[i] and np.array_equal(dslots[i, :dl[i]], fslots[i, :full[i]])
    for i in (1, 3):
        assert (dslots[i] == 0xC3).all()
    exact = int(full[2])                                            # a slot of exactly the stream's size is room enough
    es, el, _ = device_encode(dev, imgs[2:3], slot_bytes=exact)
    assert es[0] == E.OK and el[0] == exact
    es, el, _ = device_encode(dev, imgs[2:3], slot_bytes=exact - 1)
    assert es[0] == E.E_ROOM and el[0] == exact


def test_encoder_reuses_its_buffers_and_falls_back_to_pil(dev):
    """one PngBatchEncoder: batch A, another batch of another N, batch A again -> identical bytes and the same device buffers;
    with a slot too small for the noise image that image comes from PIL, is reported, and still decodes to its pixels"""
    from mmhand_amd.png import PngBatchEncoder
    H, W = 65, 129
    a = torch.from_numpy(E.batch("photo", H, W, 4, seed=1)).to(dev)
    b = torch.from_numpy(E.batch("noise", H, W, 3, seed=2)).to(dev)
    enc = PngBatchEncoder(dev)
    first, rep = enc.encode(a)
    ptrs = (enc.scratch.data_ptr(), enc.slots_d.data_ptr(), enc.slots_h.data_ptr())
    other, _ = enc.encode(b)
    again, rep2 = enc.encode(a)
    assert rep == [] and rep2 == [] and first == again and other != first[:3]
    assert ptrs == (enc.scratch.data_ptr(), enc.slots_d.data_ptr(), enc.slots_h.data_ptr())
    plan = enc.launch(b)                                            # one plan at a time: the buffers are the launched batch's
    with pytest.raises(RuntimeError):
        enc.launch(a)
    assert enc.fetch(plan)[0] == other
    with pytest.raises(RuntimeError):
        enc.fetch(plan)
    mixed = torch.cat([a[:1], b[:1]])
    small = PngBatchEncoder(dev, slot_bytes=len(first[0]) + 64)
    files, report = small.encode(mixed)
    assert [i for i, _ in report] == [1] and "slot" in report[0][1]
    assert files[0] == first[0]
    for f, x in zip(files, mixed.cpu().numpy()):
        assert np.array_equal(pil_rgb(f), x)


def test_aug_device_png_writes_the_same_pixels(dev, monkeypatch):
    """`aug.main` on the small checkpoint shape and fixture directory of test_train_and_aug_run_on_files (ngf 8, 2 blocks,
    32 x 32; the checkpoint here is a seeded initialisation, which the path under test does not care about): 5 generation
    images at --batch 3 (a ragged last batch).  --device_png writes the same file set as the default run and every PNG
    decodes to the pixels of the PIL-written run at the SAME batch size; --batch 1 without --device_png is the default run
    byte for byte; MMH_DEVICE_PNG=1 alone does not switch the encoder on."""
    from mmhand_amd import aug
    from mmhand_amd import png as PNG
    from mmhand_amd.networks import Generator
    from tests._dataset_fixture import write_rhd
    d = tempfile.mkdtemp(prefix="mmh_ds_")
    try:
        root = os.path.join(d, "rhd")
        write_rhd(root, n=10, size=32)
        monkeypatch.chdir(d)
        os.makedirs(os.path.join("checkpoints", "files"))
        g = Generator(input_nc=[3, 42, 6], output_nc=3, ngf=8, norm_layer="batch", use_dropout=True, n_blocks=2)
        torch.save(g.init_weights("normal", seed=5).state_dict(), os.path.join("checkpoints", "files", "latest_net_netG.pth"))
        argv = ["files", root, "DST", "rhd", "0.5", "0"]

        def run(dst, *flags):
            a = list(argv)
            a[2] = dst
            return aug.main(a + list(flags), ngf=8, n_blocks=2)

        calls = []
        real_launch = PNG.PngBatchEncoder.launch
        monkeypatch.setattr(PNG.PngBatchEncoder, "launch", lambda self, *a, **k: (calls.append(1), real_launch(self, *a, **k))[1])
        base = run("base")
        b1 = run("b1", "--batch", "1")
        monkeypatch.setenv("MMH_DEVICE_PNG", "1")
        pil3 = run("pil3", "--batch", "3")
        assert calls == []                                          # the loader's switch is not the writer's
        monkeypatch.delenv("MMH_DEVICE_PNG")
        dev3 = run("dev3", "--device_png", "--batch", "3")
        assert len(calls) == 2                                      # 5 images: batches of 3 and 2
        rel = lambda paths, top: sorted(os.path.relpath(p, top) for p in paths)
        assert len(base) == 5 and rel(base, "base") == rel(b1, "b1") == rel(pil3, "pil3") == rel(dev3, "dev3")
        for p in rel(base, "base"):
            assert open(os.path.join("base", p), "rb").read() == open(os.path.join("b1", p), "rb").read(), p
            want = pil_rgb(open(os.path.join("pil3", p), "rb").read())
            data = open(os.path.join("dev3", p), "rb").read()
            assert np.array_equal(pil_rgb(data), want), p
            assert want.shape == (32, 32, 3) and want.std() > 0
            w, h, depth, colour, interlace, _ = PNG.parse_png(data)
            assert (w, h, depth, colour, interlace) == (32, 32, 8, 2, 0)
    finally:
        shutil.rmtree(d, ignore_errors=True)
