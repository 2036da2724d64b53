"""mmh_png_decode_batch on the device: the valid matrix of tests/test_png_cpu.py bit for bit against zlib.decompress + the
numpy unfilter and against data._read_bgr, batches of 1 / 3 / 130 mixed streams, 256 x 256 under every compressor setting,
the fixed corrupt table status for status against the host build with canaries around every buffer, and the loader /
entry-point equivalence of --device_png with the default PIL path."""
import ctypes as C
import json
import os
import subprocess
import sys
import zlib
from collections import Counter

import numpy as np
import pytest
import torch

from tests import _dataset_fixture as F
from tests import png_cases as P
from tests.test_png_cpu import host, host_decode, valid_matrix  # noqa: F401  (host is a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 256


def device_decode(dev, streams, H, W, bgr=True):
    """raw C-ABI call with canaries around the stream, scratch, output and status buffers -> (status, out) as numpy"""
    from mmhand_amd import lib as L
    n, raw = len(streams), H * (1 + 3 * W)
    blob = np.frombuffer(b"".join(streams), dtype=np.uint8)
    off = torch.tensor(np.cumsum([0] + [len(s) for s in streams]), dtype=torch.int64, device=dev)
    sb = torch.full((len(blob) + 2 * CANARY,), 0x3C, dtype=torch.uint8, device=dev)
    sb[CANARY:CANARY + len(blob)] = torch.from_numpy(blob.copy()).to(dev)
    scr = torch.full((n * raw + 2 * CANARY,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((n * H * W * 3 + 2 * CANARY,), 0x5A, dtype=torch.uint8, device=dev)
    st = torch.full((n + 2 * CANARY // 4,), -7, dtype=torch.int32, device=dev)
    L.call("mmh_png_decode_batch", C.c_void_p(sb.data_ptr() + CANARY), len(blob), C.c_void_p(off.data_ptr()), n, H, W,
           C.c_void_p(scr.data_ptr() + CANARY), C.c_void_p(out.data_ptr() + CANARY), C.c_void_p(st.data_ptr() + CANARY // 2),
           int(bgr), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for t, v in ((sb, 0x3C), (scr, 0xA5), (out, 0x5A)):
        assert bool((t[:CANARY] == v).all()) and bool((t[-CANARY:] == v).all()), "canary"
    assert bool((sb[CANARY:CANARY + len(blob)].cpu() == torch.from_numpy(blob.copy())).all())
    q = CANARY // 8
    assert bool((st[:q] == -7).all()) and bool((st[q + n:] == -7).all()), "status canary"
    return st[q:q + n].cpu().numpy(), out[CANARY:-CANARY].view(n, H, W, 3).cpu().numpy()


@pytest.fixture(scope="module")
def matrix():
    """the valid matrix grouped by size, with its oracle computed once: {(W, H): [(name, file, idat, rgb)]}"""
    from mmhand_amd.png import parse_png
    groups = {}
    for name, W, H, data in valid_matrix():
        idat = parse_png(data)[5]
        groups.setdefault((W, H), []).append((name, data, idat, P.unfilter(zlib.decompress(idat), H, W)))
    return groups


def test_valid_matrix_both_orders(dev, matrix, tmp_path):
    from mmhand_amd.data import _read_bgr
    for (W, H), group in matrix.items():
        for bgr in (True, False):
            st, out = device_decode(dev, [g[2] for g in group], H, W, bgr=bgr)
            for i, (name, data, _, rgb) in enumerate(group):
                assert st[i] == 0, (name, st[i])
                assert np.array_equal(out[i], rgb[:, :, ::-1] if bgr else rgb), (name, bgr)
        path = os.path.join(tmp_path, "x.png")
        with open(path, "wb") as fh:
            fh.write(group[-1][1])
        assert np.array_equal(out[-1][:, :, ::-1], _read_bgr(path))


def test_batches_of_1_3_130_and_position_independence(dev, matrix):
    group = matrix[(129, 65)]
    assert len({len(g[2]) for g in group}) > 5                       # unequal stream lengths
    for n in (1, 3, 130):
        pick = [group[(i * 5 + n) % len(group)] for i in range(n)]
        st, out = device_decode(dev, [g[2] for g in pick], 65, 129)
        st2, out2 = device_decode(dev, [g[2] for g in pick][::-1], 65, 129)
        assert not st.any() and not st2.any()
        assert np.array_equal(out, out2[::-1])                        # a second run, every image at another position
        for i, g in enumerate(pick):
            assert np.array_equal(out[i], g[3][:, :, ::-1]), (n, i, g[0])


def test_256_under_every_compressor(dev):
    img = P.content("gradient", 256, 256, seed=6)
    raw = P.filter_rows(img, [(r * 3) % 5 for r in range(256)])
    streams = [P.deflate(raw, how) for how in P.COMPRESSORS] + [P.deflate(P.filter_rows(P.content("noise", 256, 256), [4] * 256), "l1")]
    st, out = device_decode(dev, streams, 256, 256, bgr=False)
    assert not st.any(), st
    for i in range(len(P.COMPRESSORS)):
        assert np.array_equal(out[i], img), P.COMPRESSORS[i]
    assert np.array_equal(out[-1], P.content("noise", 256, 256))


def test_corrupt_table_matches_host_build(dev, host):     # noqa: F811
    """rejection by status: the streams the host build has already judged (tests/test_png_cpu.py runs first), each between
    valid neighbours"""
    img, raw, good, table = P.corrupt_table()
    H, W = img.shape[:2]
    streams = [good]
    for _, z, _ in table:
        streams += [z, good]
    hst, _ = host_decode(host, streams, H, W, bgr=True)
    st, out = device_decode(dev, streams, H, W, bgr=True)
    assert list(st) == list(hst)
    assert [int(s) for s in st[1::2]] == [want for _, _, want in table]
    for i in range(0, len(streams), 2):
        assert st[i] == 0 and np.array_equal(out[i], img[:, :, ::-1])


# ----------------------------------------------------------------------------------------------------------- loader
class _Spy:
    def __init__(self, monkeypatch):
        from mmhand_amd import lib
        self.calls = Counter()
        real = lib.call

        def call(name, *args):
            self.calls[name] += 1
            return real(name, *args)

        monkeypatch.setattr(lib, "call", call)


def _rewrite(path, mode):
    from PIL import Image
    with Image.open(path) as im:
        im = im.convert("RGB")
    if mode == "palette":
        im.quantize(256).save(path)
    else:
        W, H = im.size
        # PIL reads Adam7 but does not write it: the seven passes are laid out here
        rgb = np.asarray(im)
        passes = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]
        raw = b""
        for x0, y0, dx, dy in passes:
            sub = rgb[y0::dy, x0::dx]
            if sub.size:
                raw += P.filter_rows(np.ascontiguousarray(sub), [0] * sub.shape[0])
        with open(path, "wb") as fh:
            fh.write(P.write_png(W, H, zlib.compress(raw), interlace=1))


@pytest.fixture
def data_dir():
    """a directory without "test" in its path (such a root serves generation only)"""
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="mmh_png_")
    assert "test" not in d
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("kind", ["rhd", "stb"])
def test_loader_equivalence(kind, dev, data_dir, monkeypatch):
    from mmhand_amd.data import HandFolderLoader, _read_bgr
    from mmhand_amd.options import default_train_opt
    root = os.path.join(data_dir, kind)
    if kind == "rhd":
        names = F.write_rhd(root, n=7, size=32)
        pal, inter = os.path.join(root, "color", names[2]), os.path.join(root, "depth", names[4])
    else:
        F.write_stb(root, n=4, size=32)
        pal, inter = os.path.join(root, "B1Counting", "SK_color_1.png"), os.path.join(root, "B2Random", "SK_depth_2.png")
    before = _read_bgr(inter)
    _rewrite(pal, "palette")
    _rewrite(inter, "interlaced")
    assert np.array_equal(_read_bgr(inter), before)                   # PIL reads the hand-made Adam7 file back
    spy = _Spy(monkeypatch)
    for decoded in (False, True):
        opt = default_train_opt(batchSize=3, dataroot=root, dataset=kind, augmentation_ratio=1.0, nThreads=2)
        import random
        random.seed(5)
        a = HandFolderLoader(opt, device=dev, decoded=decoded, device_png=False)
        random.seed(5)
        b = HandFolderLoader(opt, device=dev, decoded=decoded, device_png=True)
        nb = 0
        for x, y in zip(a, b):
            nb += 1
            assert list(x.keys()) == list(y.keys())
            for k in x:
                if torch.is_tensor(x[k]):
                    assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and torch.equal(x[k], y[k]), k
                else:
                    assert x[k] == y[k], k
        assert nb == a.n_batches() and nb >= 3 and len(a.indices()) % 3 != 0          # a short last batch
        assert not a.png_fallbacks
        fell = {p for p, _ in b.png_fallbacks}
        assert fell == {pal, inter}, b.png_fallbacks
        assert all(r.startswith("format") for _, r in b.png_fallbacks)
    assert spy.calls["mmh_png_decode_batch"] >= 6


def test_loader_reuses_its_buffers(dev, data_dir):
    from mmhand_amd.data import HandFolderLoader
    from mmhand_amd.options import default_train_opt
    root = os.path.join(data_dir, "rhd")
    F.write_rhd(root, n=24, size=32)
    opt = default_train_opt(batchSize=2, dataroot=root, dataset="rhd", augmentation_ratio=1.0, nThreads=2)
    ld = HandFolderLoader(opt, device=dev, device_png=True)
    seen = []
    for i, batch in enumerate(ld):
        del batch
        torch.cuda.synchronize()
        seen.append(torch.cuda.memory_allocated())
    assert len(seen) == 12 and len(set(seen[2:])) == 1, seen


def _run(mod, args, env=None):
    """`python -m mod args` with Python's `random` seeded first: the loader shuffles its sources and the image pool draws
    with it, and two processes are compared here"""
    code = f"import random, sys; random.seed(7); from {mod} import main; main({args!r})"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env={**os.environ, **(env or {})})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_train_and_evaluate_entry_points(dev, data_dir, tmp_path):
    """two training iterations and one evaluation on the fixture: --device_png changes nothing in what is computed"""
    import re
    root = os.path.join(data_dir, "rhd")
    F.write_rhd(root, n=8, size=32)
    outs = []
    for flag in ([], ["--device_png"]):
        ck = str(tmp_path / ("ck" + str(len(flag))))
        out = _run("mmhand_amd.train", ["--dataroot", root, "--dataset", "rhd", "--augmentation_ratio", "0.5", "--batchSize", "2",
                                        "--ngf", "8", "--ndf", "8", "--G_n_blocks", "2", "--n_layers_D", "2", "--fineSize", "32",
                                        "--niter", "1", "--niter_decay", "0", "--max_dataset_size", "2", "--print_freq", "1",
                                        "--vgg_random_init", "--no_html", "--name", "t", "--checkpoints_dir", ck,
                                        "--nThreads", "2", "--no_dropout", "--no_dropout_D", "--norm", "instance"] + flag)
        losses = [m for ln in out.splitlines() if ln.startswith("(epoch:")
                  for m in re.findall(r"[A-Za-z_0-9]+: -?\d+\.\d+", ln.split(")", 1)[1])]
        ev = _run("mmhand_amd.evaluate", ["--name", "t", "--checkpoints_dir", ck, "--dataroot", root, "--dataset", "rhd",
                                          "--augmentation_ratio", "0.5", "--batchSize", "4",
                                          "--results_json", str(tmp_path / "r.json")] + flag)
        outs.append((losses, json.loads(ev.strip().splitlines()[-1])))
    assert len(outs[0][0]) >= 12 and outs[0][1]["SSIM_avg"] is not None and outs[0] == outs[1], outs
