"""--resident_dataset on the device: the scatter into the store (mmh_store_images), the indexed decode pass
(mmh_decode_inputs_indexed) bit for bit against the batch-fed passes it restates, its 64-bit offsets, and the flag through
data.HandFolderLoader (fill epoch, resident epochs) and MMHandModel.set_input.

No test hands a slot outside the store to the indexed pass: the table is range-checked on the host (data.check_table,
tests/test_resident_cpu.py)."""
import os
import random
import shutil
import tempfile
from collections import Counter

import numpy as np
import pytest
import torch

from tests import _dataset_fixture as F
from tests.golden import recipe as RC

pytestmark = pytest.mark.gpu
SM = RC.SMALL
S, HS, WS = 7, 12, 20               # H != W: a transposed index shows
CANARY = 256


# ----------------------------------------------------------------------------------------------------------- scatter
@pytest.mark.parametrize("H,W,shift", [(12, 20, 0), (12, 20, 4), (5, 7, 0)], ids=["16-byte words", "misaligned", "odd bytes"])
def test_scatter_writes_the_named_slots_and_nothing_else(dev, H, W, shift):
    """5 images into slots [3, -1, 0, 6, 2] of 7: the named slots equal their images, slots 1, 4, 5 and the canaries on both
    sides keep their bytes, status stays 0.  12 x 20 x 3 = 720 bytes goes in 16-byte words when both buffers are aligned;
    the shifted store and the 105-byte images take the byte kernel."""
    from mmhand_amd import ops
    rs = np.random.RandomState(21)
    per = H * W * 3
    src = torch.from_numpy(rs.randint(0, 256, size=(5, H, W, 3)).astype(np.uint8)).to(dev)
    buf = torch.full((2 * CANARY + shift + S * per,), 0x5A, dtype=torch.uint8, device=dev)
    store = buf[CANARY + shift: CANARY + shift + S * per].view(S, H, W, 3)
    store.copy_(torch.from_numpy((np.arange(S * per) % 251).astype(np.uint8).reshape(S, H, W, 3)).to(dev))
    before = buf.clone()
    slots = torch.tensor([3, -1, 0, 6, 2], dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.store_images(src, slots, store, status)
    torch.cuda.synchronize()
    assert int(status) == 0
    for n, s in enumerate([3, -1, 0, 6, 2]):
        if s >= 0:
            assert torch.equal(store[s], src[n]), (n, s)
    want = before.clone()
    w = want[CANARY + shift: CANARY + shift + S * per].view(S, H, W, 3)
    for n, s in ((0, 3), (2, 0), (3, 6), (4, 2)):
        w[s] = src[n]
    assert torch.equal(buf, want)                   # slots 1, 4, 5 and both canaries included
    assert bool((buf[: CANARY + shift] == 0x5A).all()) and bool((buf[CANARY + shift + S * per:] == 0x5A).all())


def test_scatter_flags_a_slot_outside_the_store_and_writes_nothing_for_it(dev):
    """the guard of the WRITING kernel (the only one a bad slot is fed to on the device): slot S and slot -2 leave the
    store and the canaries as they were and raise the status bit; the good image next to them still lands"""
    from mmhand_amd import ops
    rs = np.random.RandomState(22)
    per = HS * WS * 3
    src = torch.from_numpy(rs.randint(0, 256, size=(3, HS, WS, 3)).astype(np.uint8)).to(dev)
    pad = 2 * per                       # canaries wide enough to hold what a missing guard would write for slots -2 and S
    buf = torch.full((2 * pad + S * per,), 0x5A, dtype=torch.uint8, device=dev)
    store = buf[pad: pad + S * per].view(S, HS, WS, 3)
    want = buf.clone()
    want[pad: pad + S * per].view(S, HS, WS, 3)[5] = src[1]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.store_images(src, torch.tensor([S, 5, -2], dtype=torch.int32, device=dev), store, status)
    torch.cuda.synchronize()
    assert int(status) == 1 and torch.equal(buf, want)


# ---------------------------------------------------------------------------------------------------- indexed decode
# slot 0 and slot 6; sample 1 has ONE slot as img1 and img2; slot 6 serves two samples (img2 of sample 0, img1 of sample 2)
IDX = [[0, 6, 1, 2], [3, 3, 4, 5], [6, 2, 0, 1]]
# no resize, up, down, and one size past the grid-stride loop's first round (4096 blocks x 256 lanes / 15 = 69,905 pixels)
OUT_SIZES = [None, (24, 40), (8, 12), (192, 200)]


@pytest.fixture(scope="module")
def small_store(dev):
    rs = np.random.RandomState(23)
    store = rs.randint(0, 256, size=(S, HS, WS, 3)).astype(np.uint8)
    store[..., 1] = np.where(rs.rand(S, HS, WS) < 0.5, rs.randint(0, 3, size=(S, HS, WS)), store[..., 1])
    # joints as tests/_dataset_fixture.py draws them: uniform over the image and 4 pixels beyond it
    uv = np.stack([rs.uniform(-4, WS + 4, size=(S, 21)), rs.uniform(-4, HS + 4, size=(S, 21))], -1)
    return torch.from_numpy(store).to(dev), torch.from_numpy(uv).to(dev)


@pytest.mark.parametrize("out", OUT_SIZES, ids=lambda o: "plain" if o is None else "%dx%d" % o)
def test_indexed_decode_is_the_batch_fed_pass_bit_for_bit(dev, small_store, out):
    from mmhand_amd import ops
    store, uv = small_store
    idx = torch.tensor(IDX, dtype=torch.int32, device=dev)
    i = [idx[:, j].long() for j in range(4)]
    want = ops.decode_inputs(store[i[0]], store[i[1]], store[i[2]], store[i[3]], uv[i[0]], uv[i[1]], out_size=out)
    table = uv if out is None else ops.resize_joints(uv, (HS, WS), out)         # the table is on the OUTPUT grid
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    got = ops.decode_inputs_indexed(store, idx, table.contiguous(), out_size=out, status=status)
    torch.cuda.synchronize()
    assert int(status) == 0
    Ho, Wo = out or (HS, WS)
    for name, g, w, c in zip(("x_h1", "x_h2", "x_p", "x_d"), got, want, (4, 4, 44, 8)):
        assert tuple(g.shape) == (3, Ho, Wo, c) and g.dtype == torch.float32, name
        assert torch.equal(g, w), name
    assert float(got[2].abs().sum()) > 0 and float(got[0].abs().sum()) > 0
    # the store's own size given as out_size is the plain pass too
    if out is None:
        same = ops.decode_inputs_indexed(store, idx, uv, out_size=(HS, WS))
        assert all(torch.equal(a, b) for a, b in zip(same, want))


def test_offsets_into_the_store_are_64_bit(dev):
    """11,000 slots of 256 x 256 (2.16 GB, never initialised): slot * Hs * Ws * 3 passes 2^31 at slot 10,923.  Only slots 0
    and 10,999 are written - through the scatter, whose offsets are 64-bit too - and one sample reading both equals the
    batch-fed pass on those two images."""
    from mmhand_amd import ops
    n, hw = 11000, 256
    rs = np.random.RandomState(24)
    two = torch.from_numpy(rs.randint(0, 256, size=(2, hw, hw, 3)).astype(np.uint8)).to(dev)
    uv2 = torch.from_numpy(rs.uniform(-4, hw + 4, size=(2, 21, 2))).to(dev)
    store = torch.empty((n, hw, hw, 3), dtype=torch.uint8, device=dev)
    assert (n - 1) * hw * hw * 3 > 2 ** 31
    store[n - 2].zero_()
    ops.store_images(two, torch.tensor([0, n - 1], dtype=torch.int32, device=dev), store)
    assert torch.equal(store[0], two[0]) and torch.equal(store[n - 1], two[1]) and int(store[n - 2].max()) == 0
    uv = torch.zeros((n, 21, 2), dtype=torch.float64, device=dev)
    uv[0], uv[n - 1] = uv2[0], uv2[1]
    a, b = two[0:1], two[1:2]
    for row, srcs in (([0, n - 1, n - 1, 0], (a, b, b, a, uv2[0:1], uv2[1:2])), ([n - 1, 0, 0, n - 1], (b, a, a, b, uv2[1:2], uv2[0:1]))):
        want = ops.decode_inputs(*[t.contiguous() for t in srcs])
        got = ops.decode_inputs_indexed(store, torch.tensor([row], dtype=torch.int32, device=dev), uv)
        assert all(torch.equal(g, w) for g, w in zip(got, want)), row
    del store
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ loader
class _Spy:
    def __init__(self, monkeypatch):
        from mmhand_amd import lib
        self.calls = Counter()
        real = lib.call

        def call(name, *args):
            self.calls[name] += 1
            return real(name, *args)

        monkeypatch.setattr(lib, "call", call)


@pytest.fixture
def data_dir():
    """a directory without "test" in its path (such a root serves generation only)"""
    d = tempfile.mkdtemp(prefix="mmh_res_")
    assert "test" not in d
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _loader_opt(root, kind, **kw):
    from mmhand_amd.options import default_train_opt
    return default_train_opt(batchSize=3, dataroot=root, dataset=kind, augmentation_ratio=1.0, nThreads=2, **kw)


def _snapshot(batch):
    """a batch with its tensors copied (the --device_png buffer sets take turns: a raw batch is valid for two more yields)"""
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}


def _no_files(monkeypatch):
    from mmhand_amd import data

    def refuse(path):
        raise AssertionError(f"a resident epoch read {path}")

    monkeypatch.setattr(data, "_read_bgr", refuse)
    monkeypatch.setattr(data, "_read_bytes", refuse)


@pytest.mark.parametrize("kind,device_png,resize", [("rhd", False, 0), ("rhd", True, 0), ("rhd", False, 48), ("stb", False, 0)],
                         ids=["rhd", "rhd-device_png", "rhd-resize48", "stb"])
def test_loader_serves_the_second_epoch_from_the_store(kind, device_png, resize, dev, data_dir, monkeypatch):
    """two epochs of a resident loader, raw form and decoded form.  Epoch 1 is today's path (raw batches from the files,
    and the store fills behind them); epoch 2 reads no file and, in the decoded form, makes ONE mmh_decode_inputs_indexed
    call per batch and none of the batch-fed passes.  Per batch, epoch 2 == epoch 1: the uint8 images (gather()), the
    decoded tensors, C1 / C2 and the paths.  Under --resize_inputs the raw form's C1 / C2 of epoch 1 are on the files' grid
    (MMHandModel.set_input scales them) while a resident batch carries them on the output grid already: there they are
    compared through ops.resize_joints, the one place joints are scaled; the decoded form scales in both epochs."""
    from mmhand_amd import ops
    from mmhand_amd.data import HandFolderLoader
    root = os.path.join(data_dir, kind)
    if kind == "rhd":
        F.write_rhd(root, n=7, size=32)
    else:
        F.write_stb(root, n=4, size=32)
    opt = _loader_opt(root, kind, resize_inputs=resize)
    random.seed(5)
    raw = HandFolderLoader(opt, device=dev, device_png=device_png, resident=True)
    random.seed(5)
    dec = HandFolderLoader(opt, device=dev, decoded=True, device_png=device_png, resident=True)
    assert raw.resident_state.startswith("on") and dec.resident_state.startswith("on")
    first_raw = [_snapshot(b) for b in raw]
    first_dec = [_snapshot(b) for b in dec]
    nb = raw.n_batches()
    assert len(first_raw) == len(first_dec) == nb >= 3 and len(raw.indices()) % 3 != 0           # a short last batch
    assert all("img1" in b and "resident" not in b for b in first_raw)
    assert not raw.png_fallbacks and not dec.png_fallbacks
    torch.cuda.synchronize()
    _no_files(monkeypatch)
    spy = _Spy(monkeypatch)
    second_raw = list(raw)
    assert not spy.calls, spy.calls                                 # the raw form: a dictionary per batch, no kernel at all
    second_dec = list(dec)
    assert spy.calls == Counter({"mmh_decode_inputs_indexed": nb}), spy.calls
    assert len(second_raw) == len(second_dec) == nb
    dst = ops.resize_size(resize, (32, 32))
    for b1, b2 in zip(first_raw, second_raw):
        assert set(b2) == {"resident", "C1", "C2", "H1_path", "H2_path"}
        rb = b2["resident"]
        n = len(b1["H1_path"])
        assert rb.B == n == rb.idx.shape[0] and tuple(rb.store.shape[1:]) == (32, 32, 3)
        for k, g in zip(("img1", "img2", "dep1", "dep2"), rb.gather()):
            assert g.dtype == torch.uint8 and torch.equal(g, b1[k]), k
        for k in ("C1", "C2"):
            assert torch.equal(b2[k], b1[k] if dst is None else ops.resize_joints(b1[k], (32, 32), dst)), k
        assert b2["H1_path"] == b1["H1_path"] and b2["H2_path"] == b1["H2_path"]
    for b1, b2 in zip(first_dec, second_dec):
        assert list(b1.keys()) == list(b2.keys())
        for k in b1:
            if torch.is_tensor(b1[k]):
                assert b1[k].dtype == b2[k].dtype and b1[k].shape == b2[k].shape and torch.equal(b1[k], b2[k]), k
            else:
                assert b1[k] == b2[k], k
        assert tuple(b2["H1"].shape[2:]) == ((resize, resize) if resize else (32, 32))
    # the raw form's resident batch, decoded by hand, is the decoded form's batch
    rb = second_raw[0]["resident"]
    xh1, _, xp, _ = ops.decode_inputs_indexed(rb.store, rb.idx, rb.uv_table, out_size=rb.out_size)
    assert torch.equal(ops.nhwc_to_nchw_view(xh1, 3), first_dec[0]["H1"])
    assert torch.equal(ops.nhwc_to_nchw_view(xp)[:, 21:42], first_dec[0]["P2"])
    # a third epoch is the second
    assert all(torch.equal(a["resident"].idx, b["resident"].idx) for a, b in zip(second_raw, raw))


def test_an_epoch_left_early_is_finished_from_the_files(dev, data_dir, monkeypatch):
    """the fill is per batch: a consumer that leaves the first epoch after one batch gets that batch from the store the next
    time and the others from their files, in the loader's order; the epoch after that is resident throughout"""
    from mmhand_amd.data import HandFolderLoader
    root = os.path.join(data_dir, "rhd")
    F.write_rhd(root, n=7, size=32)
    random.seed(5)
    ld = HandFolderLoader(_loader_opt(root, "rhd"), device=dev, resident=True)
    random.seed(5)
    plain = [_snapshot(b) for b in HandFolderLoader(_loader_opt(root, "rhd"), device=dev)]
    for b in ld:
        break
    second = list(ld)
    assert ["resident" in b for b in second] == [True, False, False]
    third = list(ld)
    assert all("resident" in b for b in third)
    keys = ("img1", "img2", "dep1", "dep2")
    for p, b2, b3 in zip(plain, second, third):
        images2 = b2["resident"].gather() if "resident" in b2 else [b2[k] for k in keys]
        for k, g2, g3 in zip(keys, images2, b3["resident"].gather()):
            assert torch.equal(g2, p[k]) and torch.equal(g3, p[k]), k
        assert b2["H1_path"] == b3["H1_path"] == p["H1_path"] and torch.equal(b3["C2"], p["C2"])


def test_a_budget_of_one_byte_leaves_the_loader_as_it_is(dev, data_dir, capsys):
    from mmhand_amd.data import HandFolderLoader
    root = os.path.join(data_dir, "rhd")
    F.write_rhd(root, n=7, size=32)
    random.seed(5)
    ld = HandFolderLoader(_loader_opt(root, "rhd", resident_dataset=True, resident_gb=1e-9), device=dev)
    assert ld.resident_state.startswith("off: ") and "budget" in ld.resident_state
    assert capsys.readouterr().out.count("--resident_dataset off") == 1                 # one line
    random.seed(5)
    plain = HandFolderLoader(_loader_opt(root, "rhd"), device=dev)
    assert plain.resident_state == "off"
    for epoch in range(2):
        got, want = list(ld), list(plain)
        assert len(got) == len(want) == 3
        for x, y in zip(got, want):
            assert list(x.keys()) == list(y.keys()) and "resident" not in x
            assert all(torch.equal(x[k], y[k]) if torch.is_tensor(x[k]) else x[k] == y[k] for k in x)


def test_the_flag_and_the_environment_switch_it_on(dev, data_dir, monkeypatch):
    from mmhand_amd.data import HandFolderLoader, make_loader
    root = os.path.join(data_dir, "rhd")
    F.write_rhd(root, n=7, size=32)
    assert make_loader(_loader_opt(root, "rhd"), device=dev).resident_state == "off"
    assert make_loader(_loader_opt(root, "rhd", resident_dataset=True), device=dev).resident_state.startswith("on: 14 images")
    monkeypatch.setenv("MMH_RESIDENT_DATASET", "1")
    assert HandFolderLoader(_loader_opt(root, "rhd"), device=dev).resident_state.startswith("on")


# ------------------------------------------------------------------------------------------------------------- model
def _model_opt(root, **kw):
    """the configuration tests/test_model_gpu.py's file-fed test runs (its _small_opt("instance") at batch size 2)"""
    from mmhand_amd.options import default_train_opt
    args = dict(batchSize=2, ngf=SM["ngf"], ndf=SM["ndf"], n_layers_D=SM["n_layers_D"], G_n_blocks=SM["n_blocks"],
                norm="instance", no_dropout=True, no_dropout_D=True, pool_size=2, name="resident",
                checkpoints_dir="/tmp/mmh_resident_ckpt", local_rank=0, dataroot=root, dataset="rhd", augmentation_ratio=1.0,
                nThreads=2)
    args.update(kw)
    return default_train_opt(**args)


BUFFERS = ("x_H1", "x_H2", "x_P", "x_D", "input_C1", "input_C2")


@pytest.mark.parametrize("resize", [0, 48], ids=["files' size", "resize48"])
def test_set_input_on_a_resident_batch_is_set_input_on_the_raw_batch(resize, dev, data_dir):
    """the six buffers bit for bit, the paths, and - with equal seeds, on models built alike - equal losses after one
    optimize_parameters(): the inputs are the same bits and the step is deterministic (test_resize_inputs_gpu.py holds two
    runs of it to the bit), so equal means equal"""
    from mmhand_amd.data import HandFolderLoader
    from mmhand_amd.mmhand_model import MMHandModel
    root = os.path.join(data_dir, "rhd")
    F.write_rhd(root, n=6, size=32)
    opt = _model_opt(root, resize_inputs=resize, resident_dataset=True)
    random.seed(5)
    ld = HandFolderLoader(opt, device=dev)
    first = [_snapshot(b) for b in ld]
    second = list(ld)
    assert len(first) == 3 and all("resident" in b for b in second)
    losses, kept = [], []
    for batch in (first[1], second[1]):
        model = MMHandModel(opt)
        model.set_input(batch)
        kept.append({k: getattr(model, k).clone() for k in BUFFERS})
        assert model.get_image_paths() == first[1]["H1_path"][0] + "___" + first[1]["H2_path"][0]
        random.seed(9)
        model.optimize_parameters()
        losses.append([float(v) for v in model.get_current_errors().values()])
    size = resize or 32
    assert tuple(kept[1]["x_P"].shape) == (2, size, size, 44)
    for k in BUFFERS:
        assert torch.equal(kept[0][k], kept[1][k]), k
    print("losses on the raw batch", losses[0], "on the resident batch", losses[1])
    assert losses[0] == losses[1] and all(np.isfinite(losses[0]))


def test_graph_step_replays_on_resident_batches(dev, data_dir, monkeypatch):
    """--graph_step fed resident batches == --graph_step fed the same pairs' raw batches, losses, weights and the generated
    image to the bit: the indexed decode runs in front of the replay and is copied into the captured iteration's inputs, as
    the batch-fed decode is.  Six iterations, as test_resize_inputs_gpu.py runs them: the last two go through the replay."""
    from mmhand_amd.data import HandFolderLoader
    from mmhand_amd.mmhand_model import MMHandModel
    root = os.path.join(data_dir, "rhd")
    F.write_rhd(root, n=8, size=32)
    kw = dict(graph_step=True, resident_dataset=True, name="resident_graph")
    random.seed(5)
    ld = HandFolderLoader(_model_opt(root, **kw), device=dev)
    first = [_snapshot(b) for b in ld]
    second = list(ld)
    assert len(first) == 4 and all("resident" in b for b in second)
    monkeypatch.setenv("MMH_GRAPH_CAPTURE", "1")
    runs = []
    for batches in (first, second):
        random.seed(17)
        model = MMHandModel(_model_opt(root, **kw))
        losses = []
        for it in range(6):
            model.set_input(batches[it % 4])
            model.optimize_parameters()
            losses.append([float(v) for v in model.get_current_errors().values()])
        model._settle_overflow(drain=True)
        torch.cuda.synchronize()
        assert model.graph_error is None and model._graph is not None and model.graph_replays >= 2
        runs.append((losses, [getattr(model, n).flat_param.detach().clone() for n in ("netG", "netD_PB", "netD_PP")],
                     model.fake_p2.detach().clone()))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1])) and torch.equal(runs[0][2], runs[1][2])
