"""mmh_render_pose_depth on the device against tests/_render_oracle.py, bit for bit, in both output forms; --depth_source joints
through the loaders and MMHandModel.set_input on a prepared directory (also with its depth PNGs gone); aug --novel end to end."""
import contextlib
import json
import os
import pickle
import random
import shutil
import tempfile
from collections import Counter

import numpy as np
import pytest
import torch

from tests import _render_oracle as R
from tests._dataset_fixture import write_rhd

pytestmark = pytest.mark.gpu
SENTINEL = 0x7FC12345               # a NaN with a payload: any arithmetic on it, or a rewrite as another NaN, shows


def _side1(xyz):
    """a second pose set for side 1: the samples in reverse order, moved by a fraction of a pixel and nearer by 7 z units"""
    return np.ascontiguousarray(xyz[::-1] + np.array([2.25, -1.5, -7.0]))


_SIDE1 = {}


def _side1_reference(case):
    if case[0] not in _SIDE1:
        xyz = _side1(R.case_reference(case)[0])
        _SIDE1[case[0]] = (xyz, R.render(xyz, case[1], case[2], case[4], R.BG))
    return _SIDE1[case[0]]


def _sentinel(shape, dev):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


# ----------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_kernel_equals_the_oracle_in_both_output_forms(case, dev):
    from mmhand_amd import ops
    _, H, W, N, radius, _, _ = case
    xyz0, want0, _ = R.case_reference(case)
    xyz1, want1 = _side1_reference(case)
    t0, t1 = torch.from_numpy(np.array(xyz0)).to(dev), torch.from_numpy(xyz1).to(dev)
    # standalone: [N,H,W,4], lanes 0..2 the value, lane 3 zero, and its NCHW view
    alone = ops.render_pose_depth(t0, size=(H, W), radius=radius, bg=R.BG)
    got = alone.cpu().numpy()
    assert got.shape == (N, H, W, 4) and got.dtype == np.float32
    for lane in range(3):
        assert np.array_equal(got[..., lane], want0), (case[0], lane, int((got[..., lane] != want0).sum()))
    assert (_bits(alone)[..., 3] == 0).all()
    view = ops.nhwc_to_nchw_view(alone, 3)
    assert tuple(view.shape) == (N, 3, H, W) and np.array_equal(view[:, 1].cpu().numpy(), want0)
    # in place, both sides in one launch: all eight lanes written, 6 and 7 as zeros
    both = _sentinel((N, H, W, 8), dev)
    assert ops.render_pose_depth(t0, t1, radius=radius, bg=R.BG, out=both) is both
    g = both.cpu().numpy()
    for lane in range(3):
        assert np.array_equal(g[..., lane], want0) and np.array_equal(g[..., 3 + lane], want1), (case[0], lane)
    assert (_bits(both)[..., 6:] == 0).all()
    # one side selected: the other side's lanes (and 6, 7) keep the sentinel bit for bit; the two launches give what one gave
    one = _sentinel((N, H, W, 8), dev)
    ops.render_pose_depth(t0, None, radius=radius, bg=R.BG, out=one)
    b = _bits(one)
    assert (b[..., 3:] == SENTINEL).all() and np.array_equal(b[..., :3], _bits(both)[..., :3])
    ops.render_pose_depth(None, t1, radius=radius, bg=R.BG, out=one)
    b = _bits(one)
    assert (b[..., 6:] == SENTINEL).all() and np.array_equal(b[..., :6], _bits(both)[..., :6])


def test_kernel_background_and_refusals(dev):
    from mmhand_amd import ops
    xyz = torch.full((2, 21, 3), float("nan"), dtype=torch.float64, device=dev)
    out = ops.render_pose_depth(xyz, size=(5, 7), radius=300.0, bg=100.0)
    assert np.array_equal(out[..., :3].cpu().numpy(), np.full((2, 5, 7, 3), np.float32(((100.0 / 255.0) - 0.5) / 0.5)))
    with pytest.raises(ValueError):
        ops.render_pose_depth(xyz, size=(5, 7), radius=-1.0)
    with pytest.raises(ValueError):
        ops.render_pose_depth(xyz, size=(5, 7), bg=float("nan"))
    with pytest.raises(AssertionError):
        ops.render_pose_depth(xyz, size=(5, 7), out=torch.empty((3, 5, 7, 8), device=dev))
    with pytest.raises(AssertionError):
        ops.render_pose_depth(xyz.float(), size=(5, 7))


# ----------------------------------------------------------------------------- the loaders
@pytest.fixture(scope="module")
def rhd_dir():
    """a prepared directory of 32 x 32 files (its path must not contain "test": generic_dataset.py:116 keys on that)"""
    d = tempfile.mkdtemp(prefix="mmh_rd_")
    root = os.path.join(d, "rhd")
    write_rhd(root, n=8, size=32)
    yield root
    shutil.rmtree(d, ignore_errors=True)


@contextlib.contextmanager
def _without_depth(root):
    """the directory with its depth PNGs gone for the time being"""
    away = root + "_depth_away"
    shutil.move(os.path.join(root, "depth"), away)
    try:
        yield
    finally:
        shutil.move(away, os.path.join(root, "depth"))


def _opt(root, **kw):
    from mmhand_amd.options import default_train_opt
    args = dict(batchSize=3, dataroot=root, dataset="rhd", nThreads=2, augmentation_ratio=1.0, ngf=8, ndf=8, n_layers_D=2,
                G_n_blocks=2, norm="instance", pool_size=2, name="render", checkpoints_dir="/tmp/mmh_render", local_rank=0)
    args.update(kw)
    return default_train_opt(**args)


def _loader(root, dev, **kw):
    from mmhand_amd.data import HandFolderLoader
    lkw = {k: kw.pop(k) for k in ("decoded", "resident") if k in kw}
    random.seed(5)
    return HandFolderLoader(_opt(root, **kw), device=dev, **lkw)


def _epoch(ld, epoch=0):
    ld.set_epoch(epoch)
    return [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()} for b in ld]


DECODED = ("H1", "H2", "P1", "P2", "D1", "D2", "C1", "C2")


def _check_against_files_and_oracle(files, joints, size, radius=5.0, bg=R.BG):
    assert len(files) == len(joints) == 3
    for f, j in zip(files, joints):
        assert set(f) == set(j) and f["H1_path"] == j["H1_path"] and f["H2_path"] == j["H2_path"]
        for k in ("H1", "H2", "P1", "P2", "C1", "C2"):
            assert torch.equal(f[k], j[k]), k
        for s in ("1", "2"):
            d = j["D" + s].cpu().numpy()
            assert d.shape == (len(j["H1_path"]), 3, size, size)
            want = R.render(j["C" + s].cpu().numpy(), size, size, radius, bg)
            for c in range(3):
                assert np.array_equal(d[:, c], want), (s, c)
            assert not torch.equal(f["D" + s], j["D" + s])


@pytest.mark.parametrize("kw,size", [({}, 32), ({"resize_inputs": 24}, 24), ({"augment_geom": True, "resize_inputs": 40}, 40),
                                      ({"render_radius": 1.5, "render_bg": 200.0, "device_png": True}, 32)],
                         ids=["plain", "resize24", "augment", "radius-bg-devicepng"])
def test_decoded_loader_joints_vs_files(rhd_dir, dev, kw, size):
    files = _epoch(_loader(rhd_dir, dev, decoded=True, **kw), 1)
    with _without_depth(rhd_dir):
        joints = _epoch(_loader(rhd_dir, dev, decoded=True, depth_source="joints", **kw), 1)
    _check_against_files_and_oracle(files, joints, size, kw.get("render_radius", 5.0), kw.get("render_bg", R.BG))


def test_present_depth_files_change_nothing_and_the_spy_sees_the_render(rhd_dir, dev, monkeypatch):
    from mmhand_amd import lib
    calls = Counter()
    real = lib.call

    def spy(name, *a):
        calls[name] += 1
        return real(name, *a)
    monkeypatch.setattr(lib, "call", spy)
    files = _epoch(_loader(rhd_dir, dev, decoded=True))
    assert calls["mmh_render_pose_depth"] == 0 and calls["mmh_decode_inputs"] == 3
    with_files = _epoch(_loader(rhd_dir, dev, decoded=True, depth_source="joints"))
    assert calls["mmh_render_pose_depth"] == 3 and calls["mmh_decode_inputs"] == 6
    with _without_depth(rhd_dir):
        without = _epoch(_loader(rhd_dir, dev, decoded=True, depth_source="joints"))
    for a, b in zip(with_files, without):
        for k in DECODED:
            assert torch.equal(a[k], b[k]), k
    # the raw form carries two images per pair and no depth key
    raw = _epoch(_loader(rhd_dir, dev, depth_source="joints"))
    assert all("dep1" not in b and "dep2" not in b and tuple(b["img1"].shape[1:]) == (32, 32, 3) for b in raw)
    assert "dep1" in _epoch(_loader(rhd_dir, dev))[0] and len(files) == 3


@pytest.mark.parametrize("kw,size", [({}, 32), ({"resize_inputs": 24}, 24), ({"augment_geom": True}, 32)],
                         ids=["plain", "resize24", "augment"])
def test_resident_loader_joints_mode(rhd_dir, dev, kw, size, monkeypatch):
    """the store's second epoch == the batch-fed path bit for bit, one slot per colour file, no file read and no upload"""
    from mmhand_amd import data
    files = _epoch(_loader(rhd_dir, dev, decoded=True, **kw), 1)
    with _without_depth(rhd_dir):
        fed = _epoch(_loader(rhd_dir, dev, decoded=True, depth_source="joints", **kw), 1)
        res = _loader(rhd_dir, dev, decoded=True, resident=True, depth_source="joints", **kw)
        assert res.resident_state.startswith("on: 8 images of 32 x 32, %d bytes" % (8 * 32 * 32 * 3)), res.resident_state
        assert res._res["store"].shape[0] == 8 == len(set(res.image_source) | set(res.image_target))
        assert not any("depth" in os.path.basename(os.path.dirname(p)) for p in res._res["paths"])
        _epoch(res, 0)
        assert all(res._batch_is_resident(g) for g in range(3))

        def refuse(*a, **k):
            raise AssertionError("a served resident batch reads no file")
        monkeypatch.setattr(data, "_read_bgr", refuse)
        monkeypatch.setattr(data, "_read_bytes", refuse)
        second = _epoch(res, 1)
    for a, b in zip(fed, second):
        assert a["H1_path"] == b["H1_path"]
        for k in DECODED:
            assert torch.equal(a[k], b[k]), k
    _check_against_files_and_oracle(files, second, size)
    assert _loader(rhd_dir, dev, resident=True, **kw).resident_state.startswith("on: 16 images")


def test_raw_and_resident_forms_through_set_input(rhd_dir, dev, monkeypatch):
    """MMHandModel.set_input renders behind its own decode pass: raw batches and resident batches, plain and under
    --resize_inputs, give the decoded loader's tensors; a model without the flag refuses a batch without depth images"""
    from mmhand_amd import lib
    from mmhand_amd.mmhand_model import MMHandModel
    for kw, size in (({}, 32), ({"resize_inputs": 24}, 24)):
        with _without_depth(rhd_dir):
            want = _epoch(_loader(rhd_dir, dev, decoded=True, depth_source="joints", **kw))
            raw = _epoch(_loader(rhd_dir, dev, depth_source="joints", **kw))
            res = _loader(rhd_dir, dev, resident=True, depth_source="joints", **kw)
            _epoch(res)
            served = _epoch(res)
        assert all("resident" in b for b in served)
        model = MMHandModel(_opt(rhd_dir, depth_source="joints", **kw))
        calls = Counter()
        real = lib.call

        def spy(name, *a):
            calls[name] += 1
            return real(name, *a)
        monkeypatch.setattr(lib, "call", spy)
        for batches in (raw, served):
            for w, b in zip(want, batches):
                model.set_input(b)
                assert tuple(model.x_D.shape) == (len(w["H1_path"]), size, size, 8)
                for k in ("H1", "H2", "P1", "P2", "D1", "D2", "C1", "C2"):
                    assert torch.equal(getattr(model, "input_" + k), w[k]), k
                assert (model.x_D[..., 6:] == 0).all()
        assert calls["mmh_render_pose_depth"] == 6
        monkeypatch.setattr(lib, "call", real)
        assert np.array_equal(model.input_D1.cpu().numpy()[:, 0], R.render(model.input_C1.cpu().numpy(), size, size, 5.0))
        assert np.array_equal(model.input_D2.cpu().numpy()[:, 2], R.render(model.input_C2.cpu().numpy(), size, size, 5.0))
    plain = MMHandModel(_opt(rhd_dir))
    with pytest.raises(ValueError, match="depth_source"):
        plain.set_input(raw[0])
    no_c = {k: v for k, v in raw[0].items() if k not in ("C1", "C2")}
    with pytest.raises(ValueError, match="C1"):
        model.set_input(no_c)


def test_one_step_and_graph_step_on_rendered_depth(rhd_dir, dev, monkeypatch):
    """a training step on raw joints-mode batches runs, eagerly and replayed from the captured graph, with the same losses"""
    from mmhand_amd.mmhand_model import MMHandModel
    with _without_depth(rhd_dir):
        batches = [b for b in _epoch(_loader(rhd_dir, dev, depth_source="joints", batchSize=2)) if b["img1"].shape[0] == 2]
    out = []
    for capture in (False, True):
        monkeypatch.setenv("MMH_GRAPH_CAPTURE", "1" if capture else "0")
        random.seed(17)
        model = MMHandModel(_opt(rhd_dir, depth_source="joints", batchSize=2, graph_step=True, name="render_graph"))
        losses = []
        for it in range(6):
            model.set_input(batches[it % len(batches)])
            model.optimize_parameters()
            losses.append([float(v) for v in model.get_current_errors().values()])
        model._settle_overflow(drain=True)
        torch.cuda.synchronize()
        out.append((model, losses))
    assert out[1][0].graph_error is None and out[1][0].graph_replays >= 1
    assert np.isfinite(out[0][1]).all() and np.array_equal(np.array(out[0][1]), np.array(out[1][1]))


# ----------------------------------------------------------------------------- aug --novel
@pytest.fixture()
def aug_dir(monkeypatch):
    from mmhand_amd.networks import Generator
    d = tempfile.mkdtemp(prefix="mmh_rn_")
    root = os.path.join(d, "rhd")
    write_rhd(root, n=8, size=32)
    monkeypatch.chdir(d)
    torch.manual_seed(3)
    net = Generator(input_nc=[3, 42, 6], output_nc=3, ngf=8, norm_layer="batch", use_dropout=True, n_blocks=2)
    os.makedirs(os.path.join("checkpoints", "tiny"))
    torch.save(net.state_dict(), os.path.join("checkpoints", "tiny", "latest_net_netG.pth"))
    yield d, root
    shutil.rmtree(d, ignore_errors=True)


def _read_all(dst, names):
    return [open(os.path.join(dst, n), "rb").read() for n in names]


def test_aug_novel_writes_a_prepared_directory_twice_the_same_and_train_reads_it(dev, aug_dir):
    from PIL import Image

    from mmhand_amd import aug, evaluate, novel, train
    d, root = aug_dir
    ann = pickle.load(open(os.path.join(root, "annotation.pickle"), "rb"))["color"]
    targets = sorted(ann, key=lambda x: int(x[:-4]))[:4]                     # the generation split of ratio 0.5
    written = aug.main(["tiny", root, "nov", "rhd", "0.5", "0", "--novel", "2"], ngf=8, n_blocks=2)
    names = [f"{i:05d}.png" for i in range(8)]
    assert [os.path.relpath(p, "nov") for p in written] == [os.path.join("color", n) for n in names]
    assert sorted(os.listdir("nov")) == ["annotation.pickle", "color", "novel_index.json"]
    assert sorted(os.listdir(os.path.join("nov", "color"))) == names
    assert all(Image.open(p).size == (32, 32) for p in written)
    index = json.load(open(os.path.join("nov", "novel_index.json")))
    back = pickle.load(open(os.path.join("nov", "annotation.pickle"), "rb"))
    assert list(back) == ["color"] and list(back["color"]) == names
    assert [r["file"] for r in index] == names and [r["rank"] for r in index] == [1, 2] * 4
    assert [r["target"] for r in index] == [os.path.join("color", t) for t in targets for _ in range(2)]
    for r in index:
        assert set(r) == {"file", "target", "neighbour", "rank", "alpha", "pose_distance"} and r["alpha"] == 0.5
        t, nb = ann[os.path.basename(r["target"])], ann[os.path.basename(r["neighbour"])]
        assert r["neighbour"] != r["target"] and os.path.basename(r["neighbour"]) in targets      # --match_pool self
        uv, depth = novel.blend(t["uv_coord"], t["depth"], nb["uv_coord"], nb["depth"], 0.5)
        assert np.array_equal(np.float64(back["color"][r["file"]]["uv_coord"]), uv)
        assert np.array_equal(np.float64(back["color"][r["file"]]["depth"]), depth)
    assert all(index[2 * i]["pose_distance"] <= index[2 * i + 1]["pose_distance"] for i in range(4))
    # a second run writes the same bytes
    aug.main(["tiny", root, "nov2", "rhd", "0.5", "0", "--novel", "2"], ngf=8, n_blocks=2)
    files = ["annotation.pickle", "novel_index.json"] + [os.path.join("color", n) for n in names]
    assert _read_all("nov", files) == _read_all("nov2", files)
    # the pool of the training share, rendered D1, other radius, resized, batched, written by the device: composes
    with _without_depth(root):
        w3 = aug.main(["tiny", root, "nov3", "rhd", "0.5", "0", "--novel", "3", "--novel_alpha", "0.25", "--match_pool", "train",
                       "--depth_source", "joints", "--render_radius", "3", "--resize_inputs", "24", "--batch", "5", "--device_png"],
                      ngf=8, n_blocks=2)
        # evaluate takes the flag too: the generator scored on the generation split without a depth file
        evaluate.main(["--name", "tiny", "--dataroot", root, "--dataset", "rhd", "--augmentation_ratio", "0.5", "--batchSize", "3",
                       "--depth_source", "joints", "--results_json", "ev.json"])
    ev = json.load(open("ev.json"))
    assert ev["summary"]["n"] == 4 and ev["options"]["depth_source"] == "joints" and np.isfinite(ev["summary"]["SSIM_avg"])
    assert len(w3) == 12 and all(Image.open(p).size == (24, 24) for p in w3)
    idx3 = json.load(open(os.path.join("nov3", "novel_index.json")))
    back3 = pickle.load(open(os.path.join("nov3", "annotation.pickle"), "rb"))["color"]
    assert all(os.path.basename(r["neighbour"]) not in targets for r in idx3)
    r = idx3[4]
    uv, _ = novel.blend(ann[os.path.basename(r["target"])]["uv_coord"], ann[os.path.basename(r["target"])]["depth"],
                        ann[os.path.basename(r["neighbour"])]["uv_coord"], ann[os.path.basename(r["neighbour"])]["depth"], 0.25)
    assert np.array_equal(np.float64(back3[r["file"]]["uv_coord"]), (uv + 0.5) * 24.0 / 32.0 - 0.5)
    # one training iteration on the written directory
    train.main(["--name", "on_novel", "--dataroot", os.path.join(d, "nov"), "--dataset", "rhd", "--augmentation_ratio", "1.0",
                "--depth_source", "joints", "--batchSize", "2", "--max_dataset_size", "1", "--ngf", "8", "--ndf", "8",
                "--G_n_blocks", "2", "--n_layers_D", "2", "--norm", "batch", "--niter", "1", "--niter_decay", "0", "--print_freq", "2",
                "--vgg_random_init", "--checkpoints_dir", "checkpoints", "--pool_size", "2"])
    log = open(os.path.join("checkpoints", "on_novel", "loss_log.txt")).read()
    assert "pair_L1loss" in log and os.path.isfile(os.path.join("checkpoints", "on_novel", "latest_net_netG.pth"))
