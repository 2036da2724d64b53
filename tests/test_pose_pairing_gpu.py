"""Pose-distance pairing on the device: ops.pose_features / pose_knn / pose_pair_distance (csrc/pose_knn.hip) against the float64
numpy oracle of tests/_pose_oracle.py (itself checked against the reference in tests/test_pose_pairing_cpu.py), the loader's
curriculum and nearest modes, and `aug` / `evaluate` under --pairing.

Indices must match the oracle EXACTLY: the rounding of a 64-term fp64 chain is <= 1e-14, and every test first asserts on the
CPU that neighbouring oracle cosines inside the top k + 1 differ by at least 1e-9 (constructed exact duplicates aside), so no
ranking is decided by rounding.  Distances: within 1e-12 where the oracle cosine is <= 0.999, within 1e-7 elsewhere (arccos is
ill-conditioned at 1)."""
import csv
import json
import os
import random
import shutil
import tempfile
from collections import Counter

import numpy as np
import pytest
import torch

from tests import _dataset_fixture as F
from tests._pose_oracle import draw_poses, oracle_distance, oracle_features, oracle_knn, oracle_valid

pytestmark = pytest.mark.gpu

MIN_GAP = 1e-9


def _features(ops, poses, dev):
    return ops.pose_features(torch.from_numpy(np.ascontiguousarray(poses)).to(dev))


def _assert_gaps(ranked, k, allow_zero=False):
    """neighbouring oracle cosines inside every query's top k + 1 are at least MIN_GAP apart (exact ties only when constructed)"""
    worst = np.inf
    for r in ranked:
        gaps = -np.diff(r[:k + 1])
        if allow_zero:
            gaps = gaps[gaps != 0.0]
        if len(gaps):
            worst = min(worst, gaps.min())
    assert worst >= MIN_GAP, worst
    return worst


def _assert_knn(idx, dist, want_idx, want_cos):
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert idx.dtype == np.int32 and dist.dtype == np.float64 and idx.shape == dist.shape == want_idx.shape
    assert np.array_equal(idx, want_idx), np.argwhere(idx != want_idx)[:5]
    empty = want_idx < 0
    assert np.isnan(dist[empty]).all() and np.isfinite(dist[~empty]).all()
    err = np.abs(dist - oracle_distance(want_cos))[~empty]
    easy = want_cos[~empty] <= 0.999
    assert (err[easy] <= 1e-12).all(), err[easy].max()
    assert (err[~easy] <= 1e-7).all(), err[~easy].max()


@pytest.fixture(scope="module")
def big():
    """130 queries against 1500 OTHER poses (a row / column swap cannot pass), the oracle ranking once for k = 16"""
    q, c = draw_poses(130, seed=21), draw_poses(1500, seed=22)
    idx, cos, ranked = oracle_knn(q, c, 16)
    return q, c, idx, cos, ranked


def test_pose_features_match_the_oracle(dev):
    from mmhand_amd import ops
    poses = draw_poses(37, seed=4)
    poses[7] = poses[7][:1]                      # every joint at one point: zero norm
    poses[9, 3, 1] = np.nan
    poses[11, 20, 2] = np.inf
    f, valid = _features(ops, poses, dev)
    f, valid = f.cpu().numpy(), valid.cpu().numpy()
    assert f.shape == (37, 64) and valid.dtype == np.int32
    want_valid = oracle_valid(poses)
    assert want_valid.sum() == 34 and np.array_equal(valid != 0, want_valid)
    assert (f[:, 60:] == 0).all() and (f[~want_valid] == 0).all()
    assert np.abs(f[want_valid, :60] - oracle_features(poses[want_valid])).max() <= 1e-15


@pytest.mark.parametrize("nq,nc,k", [(1, 2, 1), (17, 33, 3)])
def test_knn_small_shapes_match_the_oracle(nq, nc, k, dev):
    """one tile with two candidates; ragged 16-tiles on both sides"""
    from mmhand_amd import ops
    q, c = draw_poses(nq, seed=31), draw_poses(nc, seed=32)
    want_idx, want_cos, ranked = oracle_knn(q, c, k)
    _assert_gaps(ranked, k)
    idx, dist = ops.pose_knn(_features(ops, q, dev), _features(ops, c, dev), k)
    _assert_knn(idx, dist, want_idx, want_cos)


@pytest.mark.parametrize("split", [0, 16, 64])
@pytest.mark.parametrize("k", [8, 16])
def test_knn_matches_the_oracle_for_every_split(k, split, big, dev):
    """several query workgroups, one slice (0), 94 slices of one tile (16) and 24 slices of one tile per wave (64)"""
    from mmhand_amd import ops
    q, c, want_idx, want_cos, ranked = big
    _assert_gaps(ranked, k)
    idx, dist = ops.pose_knn(_features(ops, q, dev), _features(ops, c, dev), k, cand_split=split)
    _assert_knn(idx, dist, want_idx[:, :k], want_cos[:, :k])


def test_knn_is_bit_identical_for_any_split(big, dev):
    from mmhand_amd import ops
    q, c, *_ = big
    fq, fc = _features(ops, q, dev), _features(ops, c, dev)
    ref_idx, ref_dist = ops.pose_knn(fq, fc, 16, cand_split=0)
    for split in (16, 64):
        idx, dist = ops.pose_knn(fq, fc, 16, cand_split=split)
        assert torch.equal(idx, ref_idx) and torch.equal(dist.view(torch.int64), ref_dist.view(torch.int64)), split


def test_knn_ties_exclusion_and_invalid_poses(dev):
    from mmhand_amd import ops
    poses = draw_poses(50, seed=41)
    poses[40] = poses[5]
    poses[41] = poses[5]
    poses[7] = poses[7][:1]                      # zero norm
    poses[9, 0, 0] = np.nan
    f = _features(ops, poses, dev)
    k = 4
    # without exclusion: the three identical poses come back first, in index order, at distance ~0
    want_idx, want_cos, ranked = oracle_knn(poses, poses, k)
    _assert_gaps(ranked, k, allow_zero=True)
    idx, dist = ops.pose_knn(f, f, k)
    got = idx.cpu().numpy()
    for q in (5, 40, 41):
        assert got[q, :3].tolist() == [5, 40, 41]
        assert (dist[q, :3].cpu().numpy() <= 1e-7).all()
    plain = [q for q in range(50) if q not in (5, 40, 41)]
    _assert_knn(idx[plain], dist[plain], want_idx[plain], want_cos[plain])
    assert not np.isin(got, (7, 9)).any()
    for q in (7, 9):                             # as queries: nothing
        assert (got[q] == -1).all() and torch.isnan(dist[q]).all()
    # exclusion removes the self match (and only it)
    ex = np.arange(50, dtype=np.int32)
    want_idx, want_cos, ranked = oracle_knn(poses, poses, k, exclude=ex)
    idx, dist = ops.pose_knn(f, f, k, exclude=torch.from_numpy(ex).to(dev))
    got = idx.cpu().numpy()
    assert got[5, :2].tolist() == [40, 41] and got[40, :2].tolist() == [5, 41] and got[41, :2].tolist() == [5, 40]
    assert all(q not in got[q] for q in range(50))
    _assert_knn(idx[plain], dist[plain], want_idx[plain], want_cos[plain])
    # k larger than the number of valid candidates: trailing -1 / NaN
    few = poses[[0, 7, 1, 9, 2, 3]]
    want_idx, want_cos, ranked = oracle_knn(poses[10:13], few, 8)
    assert (want_idx[:, 4:] == -1).all() and (want_idx[:, :4] >= 0).all()
    idx, dist = ops.pose_knn(_features(ops, poses[10:13], dev), _features(ops, few, dev), 8)
    _assert_knn(idx, dist, want_idx, want_cos)


def test_pose_pair_distance_matches_the_oracle(dev):
    from mmhand_amd import ops
    a, b = draw_poses(70, seed=51), draw_poses(70, seed=52)
    b[3] = a[3]                                  # cosine 1
    b[4] = a[4] + 1e-3 * draw_poses(1, seed=53)[0]          # cosine above 0.999
    a[6, 2, 2] = np.nan
    b[8] = b[8][:1]
    d = ops.pose_pair_distance(_features(ops, a, dev), _features(ops, b, dev)).cpu().numpy()
    ok = oracle_valid(a) & oracle_valid(b)
    assert ok.sum() == 68 and np.isnan(d[~ok]).all()
    cos = (np.nan_to_num(oracle_features(a)) * np.nan_to_num(oracle_features(b))).sum(1)
    err = np.abs(d - oracle_distance(cos))
    easy = ok & (cos <= 0.999)
    hard = ok & (cos > 0.999)
    assert hard.sum() >= 2 and (err[easy] <= 1e-12).all() and (err[hard] <= 1e-7).all()


# ----------------------------------------------------------------------------- the loader
@pytest.fixture
def data_dir():
    """a directory without "test" in its path (such a root serves generation only)"""
    d = tempfile.mkdtemp(prefix="mmh_pose_")
    assert "test" not in d
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _opt(root, **kw):
    from mmhand_amd.options import default_train_opt
    kw.setdefault("augmentation_ratio", 1.0)
    return default_train_opt(batchSize=5, dataroot=root, dataset="rhd", nThreads=2, **kw)


def _loader(opt, dev, seed=5, **kw):
    from mmhand_amd.data import HandFolderLoader
    random.seed(seed)
    return HandFolderLoader(opt, device=dev, **kw)


def _pair_oracle(ld):
    """oracle pose distance of the loader's pairs, in its order"""
    s = oracle_features(np.stack([ld.pose_of(p) for p in ld.image_source]))
    t = oracle_features(np.stack([ld.pose_of(p) for p in ld.image_target]))
    return oracle_distance((s * t).sum(1))


class _Spy:
    def __init__(self, monkeypatch):
        from mmhand_amd import lib
        self.calls = Counter()
        real = lib.call

        def call(name, *a):
            self.calls[name] += 1
            return real(name, *a)

        monkeypatch.setattr(lib, "call", call)


def _by_pair(batches):
    out = {}
    for b in batches:
        for i, (h1, h2) in enumerate(zip(b["H1_path"], b["H2_path"])):
            out[(h1, h2)] = {k: b[k][i].clone() for k in ("H1", "H2", "P1", "P2", "D1", "D2", "C1", "C2")}
    return out


def test_loader_curriculum_reorders_the_random_pairs(dev, data_dir, monkeypatch):
    from mmhand_amd.data import curriculum_order
    F.write_rhd(data_dir, n=23, size=32)
    spy = _Spy(monkeypatch)
    rnd = _loader(_opt(data_dir), dev, decoded=True)
    assert rnd.pairing == "random" and not spy.calls            # the default path launches nothing new
    cur = _loader(_opt(data_dir, pairing="curriculum"), dev, decoded=True)
    assert spy.calls["mmh_pose_pair_distance"] >= 1
    pairs_r, pairs_c = list(zip(rnd.image_source, rnd.image_target)), list(zip(cur.image_source, cur.image_target))
    assert len(pairs_c) == 23 and sorted(pairs_r) == sorted(pairs_c) and pairs_r != pairs_c
    want = _pair_oracle(cur)
    # ascending; no order is decided by rounding: a gap is at least 1e-9 or exactly 0 (the mirrored pairs (a, b), (b, a) of a
    # 2-cycle of the shuffle), and ties keep their original order
    gaps = np.diff(want)
    assert (gaps >= 0).all() and gaps[gaps != 0].min() >= 1e-9
    assert pairs_c == [pairs_r[i] for i in curriculum_order(_pair_oracle(rnd))]
    assert cur.pair_distance.dtype == np.float64 and np.abs(cur.pair_distance - want).max() <= 1e-12
    # random mode: the same quantity, on first access only
    assert spy.calls["mmh_pose_features"] == 2
    d_r = rnd.pair_distance
    assert spy.calls["mmh_pose_features"] == 4 and np.abs(d_r - _pair_oracle(rnd)).max() <= 1e-12
    assert sorted(d_r.tolist()) == cur.pair_distance.tolist()
    # a pair's decoded sample does not depend on where the curriculum put it
    a, b = _by_pair(rnd), _by_pair(cur)
    assert set(a) == set(b) == set(pairs_r)
    for key in a:
        for k, v in a[key].items():
            assert torch.equal(v, b[key][k]), (key, k)


def test_loader_nearest_takes_the_closest_pose(dev, data_dir):
    F.write_rhd(data_dir, n=23, size=32)
    ld = _loader(_opt(data_dir, pairing="nearest"), dev)
    poses = np.stack([ld.pose_of(p) for p in ld.image_target])
    want_idx, want_cos, ranked = oracle_knn(poses, poses, 1, exclude=np.arange(23))
    _assert_gaps(ranked, 1)
    assert ld.image_source == [ld.image_target[j] for j in want_idx[:, 0]] and ld.pairing_fallbacks == []
    assert np.abs(ld.pair_distance - oracle_distance(want_cos[:, 0])).max() <= 1e-12
    assert all(s != t for s, t in zip(ld.image_source, ld.image_target))
    # --resize_inputs does not move the pairing
    again = _loader(_opt(data_dir, pairing="nearest", resize_inputs=48), dev)
    assert again.image_source == ld.image_source

    # match_pool train: a generation split (the first 11 of 23) draws from the training share (the other 12)
    gen = _loader(_opt(data_dir, pairing="nearest", match_pool="train", augmentation_ratio=0.5, isTrain=False), dev)
    everything = sorted(ld.image_target, key=lambda x: int(os.path.basename(x)[:-4]))
    assert gen.image_target == everything[:11]
    pool = everything[11:]
    want_idx, want_cos, ranked = oracle_knn(np.stack([gen.pose_of(p) for p in gen.image_target]),
                                            np.stack([gen.pose_of(p) for p in pool]), 1)
    _assert_gaps(ranked, 1)
    assert gen.image_source == [pool[j] for j in want_idx[:, 0]] and set(gen.image_source) <= set(pool)
    assert np.abs(gen.pair_distance - oracle_distance(want_cos[:, 0])).max() <= 1e-12
    with pytest.raises(ValueError, match="no training share"):
        _loader(_opt(data_dir, pairing="nearest", match_pool="train", augmentation_ratio=0.0, isTrain=False), dev)
    troot = os.path.join(data_dir, "test_rhd")
    F.write_rhd(troot, n=5, size=32)
    with pytest.raises(ValueError, match="'test' directory"):
        _loader(_opt(troot, pairing="nearest", match_pool="train", augmentation_ratio=0.5, isTrain=False), dev)


def test_loader_nearest_falls_back_where_there_is_no_neighbour(dev, data_dir):
    """two degenerate poses (every joint at one point) among four: as targets they have no neighbour and keep their random
    source; as candidates they are never chosen"""
    import pickle
    names = F.write_rhd(data_dir, n=4, size=32)
    ordered = sorted(names, key=lambda x: int(x[:-4]))
    with open(os.path.join(data_dir, "annotation.pickle"), "rb") as fh:
        ann = pickle.load(fh)
    for name in (ordered[0], ordered[3]):
        for folder in ann:
            ann[folder][name] = {"uv_coord": [[3.0, 3.0]] * 21, "depth": [200.0] * 21}
    with open(os.path.join(data_dir, "annotation.pickle"), "wb") as fh:
        pickle.dump(ann, fh)
    rnd = _loader(_opt(data_dir), dev)
    ld = _loader(_opt(data_dir, pairing="nearest"), dev)
    assert ld.pairing_fallbacks == [0, 3]
    assert [ld.image_source[i] for i in (0, 3)] == [rnd.image_source[i] for i in (0, 3)]
    assert ld.image_source[1] == ld.image_target[2] and ld.image_source[2] == ld.image_target[1]
    d = ld.pair_distance
    assert np.isnan(d[[0, 3]]).all() and np.isfinite(d[[1, 2]]).all() and d[1] == d[2]


def test_loader_curriculum_with_the_resident_store(dev, data_dir):
    F.write_rhd(data_dir, n=23, size=32)
    ld = _loader(_opt(data_dir, pairing="curriculum"), dev, decoded=True, resident=True)
    assert ld.resident_state.startswith("on")
    first = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()} for b in ld]
    second = list(ld)
    assert len(first) == len(second) == 5
    for b1, b2 in zip(first, second):
        assert set(b1) == set(b2)
        for k in b1:
            assert torch.equal(b1[k], b2[k]) if torch.is_tensor(b1[k]) else b1[k] == b2[k], k
    paths = [(h1, h2) for b in second for h1, h2 in zip(b["H1_path"], b["H2_path"])]
    assert paths == list(zip(ld.image_source, ld.image_target))


# ----------------------------------------------------------------------------- aug and evaluate
def test_aug_and_evaluate_under_pairing(dev, data_dir, monkeypatch):
    """as test_model_gpu.test_train_and_aug_run_on_files, on a small checkpoint written directly"""
    from mmhand_amd import aug, evaluate
    from mmhand_amd.networks import Generator
    root = os.path.join(data_dir, "rhd")
    names = F.write_rhd(root, n=8, size=32)
    monkeypatch.chdir(data_dir)
    torch.manual_seed(3)
    net = Generator(input_nc=[3, 42, 6], output_nc=3, ngf=8, norm_layer="batch", use_dropout=True, n_blocks=2)
    os.makedirs(os.path.join("checkpoints", "tiny"))
    torch.save(net.state_dict(), os.path.join("checkpoints", "tiny", "latest_net_netG.pth"))
    random.seed(2)
    plain = aug.main(["tiny", root, "gen_plain", "rhd", "0.5", "0"], ngf=8, n_blocks=2)
    random.seed(2)
    near = aug.main(["tiny", root, "gen_near", "rhd", "0.5", "0", "--pairing", "nearest"], ngf=8, n_blocks=2)
    ordered = sorted(names, key=lambda x: int(x[:-4]))
    assert [os.path.relpath(p, "gen_near") for p in near] == [os.path.join("color", n) for n in ordered[:4]]
    assert [os.path.relpath(p, "gen_plain") for p in plain] == [os.path.relpath(p, "gen_near") for p in near]
    with pytest.raises(ValueError):
        aug.main(["tiny", root, "gen_bad", "rhd", "0.5", "0", "--pairing", "kdtree"], ngf=8, n_blocks=2)

    common = ["--dataroot", root, "--dataset", "rhd", "--augmentation_ratio", "0.5", "--batchSize", "3"]
    random.seed(2)
    evaluate.main(["--generated", "gen_plain", "--results_json", "plain.json", "--per_image_csv", "plain.csv"] + common)
    random.seed(2)
    evaluate.main(["--generated", "gen_near", "--pairing", "nearest", "--results_json", "near.json", "--per_image_csv", "near.csv"]
                  + common)
    plain_json, near_json = json.load(open("plain.json")), json.load(open("near.json"))
    assert set(plain_json) == set(near_json) == {"summary", "options", "generator", "domain"}
    assert set(plain_json["summary"]) == {"SSIM_avg", "SSIM_std", "L1_avg", "PSNR_avg", "n"}
    assert "pairing" not in plain_json["options"] and "match_pool" not in plain_json["options"]
    assert set(near_json["summary"]) == set(plain_json["summary"]) | {"pairing", "pose_distance_avg"}
    assert near_json["summary"]["pairing"] == "nearest" and near_json["options"]["pairing"] == "nearest"
    rows_p, rows_n = list(csv.reader(open("plain.csv"))), list(csv.reader(open("near.csv")))
    assert rows_p[0] == ["target", "source", "ssim", "l1", "psnr"] and rows_n[0] == rows_p[0] + ["pose_distance"]
    assert len(rows_p) == len(rows_n) == 5
    # the oracle: every target of the generation share against the share's other poses
    import pickle
    with open(os.path.join(root, "annotation.pickle"), "rb") as fh:
        ann = pickle.load(fh)["color"]
    poses = np.stack([np.concatenate([np.asarray(ann[n]["uv_coord"], dtype=np.float64).reshape(21, 2),
                                      np.expand_dims(np.asarray(ann[n]["depth"], dtype=np.float64), -1) / 700.0 * 255], -1)
                      for n in ordered[:4]])
    want_idx, want_cos, ranked = oracle_knn(poses, poses, 1, exclude=np.arange(4))
    _assert_gaps(ranked, 1)
    want = oracle_distance(want_cos[:, 0])
    assert abs(near_json["summary"]["pose_distance_avg"] - want.mean()) <= 1e-12
    for row, n, j, d in zip(rows_n[1:], ordered[:4], want_idx[:, 0], want):
        assert os.path.basename(row[0]) == n and os.path.basename(row[1]) == ordered[j] and abs(float(row[5]) - d) <= 1e-12
