"""Pose-distance pairing, the part that needs no GPU: the numpy oracle against the reference's recorded distances
(tests/golden/pose_distance.npz, written by tests/golden/make_pose_distance.py), the four entry points' declarations and argument
checks, the workspace bound, the host helpers of data.py, the loader's curriculum shard and the selection header's host check."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests._pose_oracle import oracle_distance, oracle_features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def built_lib():
    from mmhand_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mmhand_amd", "csrc")])
    return lib


def test_oracle_equals_the_reference_off_the_diagonal():
    z = np.load(os.path.join(G, "pose_distance.npz"))
    poses, want = z["poses"], z["distance"]
    assert poses.shape == (24, 21, 3) and want.shape == (24, 24) and poses.dtype == want.dtype == np.float64
    f = oracle_features(poses)
    got = oracle_distance(f @ f.T)
    off = ~np.eye(24, dtype=bool)
    assert np.isfinite(want[off]).all() and want[off].min() > 0.05          # real distances, not a degenerate fixture
    assert np.abs(got - want)[off].max() <= 1e-14
    # the stated divergence: on the diagonal the reference gives 0 or NaN (a cosine rounded above 1); the clamp gives ~0
    assert np.all(np.isnan(np.diag(want)) | (np.diag(want) < 1e-7)) and np.all(np.diag(got) < 1e-7)


def test_abi_declares_and_validates_the_pose_entry_points(built_lib):
    names = {"mmh_pose_features": 5, "mmh_pose_knn_ws_bytes": 4, "mmh_pose_knn": 13, "mmh_pose_pair_distance": 7}
    hdr = open(os.path.join(ROOT, "include", "mmhand_hip.h")).read()
    for name, n_args in names.items():
        assert len(built_lib.SIGNATURES[name][1]) == n_args
        assert name + "(" in hdr
    assert hdr.count("nearest_neighbor_search.py:68-83") >= 4
    l = built_lib.load()
    one = ctypes.c_void_p(4096)         # a non-null, aligned address: every call below is refused before anything reads it

    def refused(rc):
        assert rc != 0
        msg = l.mmh_last_error()
        assert b"pose_knn" in msg, msg
        return msg

    refused(l.mmh_pose_features(None, 4, one, one, None))
    refused(l.mmh_pose_features(one, 4, None, one, None))
    refused(l.mmh_pose_features(one, 0, one, one, None))
    good = dict(Fq=one, vq=one, Nq=4, Fc=one, vc=one, Nc=8, ex=None, k=2, split=0, ws=one, idx=one, dist=one)

    def knn(**kw):
        a = dict(good, **kw)
        return l.mmh_pose_knn(a["Fq"], a["vq"], a["Nq"], a["Fc"], a["vc"], a["Nc"], a["ex"], a["k"], a["split"], a["ws"], a["idx"],
                              a["dist"], None)

    for key in ("Fq", "vq", "Fc", "vc", "ws", "idx", "dist"):
        assert b"NULL" in refused(knn(**{key: None}))
    refused(knn(Nq=0))
    refused(knn(Nc=0))
    for k in (0, -1, 17):
        assert b"k = " in refused(knn(k=k))
    for split in (8, 17, -16):
        assert b"cand_split" in refused(knn(split=split))
    refused(l.mmh_pose_pair_distance(None, one, one, one, 3, one, None))
    refused(l.mmh_pose_pair_distance(one, one, one, one, 0, one, None))
    refused(l.mmh_pose_pair_distance(one, one, one, one, 3, None, None))
    for bad in ((0, 8, 1, 0), (8, 0, 1, 0), (8, 8, 0, 0), (8, 8, 17, 0), (8, 8, 1, 24)):
        assert l.mmh_pose_knn_ws_bytes(*bad) == 0


def test_workspace_bound(built_lib):
    """at most slices * Nq * k * 12 bytes plus alignment: 32 slices at most when the split is automatic"""
    l = built_lib.load()
    n = 41258
    full = l.mmh_pose_knn_ws_bytes(n, n, 16, 0)
    assert 0 < full <= 32 * n * 16 * 12 + 256
    assert full >= n * 16 * 12
    # a small query set is cut into more slices, never more than 32; an explicit split gives ceil(Nc / split) slices
    small = l.mmh_pose_knn_ws_bytes(33, n, 16, 0)
    assert 33 * 16 * 12 <= small <= 32 * 33 * 16 * 12 + 256
    assert l.mmh_pose_knn_ws_bytes(130, 1500, 8, 16) == -(-(94 * 130 * 8 * 12) // 256) * 256
    assert l.mmh_pose_knn_ws_bytes(130, 1500, 8, 64) == -(-(24 * 130 * 8 * 12) // 256) * 256


def test_curriculum_order_is_stable_with_nan_last():
    from mmhand_amd.data import curriculum_order
    nan = float("nan")
    d = [0.5, 0.25, nan, 0.5, 0.0, 0.25, nan, 0.5]
    order = curriculum_order(d)
    assert order.tolist() == [4, 1, 5, 0, 3, 7, 2, 6]
    assert curriculum_order([]).tolist() == [] and curriculum_order([nan, nan]).tolist() == [0, 1]
    assert curriculum_order(np.array([1.0, 1.0, 1.0])).tolist() == [0, 1, 2]
    rs = np.random.RandomState(0)
    x = np.round(rs.uniform(0, 1, 200), 1)
    assert curriculum_order(x).tolist() == np.argsort(x, kind="stable").tolist()


def test_apply_nearest_keeps_the_random_source_where_there_is_no_neighbour():
    from mmhand_amd.data import apply_nearest
    src, pool = ["s0", "s1", "s2", "s3"], ["p0", "p1", "p2"]
    out, fb = apply_nearest(src, pool, np.array([2, -1, 0, -1], dtype=np.int32))
    assert out == ["p2", "s1", "p0", "s3"] and fb == [1, 3] and src == ["s0", "s1", "s2", "s3"]
    out, fb = apply_nearest(src, pool, np.array([[1], [1], [2], [0]], dtype=np.int32))            # pose_knn's [n, k]
    assert out == ["p1", "p1", "p2", "p0"] and fb == []
    with pytest.raises(ValueError):
        apply_nearest(src, pool, np.array([0, 1, 2], dtype=np.int32))
    with pytest.raises(ValueError):
        apply_nearest(src, pool, np.array([0, 1, 2, 3], dtype=np.int32))


@pytest.mark.parametrize("world,n", [(2, 7), (3, 7), (3, 6), (3, 1)])
def test_indices_under_curriculum_are_the_padded_range_rank_strided(world, n):
    """all ranks step through the same difficulty together: rank r takes r, r + world, ... of the padded range, no permutation"""
    from mmhand_amd.data import HandFolderLoader
    total = -(-n // world) * world
    padded = list(range(n)) + [i % n for i in range(total - n)]
    seen = []
    for rank in range(world):
        ld = HandFolderLoader.__new__(HandFolderLoader)
        ld.image_source, ld.world, ld.rank, ld.epoch, ld.pairing = ["x"] * n, world, rank, 0, "curriculum"
        idx = ld.indices()
        assert idx == padded[rank::world] and len(idx) == total // world
        seen.append(idx)
    assert sorted(i for s in seen for i in s) == sorted(padded)
    # the random mode keeps DistributedSampler's permutation (seed 0)
    import torch
    ld.pairing = "random"
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(0)).tolist()
    assert ld.indices() == (perm + (perm * world)[:total - n])[world - 1:total:world]


def test_pairing_flags():
    from mmhand_amd.data import check_pairing
    from mmhand_amd.options import TrainOptions, default_train_opt
    assert check_pairing(default_train_opt()) == ("random", "self")
    o = TrainOptions()
    o.initialize()
    opt = o.parser.parse_args(["--pairing", "curriculum", "--match_pool", "train"])
    assert check_pairing(opt) == ("curriculum", "train")
    with pytest.raises(SystemExit):
        o.parser.parse_args(["--pairing", "kdtree"])
    with pytest.raises(ValueError):
        check_pairing(default_train_opt(pairing="kdtree"))
    from mmhand_amd import evaluate
    args = evaluate.build_parser().parse_args(["--generated", "g", "--dataroot", "d", "--dataset", "rhd"])
    assert args.pairing is None and args.match_pool is None
    args = evaluate.build_parser().parse_args(["--generated", "g", "--dataroot", "d", "--dataset", "rhd", "--pairing", "nearest"])
    assert args.pairing == "nearest"


def test_pose_topk_host_check_builds_and_passes():
    """the selection header of pose_knn.hip under ASan + UBSan on the host: a stand-alone program against std::sort"""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "mmhand_amd", "csrc"), "pose_topk_host_check"], capture_output=True,
                         text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pose_topk_host_check: ok" in out.stdout
