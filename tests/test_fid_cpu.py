"""The FID / KID feature's host side: the premises of the test oracle (tests/_fid_oracle.py), mmhand_amd.fid's float64 host
arithmetic (frechet_distance, kid_from_sums, draw_subsets, the statistics files), the ABI of the two new entry points and the
argument handling of mmhand_amd/evaluate.py.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _fid_oracle as FO
from tests import _inception_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mmh_feature_moments_ws_bytes", "mmh_feature_moments", "mmh_poly_mmd_sums_ws_bytes", "mmh_poly_mmd_sums")
# (N1, N2, d): two full-rank pairs and a rank-deficient one (fewer rows than features - what an evaluation split gives at d = 2048)
FULL_RANK, DEFICIENT = [(200, 150, 16), (300, 300, 128)], (40, 30, 64)


def _pair(n1, n2, d, seed=0):
    """two sets of non-negative correlated features of different means and scales"""
    rng = np.random.RandomState(seed)
    mix = rng.randn(d, d) / np.sqrt(d)
    X = np.abs(rng.randn(n1, d) @ mix + 0.3)
    Y = np.abs(rng.randn(n2, d) @ mix.T * 1.3 + 0.5)
    return X.astype(np.float32).astype(np.float64), Y.astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------- oracle premises
def test_np_cov_agrees_with_the_longdouble_form():
    X, _ = _pair(63, 5, 20)
    mean, cov, S = FO.moments(X)
    assert np.abs(mean - X.mean(0)).max() <= 4 * 2.0 ** -53 * X.max()
    assert (np.abs(cov - np.cov(X, rowvar=False)) <= 4 * (63 + 8) * 2.0 ** -53 * S / 62).all()
    assert np.array_equal(cov, cov.T)
    # the exact form on dyadic integers: one value, whatever the arithmetic
    Xi = FO.dyadic_features(16, 20, 3)
    m1, c1 = FO.moments_exact(Xi)
    m2, c2, _ = FO.moments(Xi)
    assert np.array_equal(m1, m2) and np.abs(c1 - c2).max() <= 2.0 ** -52 * np.abs(c1).max()
    assert np.array_equal(m1, np.round(m1)) and Xi.dtype == np.float32 and Xi.min() >= 0


@pytest.mark.parametrize("n1,n2,d", FULL_RANK)
def test_frechet_distance_on_full_rank_pairs(n1, n2, d):
    """the symmetric route, the nuclear norm and scipy's sqrtm give one value to 1e-13 relative"""
    from mmhand_amd import fid
    X, Y = _pair(n1, n2, d)
    mu1, s1, mu2, s2 = X.mean(0), np.cov(X, rowvar=False), Y.mean(0), np.cov(Y, rowvar=False)
    got, nuc, sq = fid.frechet_distance(mu1, s1, mu2, s2), FO.frechet_nuclear(X, Y), FO.frechet_sqrtm(mu1, s1, mu2, s2)
    print("d=%d: tr_sqrt %.15e, nuclear %.15e, sqrtm %.15e" % (d, got["tr_sqrt"], nuc["tr_sqrt"], sq["tr_sqrt"]))
    assert abs(got["tr_sqrt"] - nuc["tr_sqrt"]) <= 1e-13 * nuc["tr_sqrt"]
    assert abs(got["tr_sqrt"] - sq["tr_sqrt"]) <= 1e-13 * sq["tr_sqrt"]
    assert abs(got["fid"] - nuc["fid"]) <= 1e-13 * (np.trace(s1) + np.trace(s2))
    assert got["fid"] == got["mean_term"] + got["trace_term"] and got["mean_term"] == float((mu1 - mu2) @ (mu1 - mu2)) and got["fid"] > 0
    # a set against itself: the trace term vanishes
    own = fid.frechet_distance(mu1, s1, mu1, s1)
    assert own["mean_term"] == 0.0 and abs(own["fid"]) <= 1e-13 * np.trace(s1)


def test_frechet_distance_on_a_rank_deficient_pair():
    """N1 = 40, N2 = 30, d = 64: the covariances have null spaces; the thresholded symmetric route is no farther from the
    nuclear-norm value than scipy's sqrtm trace is on the same matrices (absolute distances on this pair, tr sqrt = 17.586, recorded in
    DESIGN 4.5k: 3.6e-15 and 2.9e-7; without the threshold the symmetric route is 9.9e-8 off)"""
    from mmhand_amd import fid
    X, Y = _pair(*DEFICIENT)
    mu1, s1, mu2, s2 = X.mean(0), np.cov(X, rowvar=False), Y.mean(0), np.cov(Y, rowvar=False)
    nuc = FO.frechet_nuclear(X, Y)["tr_sqrt"]
    mine = abs(fid.frechet_distance(mu1, s1, mu2, s2)["tr_sqrt"] - nuc)
    theirs = abs(FO.frechet_sqrtm(mu1, s1, mu2, s2)["tr_sqrt"] - nuc)
    print("rank-deficient pair: |symmetric - nuclear| = %.3e, |sqrtm - nuclear| = %.3e, tr_sqrt = %.6e" % (mine, theirs, nuc))
    assert mine <= theirs


# ------------------------------------------------------------------------------------------------- KID on the host
def test_kid_from_sums_is_the_direct_mmd():
    from mmhand_amd import fid
    X, Y = _pair(23, 17, 20, seed=2)
    ia, ib = np.stack([np.arange(23), np.arange(23)[::-1]]), np.stack([np.arange(17), np.roll(np.arange(17), 3)])
    k = fid.kid_from_sums(FO.mmd_sums(X, Y, ia, ib), 23, 17)
    want = FO.mmd2_unbiased(X, Y)
    assert k.shape == (2,) and abs(k[0] - want) <= 1e-13 * abs(want) + 1e-14 and abs(k[1] - want) <= 1e-13 * abs(want) + 1e-14
    # a repeated row is a pair of two positions
    rep = np.array([[0, 1, 0]])
    s = FO.mmd_sums(X, Y, rep, rep)
    assert s[0, 0] == pytest.approx(float(2 * (2 * FO.poly_kernel(X[:1], X[1:2]) + FO.poly_kernel(X[:1], X[:1]))[0, 0]), rel=1e-14)
    with pytest.raises(ValueError):
        fid.kid_from_sums(np.zeros((1, 3)), 1, 5)
    assert fid.kid_from_sums(np.array([[6.0, 2.0, 6.0]]), 3, 2)[0] == 6.0 / 6 + 2.0 / 2 - 2 * 6.0 / 6


def test_subsets_are_deterministic_and_clamped():
    from mmhand_amd import fid
    a, b = fid.draw_subsets(50, 30, subsets=7, subset_size=1000, seed=4)
    assert a.shape == b.shape == (7, 30) and a.dtype == b.dtype == np.int32                 # clamped to min(Na, Nb)
    a2, b2 = fid.draw_subsets(50, 30, subsets=7, subset_size=1000, seed=4)
    assert np.array_equal(a, a2) and np.array_equal(b, b2)
    assert not np.array_equal(a, fid.draw_subsets(50, 30, 7, 1000, seed=5)[0])
    for row in np.concatenate([a, b]):
        assert len(set(row.tolist())) == 30                                                  # without replacement
    assert a.max() < 50 and b.max() < 30 and (np.sort(b, 1) == np.arange(30)).all()
    rng = np.random.RandomState(4)                                                           # the documented stream
    assert np.array_equal(a[0], rng.choice(50, 30, replace=False)) and np.array_equal(b[0], rng.choice(30, 30, replace=False))
    assert fid.draw_subsets(50, 30, 2, 10, 0)[0].shape == (2, 10)
    with pytest.raises(ValueError):
        fid.draw_subsets(50, 30, 0, 10, 0)


def test_statistics_files_round_trip(tmp_path):
    from mmhand_amd import fid
    X, _ = _pair(12, 5, 8)
    mu, sigma = X.mean(0), np.cov(X, rowvar=False)
    p = str(tmp_path / "stats.npz")
    fid.save_stats(p, mu, sigma, 12, "fid", X.astype(np.float32))
    st = fid.load_stats(p)
    assert np.array_equal(st["mu"], mu) and np.array_equal(st["sigma"], sigma) and st["n"] == 12 and st["variant"] == "fid"
    assert st["features"].dtype == np.float32 and np.array_equal(st["features"], X.astype(np.float32))
    fid.save_stats(p, mu, sigma, 12, "torchvision")
    st = fid.load_stats(p)
    assert st["features"] is None and st["variant"] == "torchvision"
    # pytorch-fid's precomputed files hold mu and sigma only
    bare = str(tmp_path / "bare.npz")
    np.savez(bare, mu=mu, sigma=sigma)
    st = fid.load_stats(bare)
    assert np.array_equal(st["mu"], mu) and np.array_equal(st["sigma"], sigma) and st["n"] is None and st["variant"] is None
    np.savez(bare, mu=mu)
    with pytest.raises(ValueError):
        fid.load_stats(bare)
    # a scorer refuses another graph's statistics before it touches a device
    sc = fid.FidScorer.__new__(fid.FidScorer)
    sc.variant, sc._stats = "torchvision", None
    with pytest.raises(ValueError, match="graph"):
        sc.set_real_stats({"variant": "fid", "features": None, "mu": mu, "sigma": sigma, "n": 12})


# ------------------------------------------------------------------------------------------------- oracle graph, tables
def test_fid_graph_of_the_oracle_differs_where_pytorch_fid_does():
    """the oracle's two pools on a border, and the proxy through which _inception_oracle.forward sees them: eight average
    pools that exclude the padding, the ninth (Mixed_7c's) a max pool, everything else torch.nn.functional's own"""
    x = np.arange(2 * 3 * 4 * 4, dtype=np.float64).reshape(2, 3, 4, 4) - 200.0
    a = FO.avg_pool_valid(x)
    assert a[0, 0, 0, 0] == x[0, :2, :2, 0].mean() and a[0, 1, 1, 0] == x[0, :3, :3, 0].mean()
    assert a[0, 2, 3, 1] == x[0, 1:, 2:, 1].mean()
    m = FO.max_pool_s1(x)
    assert m[0, 0, 0, 0] == x[0, :2, :2, 0].max() and m[0, 0, 0, 0] < 0                      # no padded zero wins
    proxy = FO._FidFunctional()
    t = torch.arange(16.0).reshape(1, 1, 4, 4) - 200
    for _ in range(8):
        assert torch.equal(proxy.avg_pool2d(t, 3, 1, 1), torch.nn.functional.avg_pool2d(t, 3, 1, 1, count_include_pad=False))
    assert torch.equal(proxy.avg_pool2d(t, 3, 1, 1), torch.nn.functional.max_pool2d(t, 3, 1, 1)) and proxy.relu is torch.nn.functional.relu
    assert O.F is torch.nn.functional


def test_variant_tables_and_state_dict_handling():
    from mmhand_amd import inception as I
    lut = I.normalize_lut("fid")
    b = torch.arange(256, dtype=torch.float32)
    assert np.array_equal(lut[2].numpy().view(np.uint32), (2 * (b / 255) - 1).numpy().view(np.uint32))
    assert lut[0, 0] == -1.0 and lut[0, 255] == 1.0
    assert torch.equal(I.normalize_lut(), I.normalize_lut("torchvision"))
    assert torch.equal(I.PreprocessTables(40, 50, 299, device="cpu", variant="fid").lut, lut)
    with pytest.raises(ValueError):
        I.InceptionV3(device="cpu", variant="tf1")
    sd = O.state_dict(0)
    sd["fc.weight"], sd["fc.bias"] = torch.zeros(1008, 2048, dtype=torch.float64), torch.zeros(1008, dtype=torch.float64)
    net = I.InceptionV3(device="cpu", variant="fid").load_state_dict(sd)
    assert net.fc is None and len(net.convs) == 94
    del sd["fc.weight"], sd["fc.bias"]
    I.InceptionV3(device="cpu", variant="fid").load_state_dict(sd)                           # fc is not needed at all
    with pytest.raises(KeyError):
        I.InceptionV3(device="cpu").load_state_dict(sd)


# ------------------------------------------------------------------------------------------------- ABI and arguments
def test_header_signatures_and_exports_agree():
    from mmhand_amd import lib as L
    with open(os.path.join(ROOT, "include", "mmhand_hip.h")) as fh:
        header = fh.read()
    declared = set(re.findall(r"^(?:int|size_t|int64_t|const char\*)\s+(mmh_\w+)\(", header, re.M))
    assert declared == set(L.SIGNATURES), declared ^ set(L.SIGNATURES)
    lib = L.load()                              # binds every declared symbol: a missing export is an AttributeError here
    vs = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "mmhand_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = re.search(r"global:(.*?);", vs, re.S).group(1).split()
    import fnmatch
    for name in NEW:
        assert name in declared and getattr(lib, name) is not None
        assert any(fnmatch.fnmatchcase(name, p.strip(";")) for p in patterns), name
        proto = re.search(r"(?:int|size_t) %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(L.SIGNATURES[name][1]) == len(proto.split(",")), name
    assert re.search(r"MMH_POOL_AVG_VALID = 2, MMH_POOL_MAX_S1 = 3", header) and (L.POOL_AVG_VALID, L.POOL_MAX_S1) == (2, 3)
    assert (L.POOL_MAX, L.POOL_AVG) == (0, 1)
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert f"({len(L.SIGNATURES)} entry points" in fh.read()
    with open(os.path.join(ROOT, "mmhand_amd", "csrc", "Makefile")) as fh:
        assert "fid.hip" in fh.read()


def test_argument_parser():
    from mmhand_amd import evaluate
    p = evaluate.build_parser()
    a = p.parse_args(["--name", "x", "--dataroot", "d", "--dataset", "rhd"])
    assert a.fid is None and a.fid_variant == "torchvision" and a.fid_real is None and a.fid_stats_out is None
    assert (a.kid_subsets, a.kid_subset_size, a.kid_seed) == (100, 1000, 0) and a.fid_images is None
    a = p.parse_args(["--fid_images", "g", "--fid_real", "r.npz", "--fid", "w.pth", "--fid_variant", "fid", "--kid_subsets", "5"])
    assert a.fid_images == "g" and a.fid_variant == "fid" and a.kid_subsets == 5 and a.dataset is None
    with pytest.raises(SystemExit):
        p.parse_args(["--fid_images", "g", "--generated", "h"])                  # one source at a time
    with pytest.raises(SystemExit):
        p.parse_args(["--name", "x", "--fid_variant", "tf"])
    for bad in (["--fid_images", "g", "--fid", "w.pth"],                         # no real set
                ["--fid_images", "g", "--fid_real", "r"],                        # no weights
                ["--name", "x", "--dataroot", "d", "--dataset", "rhd", "--fid_real", "r"],
                ["--is_images", "g", "--inception", "w.pth", "--fid", "w.pth"],
                ["--name", "x", "--dataroot", "d", "--dataset", "rhd", "--fid", "w.pth", "--kid_subset_size", "1"]):
        with pytest.raises(SystemExit):
            evaluate.main(bad)
    assert set(evaluate.FID_FLAGS) == {"fid", "fid_variant", "fid_real", "fid_stats_out", "kid_subsets", "kid_subset_size",
                                       "kid_seed", "fid_images"}
    assert set(evaluate.IS_FLAGS) == {"inception", "is_group", "is_images"}
    help_text = p.format_help()
    for flag in evaluate.FID_FLAGS:
        assert "--" + flag in help_text, flag


def test_evaluate_imports_nothing_of_fid_without_its_flags():
    """a fresh interpreter: importing evaluate, building its parser and walking main() up to the first missing file leaves
    mmhand_amd.fid (and mmhand_amd.inception) unimported"""
    code = ("import sys\n"
            "from mmhand_amd import evaluate\n"
            "evaluate.build_parser().parse_args(['--name', 'x', '--dataroot', 'd', '--dataset', 'rhd'])\n"
            "try:\n"
            "    evaluate.main(['--name', 'no_such_checkpoint', '--dataroot', 'd', '--dataset', 'rhd'])\n"
            "except SystemExit as e:\n"
            "    assert 'no checkpoint' in str(e), e\n"
            "assert 'mmhand_amd.fid' not in sys.modules and 'mmhand_amd.inception' not in sys.modules, sorted(sys.modules)\n"
            "print('clean')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("clean"), out.stderr[-2000:]
