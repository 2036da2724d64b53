"""FID and KID on the device (csrc/fid.hip, the two further pool modes of csrc/inception.hip, mmhand_amd/fid.py and
`evaluate --fid`) against tests/_fid_oracle.py: the moments and the kernel sums bit for bit where float64 is exact and within
bounds derived for any accumulation order elsewhere, the pools exactly on integers, pytorch-fid's graph against the float64
forward of the same graph, and the scorer end to end.  All weights are generated: no figure here says anything about real
images."""
import json
import os
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import _fid_oracle as FO
from tests import _inception_oracle as O
from tests._hpe_oracle import hashed

pytestmark = pytest.mark.gpu
SEED = 0
SENTINEL = -77.0
U = 2.0 ** -53
D_LIST = [4, 20, 64, 132]


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module", autouse=True)
def _give_memory_back():
    yield
    import gc
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------- moments
def _guarded_moments(dev, X):
    """ops.feature_moments into the middle of sentinel-filled buffers -> (mean, cov) as numpy; the guards must be untouched"""
    from mmhand_amd import ops
    N, d = X.shape
    g = 64
    mbuf = torch.full((d + 2 * g,), SENTINEL, dtype=torch.float64, device=dev)
    cbuf = torch.full((d * d + 2 * g,), SENTINEL, dtype=torch.float64, device=dev)
    ops.feature_moments(torch.from_numpy(X).to(dev), mbuf[g:g + d], cbuf[g:g + d * d].view(d, d))
    m, c = mbuf.cpu().numpy(), cbuf.cpu().numpy()
    assert (m[:g] == SENTINEL).all() and (m[g + d:] == SENTINEL).all() and (c[:g] == SENTINEL).all() and (c[g + d * d:] == SENTINEL).all()
    return m[g:g + d], c[g:g + d * d].reshape(d, d)


# N = 2: one k-step with two zero rows; 16, 64: less than / exactly two row blocks of 32; 256: eight; d = 4, 20: one ragged
# tile; 64: exactly one; 132: three tile columns, the last ragged, off-diagonal tiles and their mirrors; d = 2048: the size in use
@pytest.mark.parametrize("N,d", [(n, d) for n in (2, 16, 64, 256) for d in D_LIST] + [(8, 2048)])
def test_moments_are_exact_on_dyadic_integers(dev, N, d):
    X = FO.dyadic_features(N, d, 1000 * N + d)
    want_mean, want_cov = FO.moments_exact(X)
    assert np.array_equal(want_mean, np.round(want_mean)) and np.abs(want_cov).max() > 0
    ld_mean, ld_cov, _ = FO.moments(X)
    assert np.array_equal(ld_mean, want_mean) and np.abs(ld_cov - want_cov).max() <= 2 * U * np.abs(want_cov).max()
    mean, cov = _guarded_moments(dev, X)
    assert np.array_equal(_bits64(mean), _bits64(want_mean))
    assert np.array_equal(_bits64(cov), _bits64(want_cov))


@pytest.mark.parametrize("N", [2, 5, 17, 63, 130])
@pytest.mark.parametrize("d", D_LIST)
def test_moments_of_general_floats_stay_within_the_derived_bound(dev, N, d):
    """|C - C_ref| <= 4 (N + 8) 2^-53 S_ij / (N - 1), S_ij = sum_n |c_ni c_nj|.  Derivation, for any accumulation order: the mean
    is a sum of N exact float64 values, relative error at most (N - 1) u (u = 2^-53), and one division, so |dm| <= N u |m|; the
    first-order effect of dm on sum c_i c_j is dm_j sum_n c_ni + dm_i sum_n c_nj, and sum_n c_ni = 0 up to N u |m|, so it is of
    second order; c = x - mean is rounded once (u |c|), a product of two such values carries 2 u; the products are exact; N
    terms accumulated in any order add (N - 1) u; the final division u.  Total (N + 3) u S to first order; the constant 4 and
    the + 8 leave room for the second-order terms and for |m| > |c| (features abs(randn): |m| / rms(c) is about 1.3)."""
    rng = np.random.RandomState(7 * N + d)
    X = np.abs(rng.randn(N, d)).astype(np.float32)
    _, want, S = FO.moments(X)
    mean, cov = _guarded_moments(dev, X)
    assert np.abs(mean - X.astype(np.float64).mean(0)).max() <= 4 * N * U * np.abs(X).max()
    err, bound = np.abs(cov - want), 4.0 * (N + 8) * U * S / (N - 1)
    print("N=%d d=%d: max err / bound = %.3f" % (N, d, float((err / bound).max())))
    assert (err <= bound).all()
    assert np.array_equal(_bits64(cov), _bits64(cov.T))
    again = _guarded_moments(dev, X)
    assert np.array_equal(_bits64(again[0]), _bits64(mean)) and np.array_equal(_bits64(again[1]), _bits64(cov))


def test_moments_refuse_what_they_cannot_do(dev):
    from mmhand_amd import lib, ops
    with pytest.raises(ValueError):
        ops.feature_moments(torch.zeros((1, 8), device=dev))
    with pytest.raises(ValueError):
        ops.feature_moments(torch.zeros((4, 6), device=dev))
    x, m, c, w = (torch.zeros(64, dtype=torch.float64, device=dev) for _ in range(4))
    assert lib.load().mmh_feature_moments(x.data_ptr(), 1, 8, m.data_ptr(), c.data_ptr(), w.data_ptr(), None) != 0
    assert lib.load().mmh_feature_moments(x.data_ptr(), 4, 6, m.data_ptr(), c.data_ptr(), w.data_ptr(), None) != 0
    assert lib.load().mmh_feature_moments_ws_bytes(1, 8) == 0 and lib.load().mmh_feature_moments_ws_bytes(4, 6) == 0


# ------------------------------------------------------------------------------------------------- kernel sums
def _lists(rng, S, M, n):
    """S permuted lists of M rows out of n; from M >= 2 on every list names one row at two positions"""
    out = np.stack([rng.permutation(n)[:M] if M <= n else rng.randint(0, n, M) for _ in range(S)])
    if M >= 2:
        out[:, M - 1] = out[:, 0]
    return out.astype(np.int32)


# (1, 1): no pair at all in the two symmetric sums; (5, 3): one ragged tile; (17, 16): more rows than one MFMA tile; (37, 21):
# more than a wave's quadrant; (130, 67): 3 x 3 and 2 x 2 tiles - off-diagonal tiles doubled, ragged last tiles
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("Ma,Mb", [(1, 1), (5, 3), (17, 16), (37, 21), (130, 67)])
@pytest.mark.parametrize("d", [8, 64])
def test_kernel_sums_are_exact_on_small_integers(dev, d, Ma, Mb, S):
    """features 0 .. 3 and d a power of two: every term is a multiple of 1 / d^3 below (9 + 1)^3, every sum below 2^53 / d^3"""
    from mmhand_amd import ops
    rng = np.random.RandomState(d * 1000 + Ma * 10 + S)
    A = rng.randint(0, 4, size=(Ma + 7, d)).astype(np.float32)
    B = rng.randint(0, 4, size=(Mb + 5, d)).astype(np.float32)
    ia, ib = _lists(rng, S, Ma, len(A)), _lists(rng, S, Mb, len(B))
    want = FO.mmd_sums(A, B, ia, ib)
    assert np.array_equal(want, FO.mmd_sums(A, B, ia, ib, np.float64))            # exact: longdouble and float64 agree
    if Ma >= 2:     # the repeated row counts as a pair: by value it would not
        assert want[0, 0] > FO.mmd_sums(A, B, ia[:, :-1], ib)[0, 0] + 1.0
    got = ops.poly_mmd_sums(torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev), ia, ib).cpu().numpy()
    assert got.shape == (S, 3) and np.array_equal(_bits64(got), _bits64(want)), (got, want)


@pytest.mark.parametrize("d", [4, 20, 132, 2048])
def test_kernel_sums_of_general_floats_stay_within_the_bound(dev, d):
    """each sum within relative 2^-53 (4 (d + 4) + P) of the oracle, P its number of pairs (all terms are positive): the dot
    product's d products are exact and their accumulation in any order costs (d - 1) u, the division and the + 1 one u each,
    the cube 2 u on top of three times t's error - under 4 (d + 4) u per term - and P positive terms summed in any order add
    at most (P - 1) u.  The same subset gives the same bits from another slot of a larger S and from a differently ordered
    feature buffer (the lists adjusted so that they name the same row values in the same order)."""
    from mmhand_amd import ops
    Ma, Mb = 33, 18
    rng = np.random.RandomState(d)
    A = np.abs(rng.randn(Ma + 6, d)).astype(np.float32)
    B = np.abs(rng.randn(Mb + 9, d)).astype(np.float32)
    ia, ib = _lists(rng, 1, Ma, len(A)), _lists(rng, 1, Mb, len(B))
    want = FO.mmd_sums(A, B, ia, ib)
    Ad, Bd = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    got = ops.poly_mmd_sums(Ad, Bd, ia, ib).cpu().numpy()
    for j, P in enumerate((Ma * (Ma - 1), Mb * (Mb - 1), Ma * Mb)):
        rel = abs(got[0, j] - want[0, j]) / want[0, j]
        print("d=%d sum %d: rel err %.3e, bound %.3e" % (d, j, rel, U * (4 * (d + 4) + P)))
        assert rel <= U * (4 * (d + 4) + P)
    # another S, another slot, the rows at other places of the buffers
    pa, pb = rng.permutation(len(A)), rng.permutation(len(B))
    inv_a, inv_b = np.argsort(pa), np.argsort(pb)
    ia3 = np.concatenate([_lists(rng, 2, Ma, len(A)), inv_a[ia]]).astype(np.int32)
    ib3 = np.concatenate([_lists(rng, 2, Mb, len(B)), inv_b[ib]]).astype(np.int32)
    assert np.array_equal(A[pa][ia3[2]], A[ia[0]])
    got3 = ops.poly_mmd_sums(torch.from_numpy(A[pa]).to(dev), torch.from_numpy(B[pb]).to(dev), ia3, ib3).cpu().numpy()
    assert np.array_equal(_bits64(got3[2]), _bits64(got[0]))
    assert np.array_equal(_bits64(ops.poly_mmd_sums(Ad, Bd, ia, ib).cpu().numpy()), _bits64(got))


def test_kernel_sums_refuse_what_they_cannot_do(dev):
    from mmhand_amd import ops
    A = torch.zeros((4, 8), device=dev)
    with pytest.raises(ValueError):
        ops.poly_mmd_sums(A, A, [[0, 4]], [[0, 1]])               # no row 4
    with pytest.raises(ValueError):
        ops.poly_mmd_sums(A, A, [[0, -1]], [[0, 1]])
    with pytest.raises(ValueError):
        ops.poly_mmd_sums(A, torch.zeros((4, 12), device=dev), [[0]], [[0]])
    with pytest.raises(ValueError):
        ops.poly_mmd_sums(A, A, [[0, 1]], [[0, 1], [1, 2]])       # S differs


# ------------------------------------------------------------------------------------------------- pools
def _pool_input(B, H, W_, C, seed):
    return np.floor(hashed(seed, B * H * W_ * C, SEED).reshape(B, H, W_, C) * 9.0)        # integers -9 .. 8


@pytest.mark.parametrize("H,W_", [(5, 4), (2, 1), (17, 17)])
def test_new_pool_modes_are_exact_and_the_old_ones_unchanged(dev, H, W_):
    from mmhand_amd import ops
    C = 8
    x = _pool_input(2, H, W_, C, 83)
    x[0, 0, 0, :] = -7.0                   # a negative corner: a padded zero must not win the max nor enter the average
    xd = torch.from_numpy(x.astype(np.float32)).to(dev)
    # window sums are integers: float64 sum / count rounded once to fp32 is the correctly rounded fp32 quotient
    wants = {"avg_valid": FO.avg_pool_valid(x).astype(np.float32), "max_s1": FO.max_pool_s1(x).astype(np.float32)}
    if (H, W_) == (2, 1):
        assert wants["avg_valid"][0, 0, 0, 0] == np.float32((-7.0 + x[0, 1, 0, 0]) / 2.0)
    before = {m: ops.pool3x3(xd, m).cpu().numpy() for m in (("avg", "max") if H >= 3 and W_ >= 3 else ("avg",))}
    for mode, want in wants.items():
        got = ops.pool3x3(xd, mode).cpu().numpy()
        assert got.shape == (2, H, W_, C) and np.array_equal(_bits32(got), _bits32(want)), mode
        xw = torch.full((2, H, W_, C + 8), 99.0, device=dev)
        xw[..., 4:4 + C] = xd
        out = torch.full((2, H, W_, C + 12), SENTINEL, device=dev)
        ops.pool3x3(xw, mode, c=C, x_off=4, out=out, y_off=8)
        assert np.array_equal(_bits32(out[..., 8:8 + C].cpu().numpy()), _bits32(want))
        assert bool((out[..., :8] == SENTINEL).all()) and bool((out[..., 8 + C:] == SENTINEL).all())
    assert np.array_equal(_bits32(before["avg"]), _bits32(O.avg_pool(x).astype(np.float32)))
    if "max" in before:
        assert np.array_equal(before["max"].astype(np.float64), O.max_pool(x))
    for m, b in before.items():
        assert np.array_equal(_bits32(ops.pool3x3(xd, m).cpu().numpy()), _bits32(b))


# ------------------------------------------------------------------------------------------------- the "fid" variant
@pytest.fixture(scope="module")
def sd32():
    return OrderedDict((k, v.float() if v.is_floating_point() else v) for k, v in O.state_dict(SEED).items())


@pytest.fixture(scope="module")
def net(dev, sd32):
    from mmhand_amd import inception
    return inception.InceptionV3(dev).load_state_dict(sd32)


def _rel_l1(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).sum() / np.abs(b).sum())


def test_fid_variant_stays_within_twice_pytorch_fp32(dev, sd32, net):
    """pooled features under pytorch-fid's graph against the float64 forward of the same graph on the same inputs and weights:
    relative L1 at most twice what PyTorch's fp32 CPU forward keeps (DESIGN 4.5h's bar).  The checkpoint is pytorch-fid's shape:
    fc [1008,2048], never read.  The torchvision variant's features keep the bits of features() as it stands."""
    from mmhand_amd import inception
    sd_fid = OrderedDict(sd32)
    sd_fid["fc.weight"], sd_fid["fc.bias"] = torch.zeros(1008, 2048), torch.zeros(1008)
    fid_net = inception.InceptionV3(dev, variant="fid").load_state_dict(sd_fid)
    assert fid_net.fc is None
    with pytest.raises(ValueError):
        inception.InceptionV3(dev, variant="tf")
    sd64 = OrderedDict((k, v.double()) for k, v in sd32.items() if v.is_floating_point())
    for shape, index in (((2, 3, 75, 75), 0), ((1, 3, 107, 91), 1)):
        x = O.net_inputs(shape, SEED, index).astype(np.float32)
        xd = torch.zeros((shape[0], shape[2], shape[3], 4), device=dev)
        xd[..., :3] = torch.from_numpy(x).to(dev).permute(0, 2, 3, 1)
        f64 = FO.forward(sd64, x.astype(np.float64), variant="fid").numpy()
        f32 = FO.forward(sd64, x, torch.float32, variant="fid").double().numpy()
        tv64 = FO.forward(sd64, x.astype(np.float64)).numpy()
        got = fid_net.features(xd).cpu().numpy()
        e, ref = _rel_l1(got, f64), _rel_l1(f32, f64)
        print("%s: device %.3e, PyTorch fp32 %.3e, ratio %.2f; the two graphs differ by %.3e" % (shape, e, ref, e / ref, _rel_l1(tv64, f64)))
        assert got.shape == (shape[0], 2048) and e <= 2.0 * ref
        assert _rel_l1(tv64, f64) > 100 * ref                      # the graphs differ by far more than the bar
        with pytest.raises(RuntimeError):
            fid_net(xd)
        tv = net.features(xd)
        assert np.array_equal(_bits32(inception.InceptionV3(dev, variant="torchvision").load_state_dict(sd32).features(xd).cpu().numpy()),
                              _bits32(tv.cpu().numpy()))
        assert np.array_equal(_bits32(net.logits_of(tv).cpu().numpy()), _bits32(net(xd).cpu().numpy()))
    lut = inception.normalize_lut("fid")
    b = torch.arange(256, dtype=torch.float32)
    assert np.array_equal(_bits32(lut[1].numpy()), _bits32((2 * (b / 255) - 1).numpy())) and lut.shape == (3, 256)


# ------------------------------------------------------------------------------------------------- end to end
def _check_against_features(res, G, R, subsets, size, seed):
    """FID within 1e-9 relative of the nuclear-norm oracle on the same features; the KID keys within the kernel-sum bound
    (relative 2^-53 (4 (d + 4) + P) per sum) propagated through kid_from_sums, whose three divisions, two additions and the
    mean over subsets add 4 u of the terms' sizes"""
    from mmhand_amd import fid
    G, R = np.asarray(G, dtype=np.float32), np.asarray(R, dtype=np.float32)
    d = G.shape[1]
    want = FO.frechet_nuclear(G, R)
    print("FID %.12e, oracle %.12e, rel %.3e" % (res["FID"], want["fid"], abs(res["FID"] - want["fid"]) / abs(want["fid"])))
    assert abs(res["FID"] - want["fid"]) <= 1e-9 * abs(want["fid"]), (res["FID"], want["fid"])
    ia, ib = fid.draw_subsets(len(G), len(R), subsets, size, seed)
    M = ia.shape[1]

    def kid_and_bound(sums, Ma, Mb):
        k = fid.kid_from_sums(sums, Ma, Mb)
        rel = [U * (4 * (d + 4) + P) for P in (Ma * (Ma - 1), Mb * (Mb - 1), Ma * Mb)]
        b = sums[:, 0] * rel[0] / (Ma * (Ma - 1.0)) + sums[:, 1] * rel[1] / (Mb * (Mb - 1.0)) + 2 * sums[:, 2] * rel[2] / (Ma * Mb)
        return k, b + 4 * U * (sums[:, 0] / (Ma * (Ma - 1.0)) + sums[:, 1] / (Mb * (Mb - 1.0)) + 2 * sums[:, 2] / (Ma * Mb))

    k, b = kid_and_bound(FO.mmd_sums(G, R, ia, ib), M, M)
    # np.std moves by at most the RMS of the values' errors (<= b.max()); the second b.max() covers its own rounding
    assert abs(res["KID_mean"] - np.mean(k)) <= b.max() and abs(res["KID_std"] - np.std(k)) <= 2 * b.max()
    kf, bf = kid_and_bound(FO.mmd_sums(G, R, [np.arange(len(G))], [np.arange(len(R))]), len(G), len(R))
    assert abs(res["KID_full"] - kf[0]) <= bf[0]
    assert res["n_generated"] == len(G) and res["n_real"] == len(R)
    return b.max()


def test_scorer_against_the_oracle_on_its_own_features(dev, net):
    from mmhand_amd import fid
    real = torch.from_numpy(O.images(6, 64, 64, SEED)).to(dev)
    gen = torch.from_numpy(O.images(5, 64, 64, SEED + 1)).to(dev)
    sc = fid.FidScorer(net, device=dev, size=75, kid_subsets=4, kid_subset_size=4, kid_seed=3)
    sc.feed_real(real[:4]); sc.feed_real(real[4:]); sc.feed_generated(gen)
    with pytest.warns(UserWarning, match="fewer images than features"):
        res = sc.results()
    G, R = torch.cat(sc._gen).cpu().numpy(), torch.cat(sc._real).cpu().numpy()
    assert G.shape == (5, 2048) and G.dtype == np.float32 and res["fid_variant"] == "torchvision"
    _check_against_features(res, G, R, 4, 4, 3)
    assert res["FID"] > 0
    # a set against itself: FID <= 1e-9 tr(S), KID_full negative or zero within its bound
    me = fid.FidScorer(net, device=dev, size=75, kid_subsets=2, kid_subset_size=6)
    me.feed_real(real); me.feed_generated(real)
    with pytest.warns(UserWarning):
        own = me.results()
    tr = float(np.trace(np.cov(R.astype(np.float64), rowvar=False)))
    print("self: FID %.3e of tr(S) %.3e, KID_full %.3e" % (own["FID"], tr, own["KID_full"]))
    assert abs(own["FID"]) <= 1e-9 * tr
    sums = FO.mmd_sums(R, R, [np.arange(6)], [np.arange(6)])
    bound = U * (4 * (2048 + 4) + 36 + 4) * (2 * sums[0, 0] / 30.0 + 2 * sums[0, 2] / 36.0)
    want_full = FO.mmd2_unbiased(R, R)
    assert want_full < 0 and abs(own["KID_full"] - want_full) <= bound and own["KID_full"] <= bound


@pytest.fixture
def work_dir():
    """a scratch directory whose PATH does not contain "test" (the loader keys on it)"""
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="mmh_fid_")
    assert "test" not in d
    yield d
    shutil.rmtree(d, ignore_errors=True)


def test_evaluate_fid_in_three_modes(dev, net, sd32, work_dir, monkeypatch):
    from PIL import Image
    from mmhand_amd import evaluate, fid
    from mmhand_amd.networks import Generator
    from tests._dataset_fixture import write_rhd
    root = os.path.join(work_dir, "rhd")
    write_rhd(root, n=6, size=32)
    monkeypatch.chdir(work_dir)
    torch.save(OrderedDict(("module." + k, v) for k, v in sd32.items()), "inception.pth")
    os.makedirs(os.path.join("checkpoints", "ev"))
    torch.manual_seed(5)
    torch.save(Generator([3, 42, 6], 3, 8, "instance", False, 2).state_dict(), os.path.join("checkpoints", "ev", "latest_net_netG.pth"))

    seen = {}
    results = fid.FidScorer.results

    def spy(self, stats_out=None):
        seen["G"] = torch.cat(self._gen).cpu().numpy()
        seen["R"] = torch.cat(self._real).cpu().numpy() if self._real else None
        return results(self, stats_out)

    monkeypatch.setattr(fid.FidScorer, "results", spy)
    flags = ["--fid", "inception.pth", "--kid_subsets", "3", "--kid_subset_size", "4", "--kid_seed", "2"]
    keys = {"FID", "KID_mean", "KID_std", "KID_full", "n_real", "n_generated", "fid_variant"}

    # 1. a generator checkpoint: the fake batches and their targets
    base = ["--name", "ev", "--dataroot", root, "--dataset", "rhd", "--batchSize", "4"]
    random.seed(11)
    with pytest.warns(UserWarning):
        res = evaluate.main(base + flags + ["--results_json", "g.json", "--per_image_csv", "g.csv", "--fid_stats_out", "real.npz"])
    s_gen = json.load(open("g.json"))["summary"]
    assert keys <= set(s_gen) and s_gen["n_real"] == s_gen["n_generated"] == 6 and s_gen["fid_variant"] == "torchvision"
    _check_against_features(s_gen, seen["G"], seen["R"], 3, 4, 2)
    G_gen, R_gen = seen["G"], seen["R"]
    assert open("g.csv").readline().strip() == "target,source,ssim,l1,psnr"            # no per-image column
    st = fid.load_stats("real.npz")
    assert st["n"] == 6 and st["variant"] == "torchvision" and np.array_equal(st["features"], R_gen)
    # without the flags the files are what they were
    random.seed(11)
    plain = evaluate.main(base + ["--results_json", "n.json"])
    n = json.load(open("n.json"))
    assert set(n["summary"]) == {"SSIM_avg", "SSIM_std", "L1_avg", "PSNR_avg", "n"} and not set(n["options"]) & set(evaluate.FID_FLAGS)
    assert [r["ssim"] for r in plain["rows"]] == [r["ssim"] for r in res["rows"]]
    # --inception --fid on one file: one forward, the IS figures of --inception alone bit for bit
    random.seed(11)
    with pytest.warns(UserWarning):
        evaluate.main(base + flags + ["--inception", "inception.pth", "--is_group", "4", "--results_json", "b.json"])
    both = json.load(open("b.json"))["summary"]
    random.seed(11)
    evaluate.main(base + ["--inception", "inception.pth", "--is_group", "4", "--results_json", "i.json"])
    alone = json.load(open("i.json"))["summary"]
    for k in ("IS_avg", "IS_std", "IS_all"):
        assert both[k] == alone[k], k
    assert both["FID"] == s_gen["FID"] and both["KID_full"] == s_gen["KID_full"]

    # 2. a directory of PNGs under the targets' names: --generated, the real side again the split's targets
    os.makedirs(os.path.join("gen", "color"), exist_ok=True)
    rng = np.random.RandomState(4)
    for r in res["rows"]:
        Image.fromarray(rng.randint(0, 256, size=(32, 32, 3), dtype=np.uint8)).save(os.path.join("gen", "color", os.path.basename(r["target"])))
    random.seed(11)
    with pytest.warns(UserWarning):
        evaluate.main(["--generated", "gen", "--dataroot", root, "--dataset", "rhd", "--batchSize", "3", "--results_json", "d.json"] + flags)
    s_dir = json.load(open("d.json"))["summary"]
    _check_against_features(s_dir, seen["G"], seen["R"], 3, 4, 2)
    assert np.array_equal(np.sort(seen["R"], 0), np.sort(R_gen, 0))                    # the same targets, as bytes both times
    G_dir = seen["G"]

    # 3. two directories, no labels: the PNGs above against the dataset's colour images, then against the statistics file
    with pytest.warns(UserWarning):
        evaluate.main(["--fid_images", "gen", "--fid_real", os.path.join(root, "color"), "--batchSize", "4", "--results_json", "t.json"] + flags)
    s_two = json.load(open("t.json"))["summary"]
    assert set(s_two) == keys | {"n"} and s_two["n"] == 6
    _check_against_features(s_two, seen["G"], seen["R"], 3, 4, 2)
    assert np.array_equal(np.sort(seen["G"], 0), np.sort(G_dir, 0))
    with pytest.warns(UserWarning):
        evaluate.main(["--fid_images", "gen", "--fid_real", "real.npz", "--batchSize", "4", "--results_json", "u.json"] + flags)
    s_npz = json.load(open("u.json"))["summary"]
    assert s_npz["n_real"] == 6 and s_npz["KID_full"] is not None
    # a file with pytorch-fid's two keys only: FID, and KID reported as null
    np.savez("bare.npz", mu=st["mu"], sigma=st["sigma"])
    evaluate.main(["--fid_images", "gen", "--fid_real", "bare.npz", "--batchSize", "4", "--results_json", "v.json"] + flags)
    s_bare = json.load(open("v.json"))["summary"]
    assert s_bare["KID_mean"] is None and s_bare["KID_std"] is None and s_bare["KID_full"] is None and s_bare["n_real"] is None
    assert s_bare["FID"] == s_npz["FID"]
