"""The 3D estimator training's host side (mmhand_amd/hpe_train.py: Hpm3dTrainer, train_hpe.py --net hpm3d, csrc/hpe3d_train.hip's
argument checks): the ABI's lists agree, bad arguments are refused before any launch, the oracle (tests/_hpe3d_train_oracle.py)
against the numbers recorded from the reference's own network (tests/golden/hpe3d_train.npz) and against torch's own smooth-L1
and Linear backward, the checkpoint layout's round trip, the command line's refusals, and the premise of the GPU cases' poses.
No GPU."""
import ctypes as C
import json
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _hpe_oracle as O
from tests import _hpe_train_oracle as T
from tests import _hpe3d_train_oracle as T3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0
NEW = ("mmh_gauss_heatmaps", "mmh_smooth_l1", "mmh_linear_dgrad", "mmh_linear_wgrad")
# (H, W) of every mmh_gauss_heatmaps case of tests/test_hpe3d_train_gpu.py, and the batch sizes
GRIDS, BATCHES = ((32, 32), (40, 24), (24, 40), (256, 256)), (1, 3)


def test_header_signatures_and_exports_agree():
    from mmhand_amd import lib as L
    with open(os.path.join(ROOT, "include", "mmhand_hip.h")) as fh:
        header = fh.read()
    declared = set(re.findall(r"^(?:int|size_t|int64_t|const char\*)\s+(mmh_\w+)\(", header, re.M))
    assert declared == set(L.SIGNATURES), declared ^ set(L.SIGNATURES)
    lib = L.load()                              # binds every declared symbol: a missing export is an AttributeError here
    for name in NEW:
        assert name in declared and getattr(lib, name) is not None
        proto = re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(L.SIGNATURES[name][1]) == len(proto.split(",")), name
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert f"({len(L.SIGNATURES)} entry points" in fh.read()
    with open(os.path.join(ROOT, "mmhand_amd", "csrc", "Makefile")) as fh:
        assert "hpe3d_train.hip" in fh.read()


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    from mmhand_amd import lib as L
    lib = L.load()
    # host memory stands in for every buffer: nothing is launched, so nothing is dereferenced on a device
    buf = (C.c_double * 4096)()
    p = C.addressof(buf)
    nan = float("nan")

    def err(rc):
        return rc, (lib.mmh_last_error() or b"").decode()

    def gauss(uv=p, B=2, H=32, W=32, sigma=5.0, out=p, cs=24):
        return err(lib.mmh_gauss_heatmaps(uv, B, H, W, sigma, out, cs, None))

    def sl1(pred=p, ps=24, target=p, M=2, n=21, beta=1.0, scale=10.0, loss=p, dpred=p, dcs=24):
        return err(lib.mmh_smooth_l1(pred, ps, target, M, n, beta, scale, loss, dpred, dcs, None))

    def dgrad(dy=p, wt=p, dx=p, M=2, K=8, N=8):
        return err(lib.mmh_linear_dgrad(dy, wt, dx, M, K, N, None))

    def wgrad(x=p, dy=p, dwt=p, db=p, M=2, K=8, N=8):
        return err(lib.mmh_linear_wgrad(x, dy, dwt, db, M, K, N, None))

    cases = [(gauss, dict(uv=None), "NULL"), (gauss, dict(out=None), "NULL"), (gauss, dict(B=0), "bad shape"),
             (gauss, dict(H=0), "bad shape"), (gauss, dict(cs=20), "bad shape"), (gauss, dict(cs=26), "bad shape"),
             (gauss, dict(sigma=0.0), "sigma"), (gauss, dict(sigma=nan), "sigma"), (gauss, dict(sigma=float("inf")), "sigma"),
             (gauss, dict(out=p + 4), "aligned"), (gauss, dict(uv=p + 4), "aligned"),
             (sl1, dict(pred=None), "NULL"), (sl1, dict(target=None), "NULL"), (sl1, dict(loss=None), "NULL"),
             (sl1, dict(M=0), "bad shape"), (sl1, dict(M=65), "bad shape"), (sl1, dict(n=25, ps=28), "bad shape"),
             (sl1, dict(n=0), "bad shape"), (sl1, dict(ps=20), "bad shape"), (sl1, dict(dcs=20), "bad shape"),
             (sl1, dict(beta=0.0), "beta"), (sl1, dict(beta=nan), "beta"), (sl1, dict(scale=nan), "scale"),
             (sl1, dict(dpred=p + 4), "aligned"), (sl1, dict(target=p + 4), "aligned"),
             (dgrad, dict(dy=None), "NULL"), (dgrad, dict(wt=None), "NULL"), (dgrad, dict(dx=None), "NULL"),
             (dgrad, dict(M=0), "bad shape"), (dgrad, dict(M=65), "bad shape"), (dgrad, dict(N=6), "bad shape"),
             (dgrad, dict(K=0), "bad shape"), (dgrad, dict(N=0), "bad shape"), (dgrad, dict(wt=p + 4), "aligned"),
             (dgrad, dict(dx=p + 8), "aligned"),
             (wgrad, dict(x=None), "NULL"), (wgrad, dict(dy=None), "NULL"), (wgrad, dict(dwt=None), "NULL"),
             (wgrad, dict(M=0), "bad shape"), (wgrad, dict(M=65), "bad shape"), (wgrad, dict(N=6), "bad shape"),
             (wgrad, dict(K=0), "bad shape"), (wgrad, dict(dwt=p + 4), "aligned"), (wgrad, dict(db=p + 4), "aligned"),
             (wgrad, dict(dy=p + 8), "aligned")]
    for fn, kw, word in cases:
        rc, msg = fn(**kw)
        assert rc != 0 and word in msg, (fn.__name__, kw, rc, msg)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "hpe3d_train.npz"))


def test_oracle_matches_the_reference_network(gold):
    """the 42 outputs, the loss and every parameter's gradient of the reference's own Hpm3d (NARROW widths, B = 2, 32 x 32,
    float64); stage6.* and nothing else has no gradient"""
    sd = O.state_dict("3d", O.NARROW, head_hw=4, seed=SEED)
    heat, z = T3.inputs(SEED)
    l, out, grads, none = T3.param_grads(sd, T3.nchw(heat).double(), torch.from_numpy(z))
    assert np.abs(out / gold["out"] - 1.0).max() < 1e-12 and abs(l / float(gold["loss"]) - 1.0) < 1e-12
    assert set(none) == set(gold["no_grad"].tolist()) == {k for k in sd if k.startswith("stage6.")}
    assert set("grad_" + k for k in grads) | {"out", "loss", "no_grad"} == set(gold.files)
    assert len(grads) == 110 and sum(v.numel() for v in grads.values()) == 150163
    worst = max(O.rel_l1(grads[k].numpy(), gold["grad_" + k]) for k in grads)
    print("largest relative L1 of a parameter gradient against the fixture: %.2e" % worst)
    assert worst < 1e-12
    assert all(np.abs(gold["grad_" + k]).sum() > 0 for k in grads)
    d = np.abs(out - z)
    assert int((d >= 1.0).sum()) == 2 and np.abs(out).max() < 0.14          # both branches of the loss carry terms
    # three torch.optim.Adam steps leave what has no gradient unchanged
    _, after = T3.adam_trace(sd, T3.nchw(heat), torch.from_numpy(z), steps=3)
    assert all(torch.equal(after[k], sd[k]) for k in none) and not torch.equal(after["depth_fc_3.weight"], sd["depth_fc_3.weight"])


@pytest.mark.parametrize("beta", [1.0, 0.5])
def test_smooth_l1_definition_is_torchs(beta):
    """the numpy definition against F.smooth_l1_loss and its autograd gradient in float64, with d = 0, |d| = beta exactly (the
    linear branch, gradient sign(d)), just inside and outside, and large differences"""
    M, n = 5, 21
    target = (O.hashed(31, M * n, SEED) * 0.75).reshape(M, n)
    pred = np.zeros((M, 24), dtype=np.float32)
    pred[:, :n] = (O.hashed(32, M * n, SEED) * 0.5).reshape(M, n)
    pred[:, 21:] = np.nan                                                   # lanes beyond n are not read
    target[0, 0] = np.float64(pred[0, 0])                                   # d = 0
    target[0, 1], target[0, 2] = np.float64(pred[0, 1]) - beta, np.float64(pred[0, 2]) + beta      # |d| = beta, either sign
    target[0, 3], target[0, 4] = np.float64(pred[0, 3]) - beta * (1 - 2.0 ** -40), np.float64(pred[0, 4]) + beta * (1 + 2.0 ** -40)
    target[1, 0], target[1, 1] = 7.5, -300.0
    # pred - target must give the planted differences back exactly
    assert abs(np.float64(pred[0, 1]) - target[0, 1]) == beta and abs(np.float64(pred[0, 2]) - target[0, 2]) == beta
    for scale in (1.0, 10.0):
        loss, g = T3.smooth_l1(pred, target, n, beta, scale)
        p = torch.from_numpy(pred[:, :n]).double().requires_grad_(True)
        ref = F.smooth_l1_loss(p, torch.from_numpy(target), beta=beta) * scale
        ref.backward()
        assert abs(loss / float(ref.detach()) - 1.0) < 1e-14
        assert np.abs(g[:, :n] - p.grad.numpy()).max() <= 1e-15 * np.abs(g).max() and not g[:, n:].any()
        coef = scale / (M * n)
        assert g[0, 0] == 0.0 and g[0, 1] == coef and g[0, 2] == -coef and abs(g[0, 3]) < coef and g[0, 4] == -coef
        assert g[1, 0] == -coef and g[1, 1] == coef


def test_linear_definitions_are_torchs_backward():
    M, K, N = 3, 20, 8
    x = torch.from_numpy(O.hashed(41, M * K, SEED).reshape(M, K)).requires_grad_(True)
    w = torch.from_numpy(O.hashed(42, N * K, SEED).reshape(N, K)).requires_grad_(True)      # nn.Linear's [N,K]
    b = torch.from_numpy(O.hashed(43, N, SEED)).requires_grad_(True)
    dy = torch.from_numpy(O.hashed(44, M * N, SEED).reshape(M, N))
    F.linear(x, w, b).backward(dy)
    wt = w.detach().t().contiguous().numpy()                                                # the kernels' [K,N]
    dx, tx = T3.linear_dgrad(dy.numpy(), wt)
    dwt, db, tw, tb = T3.linear_wgrad(x.detach().numpy(), dy.numpy())
    assert np.abs(dx - x.grad.numpy()).max() < 1e-14 and np.abs(dwt - w.grad.t().numpy()).max() < 1e-14
    assert np.abs(db - b.grad.numpy()).max() < 1e-14
    assert (tx >= np.abs(dx)).all() and (tw >= np.abs(dwt)).all() and (tb >= np.abs(db)).all()
    assert T3.gamma(512) == pytest.approx(512 * 2.0 ** -24, rel=1e-4)


@pytest.mark.parametrize("widths", ["narrow", "full"])
def test_state_dict_round_trips_through_the_padded_layout(widths):
    from mmhand_amd import hpe, hpe_train
    sd = O.state_dict("3d", O.NARROW if widths == "narrow" else O.FULL, head_hw=4, seed=SEED, dtype=torch.float32)
    plain = hpe_train.Hpm3dTrainer("cpu").load_state_dict(sd)
    tr = hpe_train.Hpm3dTrainer("cpu").load_state_dict(OrderedDict(("module." + k, v) for k, v in sd.items()))
    assert torch.equal(plain.p, tr.p) and tr.head_hw == 4
    out = tr.state_dict()
    assert list(out) == list(sd)
    for k in sd:
        assert out[k].dtype == torch.float32 and out[k].shape == sd[k].shape and torch.equal(out[k], sd[k]), k
    with open(os.path.join(ROOT, "tests", "golden", "hpe_keys.json")) as fh:
        keys = json.load(fh).get("hpm3d") or O.keys_and_shapes(O.state_dict("3d", O.FULL, head_hw=32))
    assert [k for k, _ in O.keys_and_shapes(out)] == [k for k, _ in keys]
    if widths == "full":        # the full-width shapes but for depth_fc_1, sized here for 4 x 4 maps
        assert [s for (k, s) in O.keys_and_shapes(out) if k != "depth_fc_1.weight"] == [s for (k, s) in keys if k != "depth_fc_1.weight"]
    # state_dict -> relay -> state_dict: bit-equal, and the same device layout as the inference network's, fc included
    again = hpe_train.Hpm3dTrainer("cpu").load_state_dict(out)
    assert torch.equal(again.p, tr.p)
    net = hpe.Hpm3d("cpu").load_state_dict(out)
    for name, (w, b) in net.convs.items():
        tw, tb = tr._views(tr.p, name)
        assert torch.equal(tw, w) and torch.equal(tb, b), name
    for name, (wt, b) in zip(hpe_train.FC, net.fc):
        tw, tb = tr._views(tr.p, name)
        assert torch.equal(tw, wt) and torch.equal(tb, b), name
    assert sorted(tr.meta) == sorted(list(net.convs) + list(hpe_train.FC)) and not any(k.startswith("stage6") for k in tr.meta)
    # the padding mask marks exactly what no reference tensor owns, and all of it is zero
    mask = tr.padding_mask()
    owned = sum(v.numel() for k, v in sd.items() if not k.startswith("stage6."))
    assert int((~mask).sum()) == owned and not tr.p[mask].any()
    w1 = tr._views(mask, "depth_fc_1")[0].view(4, 4, 24, -1)
    assert w1[:, :, 21:].all() and not w1[:, :, :21, :sd["depth_fc_1.weight"].shape[0]].any()
    w3, b3 = tr._views(mask, "depth_fc_3")
    assert w3[:, 21:].all() and not w3[:, :21].any() and b3.tolist() == [False] * 21 + [True] * 3
    c1 = tr._views(mask, "conv1_1")[0]
    assert c1[:, :, 21:24].all() and not c1[:, :, :21, :sd["conv1_1.weight"].shape[0]].any()
    g = tr.grads()
    assert list(g) == [k for k in sd if not k.startswith("stage6.")] and all(g[k].shape == sd[k].shape and not g[k].any() for k in g)


def test_init_state_dict_3d_is_torchs_default_init():
    from mmhand_amd import hpe_train
    before = torch.random.get_rng_state()
    a, b = hpe_train.init_state_dict_3d(7, O.NARROW, 4), hpe_train.init_state_dict_3d(7, O.NARROW, 4)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert O.keys_and_shapes(a) == O.keys_and_shapes(O.state_dict("3d", O.NARROW, head_hw=4))
    assert O.keys_and_shapes(hpe_train.init_state_dict_3d(0, O.NARROW, 8))[-6][1] == [16, 21 * 64]
    torch.manual_seed(7)
    first = torch.nn.Conv2d(21, O.NARROW["c1"], 3, padding=1)
    torch.random.set_rng_state(before)
    assert torch.equal(a["conv1_1.weight"], first.weight.detach()) and a["depth_fc_2.weight"].abs().max() <= 0.25     # 1 / sqrt(16)
    assert [[n + ".weight", list(s)] for n, s in hpe_train.layer_shapes_3d()] == O.keys_and_shapes(O.state_dict("3d", O.FULL, head_hw=32))[0::2]
    hpe_train.Hpm3dTrainer("cpu").load_state_dict(a)


def test_cli_parses_hpm3d_and_refuses_contradictory_flags(capsys):
    from mmhand_amd import train_hpe
    base = ["--dataroot", "D", "--dataset", "rhd", "--name", "x"]
    parser = train_hpe.build_parser()
    a = parser.parse_args(base)                                             # the hpm2d parse defaults are unchanged
    assert (a.net, a.batchSize, a.lr, a.beta1, a.sigma, a.stage_weights) == ("hpm2d", 32, 1e-4, 0.9, 5.0, [1.0] * 6)
    train_hpe.check_args(parser, a)
    a = parser.parse_args(base + ["--net", "hpm3d"])
    assert (a.net, a.smooth_l1_beta, a.loss_scale, a.heat_source, a.hpm2d, a.lr, a.beta1) == ("hpm3d", 1.0, 10.0, "target", None, 1e-4, 0.9)
    train_hpe.check_args(parser, a)
    train_hpe.check_args(parser, parser.parse_args(base + ["--net", "hpm3d", "--heat_source", "predicted", "--hpm2d", "a.pth",
                                                           "--batchSize", "64", "--lr", "2e-4", "--beta1", "0.5"]))
    for bad in (["--net", "hpm3d", "--heat_source", "predicted"], ["--net", "hpm3d", "--batchSize", "65"],
                ["--net", "hpm3d", "--stage_weights", "1", "1", "1", "1", "1", "2"], ["--net", "hpm3d", "--smooth_l1_beta", "0"],
                ["--net", "hpm3d", "--loss_scale", "nan"], ["--net", "hpm3d", "--heat_source", "upsampled"], ["--net", "hpm1d"],
                ["--hpm2d", "a.pth"], ["--heat_source", "predicted"], ["--smooth_l1_beta", "0.5"]):
        with pytest.raises(SystemExit):
            train_hpe.main(base + bad)
    capsys.readouterr()


def test_no_test_pose_puts_a_map_pixel_on_a_cut():
    """premise of tests/test_hpe3d_train_gpu.py's mmh_gauss_heatmaps cases: no pixel of any map is within 1e-9 relative of 0.0099
    or of 1 (pixels a joint sits on exactly apart: exp(-0.0) is 1.0 in every libm), so an exp that differs from numpy's in the
    last place cannot move a pixel across a cut.  The grids are those tests/test_hpe_train_cpu.py covers for mmh_heatmap_mse."""
    for sigma in (5.0, 1.5):
        for H, W_ in GRIDS:
            for B in BATCHES:
                margin, on = T.cut_margin(T.poses(B, H, W_, SEED), H, W_, sigma)
                assert margin > 1e-9 and on >= 3 * B, (sigma, H, W_, B, margin)
    m = T3.gauss_heatmaps(T.poses(1, 32, 32, SEED), 32, 32, 5.0)
    assert m.shape == (1, 32, 32, 24) and not m[..., 21:].any() and m[..., :21].max() == 1.0
