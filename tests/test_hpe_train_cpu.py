"""The estimator training's host side (mmhand_amd/hpe_train.py, train_hpe.py, csrc/hpe_train.hip's argument checks): the ABI's
three lists agree, bad arguments are refused before any launch, the checkpoint layout round-trips, the learning-rate rule,
the command line's refusals, the oracle (tests/_hpe_train_oracle.py) against the numbers recorded from the reference's own
network (tests/golden/hpe_train.npz), and the premise of the GPU cases' poses.  No GPU."""
import ctypes as C
import json
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import _hpe_oracle as O
from tests import _hpe_train_oracle as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0
NEW = ("mmh_heatmap_mse_ws_bytes", "mmh_heatmap_mse", "mmh_lane_add", "mmh_conv3x3_c4_fprop_f64")
# (h, w) of every mmh_heatmap_mse case of tests/test_hpe_train_gpu.py, and the batch sizes
SHAPES, BATCHES = ((4, 4), (5, 3), (3, 5), (32, 32)), (1, 3)


def test_header_signatures_and_exports_agree():
    from mmhand_amd import lib as L
    with open(os.path.join(ROOT, "include", "mmhand_hip.h")) as fh:
        header = fh.read()
    declared = set(re.findall(r"^(?:int|size_t|int64_t|const char\*)\s+(mmh_\w+)\(", header, re.M))
    assert declared == set(L.SIGNATURES), declared ^ set(L.SIGNATURES)
    for name in NEW:
        assert name in declared
    with open(os.path.join(ROOT, "mmhand_amd", "csrc", "exports.map")) as fh:
        assert "global: mmh_*; local: *;" in fh.read()
    lib = L.load()                              # binds every declared symbol: a missing export is an AttributeError here
    for name in NEW:
        assert getattr(lib, name) is not None
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert f"({len(L.SIGNATURES)} entry points" in fh.read()
    sig = L.SIGNATURES["mmh_heatmap_mse"][1]
    proto = re.search(r"int mmh_heatmap_mse\((.*?)\);", header, re.S).group(1)
    assert len(sig) == len(proto.split(",")) == 15


def test_heatmap_mse_refuses_bad_arguments_before_any_launch():
    from mmhand_amd import lib as L
    lib = L.load()
    ws_bytes = lib.mmh_heatmap_mse_ws_bytes
    assert ws_bytes(6, 2, 4, 4) == 6 * 2 * 2 * 8 and ws_bytes(1, 1, 5, 3) == 2 * 8 and ws_bytes(8, 3, 32, 32) == 8 * 3 * 128 * 8
    assert ws_bytes(0, 2, 4, 4) == 0 and ws_bytes(9, 2, 4, 4) == 0 and ws_bytes(6, 0, 4, 4) == 0 and ws_bytes(6, 2, 0, 4) == 0
    assert ws_bytes(1, 1, 8192, 8192) == 0                      # 2^32 output pixels
    # host memory stands in for every buffer: nothing is launched, so nothing is dereferenced on a device
    buf = (C.c_double * 4096)()
    ptrs = (C.c_void_p * 9)(*[C.addressof(buf)] * 9)
    wts = (C.c_double * 9)(*[1.0] * 9)
    p, need = C.addressof(buf), ws_bytes(6, 2, 4, 4)

    def call(S=6, B=2, h=4, w=4, cs=24, dcs=24, heat=ptrs, dheat=ptrs, ws=p, nbytes=need, sigma=5.0, weight=wts, uv=p, loss=p):
        rc = lib.mmh_heatmap_mse(heat, S, B, h, w, cs, uv, sigma, weight, loss, dheat, dcs, ws, nbytes, None)
        return rc, (lib.mmh_last_error() or b"").decode()

    for kw, word in ((dict(S=0), "bad shape"), (dict(S=9), "bad shape"), (dict(cs=20), "cs"), (dict(dcs=20), "dcs"),
                     (dict(ws=None), "NULL"), (dict(nbytes=need - 8), "workspace"), (dict(heat=None), "NULL"),
                     (dict(uv=None), "NULL"), (dict(loss=None), "NULL"), (dict(weight=None), "NULL"), (dict(sigma=0.0), "sigma"),
                     (dict(sigma=float("nan")), "sigma"), (dict(B=0), "bad shape"), (dict(ws=p + 4), "aligned"),
                     (dict(weight=(C.c_double * 9)(*[float("inf")] * 9)), "finite")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)
    holes = (C.c_void_p * 9)(*[C.addressof(buf)] * 9)
    holes[3] = None
    rc, msg = call(heat=holes)
    assert rc != 0 and "stage 3" in msg
    rc, msg = call(dheat=holes)
    assert rc != 0 and "stage 3" in msg
    assert lib.mmh_lane_add(None, 24, None, 24, 4, 24, None) != 0 and b"NULL" in lib.mmh_last_error()
    for lanes, x_cs, y_cs, pixels in ((6, 24, 24, 4), (24, 20, 24, 4), (24, 24, 26, 4), (24, 24, 24, 0)):
        assert lib.mmh_lane_add(p, x_cs, p, y_cs, pixels, lanes, None) != 0 and b"bad shape" in lib.mmh_last_error()
    assert lib.mmh_lane_add(p + 4, 24, p, 24, 4, 24, None) != 0 and b"aligned" in lib.mmh_last_error()
    c1 = lib.mmh_conv3x3_c4_fprop_f64
    assert c1(None, p, p, p, 1, 8, 8, 64, 64, 1, None) != 0 and b"NULL" in lib.mmh_last_error()
    for B, H, Cout, y_cs in ((0, 8, 64, 64), (1, 0, 64, 64), (1, 8, 6, 8), (1, 8, 260, 260), (1, 8, 64, 60), (1, 8, 64, 66)):
        assert c1(p, p, p, p, B, H, 8, Cout, y_cs, 1, None) != 0 and b"bad shape" in lib.mmh_last_error()
    assert c1(p, p, p, p, 1, 8, 8, 64, 64, 2, None) != 0 and b"act" in lib.mmh_last_error()
    assert c1(p, p + 4, p, p, 1, 8, 8, 64, 64, 1, None) != 0 and b"aligned" in lib.mmh_last_error()


def test_first_layer_oracle_is_a_convolution():
    """tests/_hpe_train_oracle.conv3x3_c4_f64 against F.conv2d in float64, and exact on integers"""
    x = O.hashed(21, 2 * 5 * 7 * 4, SEED).reshape(2, 5, 7, 4).astype(np.float32)
    w = O.hashed(22, 36 * 8, SEED).reshape(3, 3, 4, 8).astype(np.float32)
    b = O.hashed(23, 8, SEED).astype(np.float32)
    want = torch.nn.functional.conv2d(torch.from_numpy(x).double().permute(0, 3, 1, 2), torch.from_numpy(w).double().permute(3, 2, 0, 1),
                                      torch.from_numpy(b).double(), padding=1).permute(0, 2, 3, 1).numpy()
    got = T.conv3x3_c4_f64(x, w, b, relu=False)
    assert got.dtype == np.float32 and np.abs(got - want).max() <= 2.0 ** -24 * np.abs(want).max()
    assert np.array_equal(T.conv3x3_c4_f64(x, w, b), np.maximum(got, 0))
    xi, wi = np.round(x * 3), np.round(w * 3)
    assert np.array_equal(T.conv3x3_c4_f64(xi, wi, np.round(b * 3), relu=False).astype(np.float64),
                          np.round(torch.nn.functional.conv2d(torch.from_numpy(xi).double().permute(0, 3, 1, 2), torch.from_numpy(wi).double().permute(3, 2, 0, 1),
                                                              torch.from_numpy(np.round(b * 3)).double(), padding=1).permute(0, 2, 3, 1).numpy()))


@pytest.mark.parametrize("widths", ["narrow", "full"])
def test_state_dict_round_trips_through_the_padded_layout(widths):
    from mmhand_amd import hpe, hpe_train
    sd = O.state_dict("2d", O.NARROW if widths == "narrow" else O.FULL, seed=SEED, dtype=torch.float32)
    tr = hpe_train.Hpm2dTrainer("cpu").load_state_dict(OrderedDict(("module." + k, v) for k, v in sd.items()))
    out = tr.state_dict()
    assert list(out) == list(sd)
    for k in sd:
        assert out[k].dtype == torch.float32 and out[k].shape == sd[k].shape and torch.equal(out[k], sd[k]), k
    with open(os.path.join(ROOT, "tests", "golden", "hpe_keys.json")) as fh:
        keys = json.load(fh)["hpm2d"]
    if widths == "full":
        assert O.keys_and_shapes(out) == keys
    assert [k for k, _ in O.keys_and_shapes(out)] == [k for k, _ in keys]
    # state_dict -> relay -> state_dict: bit-equal, and the same device layout as the inference network's
    again = hpe_train.Hpm2dTrainer("cpu").load_state_dict(out)
    assert torch.equal(again.p, tr.p)
    net = hpe.Hpm2d("cpu").load_state_dict(out)
    for name, (w, b) in net.convs.items():
        tw, tb = tr._views(tr.p, name)
        assert torch.equal(tw, w) and torch.equal(tb, b), name
    # the padding mask marks exactly what no reference tensor owns, and all of it is zero
    mask = tr.padding_mask()
    assert int((~mask).sum()) == sum(v.numel() for v in sd.values()) and not tr.p[mask].any()
    if widths == "narrow":
        assert int(mask.sum()) > 0
        w1 = tr._views(mask, "stage3.conv1")[0]
        assert w1[:, :, 21:24].all() and not w1[:, :, :21].any() and not w1[:, :, 24:].any()
        assert tr._views(mask, "conv6_2_CPM")[1].tolist() == [False] * 21 + [True] * 3
    g = tr.grads()
    assert list(g) == list(sd) and all(g[k].shape == sd[k].shape and not g[k].any() for k in sd)


def test_init_state_dict_is_torchs_default_conv_init():
    from mmhand_amd import hpe_train
    widths = {k: v for k, v in O.NARROW.items() if k != "fc"}
    before = torch.random.get_rng_state()
    a, b = hpe_train.init_state_dict(7, widths), hpe_train.init_state_dict(7, widths)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["conv1_1.weight"], hpe_train.init_state_dict(8, widths)["conv1_1.weight"])
    assert O.keys_and_shapes(a) == O.keys_and_shapes(O.state_dict("2d", O.NARROW))
    torch.manual_seed(7)
    first = torch.nn.Conv2d(3, widths["c1"], 3, padding=1)
    torch.random.set_rng_state(before)
    assert torch.equal(a["conv1_1.weight"], first.weight.detach()) and torch.equal(a["conv1_1.bias"], first.bias.detach())
    full = hpe_train.layer_shapes()
    with open(os.path.join(ROOT, "tests", "golden", "hpe_keys.json")) as fh:
        keys = json.load(fh)["hpm2d"]
    assert [[n + ".weight", list(s)] for n, s in full] == keys[0::2]


def test_linear_lr_rule_is_the_references():
    from mmhand_amd.hpe_train import linear_lr
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-4)
    niter, decay = 3, 4
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 1.0 - max(0, e + 1 - niter) / float(decay + 1))
    for epoch in range(niter + decay):
        assert linear_lr(1e-4, epoch, niter, decay) == pytest.approx(opt.param_groups[0]["lr"], rel=1e-15)
        opt.step()
        sched.step()
    assert linear_lr(1e-4, 0, 3, 4) == 1e-4 == linear_lr(1e-4, 2, 3, 4) and linear_lr(1e-4, 3, 3, 4) == pytest.approx(0.8e-4)
    assert linear_lr(1e-4, 6, 3, 4) == pytest.approx(0.2e-4) and linear_lr(1e-4, 6, 3, 4) > 0


def test_cli_refuses_contradictory_flags(capsys):
    from mmhand_amd import train_hpe
    base = ["--dataroot", "D", "--dataset", "rhd", "--name", "x"]
    a = train_hpe.build_parser().parse_args(base)
    assert (a.batchSize, a.lr, a.beta1, a.sigma, a.stage_weights) == (32, 1e-4, 0.9, 5.0, [1.0] * 6)
    assert a.extra_dataroot == [] and a.init_from is None and a.init_seed is None
    a = train_hpe.build_parser().parse_args(base + ["--extra_dataroot", "E", "--extra_dataroot", "F"])
    assert a.extra_dataroot == ["E", "F"]
    for bad in (["--init_from", "a.pth", "--init_seed", "1"], ["--niter", "0"], ["--extra_dataroot", "D"], ["--val_dataroot", "D"],
                ["--extra_dataroot", "E", "--val_dataroot", "E"], ["--stage_weights", "0", "0", "0", "0", "0", "0"],
                ["--stage_weights", "1", "1"], ["--save_epoch_freq", "0"], ["--sigma", "0"], ["--dataset", "coco"]):
        with pytest.raises(SystemExit):
            train_hpe.main(base[:2] + (base[2:4] if "--dataset" not in bad else []) + base[4:] + bad)
    capsys.readouterr()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "hpe_train.npz"))


def test_oracle_matches_the_reference_network(gold):
    """the six losses and every parameter's gradient of the reference's own Hpm2d (NARROW widths, B = 2, 32 x 32, float64)"""
    sd = O.state_dict("2d", O.NARROW, seed=SEED)
    x = torch.from_numpy(O.normalize(O.images(2, 32, 32, SEED))[..., :3]).permute(0, 3, 1, 2).double()
    uv = T.poses(2, 32, 32, SEED)
    # the stored target is the oracle's, bit for bit (pinned to RHD_dataset.py:245-277 by formula: that module needs OpenCV)
    assert np.array_equal(gold["target"].transpose(0, 2, 3, 1), T.target(uv, 32, 32, 5.0))
    ls, grads = T.param_grads(sd, x, uv, tgt=torch.from_numpy(gold["target"]))
    assert np.abs(ls / gold["loss"] - 1.0).max() < 1e-12
    assert set("grad_" + k for k in sd) | {"target", "loss"} == set(gold.files)
    worst = max(O.rel_l1(grads[k].numpy(), gold["grad_" + k]) for k in sd)
    print("largest relative L1 of a parameter gradient against the fixture: %.2e" % worst)
    assert worst < 1e-12
    # and the numpy form of the kernel's definition agrees with the graph on the same low-resolution maps
    with torch.no_grad():
        outs = [o.permute(0, 2, 3, 1).numpy() for o in T.stage_outputs(sd, x)]
    heats = [o.astype(np.float32) for o in outs]
    loss, grad, _ = T.heatmap_mse(heats, uv, 5.0, [1.0] * 6)
    h32 = [torch.from_numpy(o).double().permute(0, 3, 1, 2).requires_grad_(True) for o in heats]
    tg = torch.from_numpy(gold["target"]).double()
    ref = [torch.nn.functional.mse_loss(torch.nn.functional.interpolate(o, scale_factor=8, mode="bilinear", align_corners=True), tg)
           for o in h32]
    sum(ref).backward()
    for s in range(6):
        # up is rounded to fp32 in the definition: 2^-24 relative on values of order 1 against a loss of 5e-2
        assert abs(loss[s] - float(ref[s].detach())) < 1e-6 * loss[s]
        assert np.abs(grad[s] - h32[s].grad.permute(0, 2, 3, 1).numpy()).max() < 1e-6 * np.abs(grad[s]).max()


def test_tap_matrix_is_the_transpose_of_the_upsample():
    for n in (1, 2, 3, 5, 32):
        A = T.tap_matrix(n, 8 * n)
        assert np.abs(A.sum(1) - 1.0).max() < 1e-15 and (A >= 0).all() and ((A > 0).sum(1) <= 2).all()
        v = O.hashed(12, n * n * 21, SEED).reshape(1, n, n, 21)
        assert np.abs(np.einsum("oy,px,byxj->bopj", A, A, v) - O.upsample(v)).max() < 1e-14


def test_no_test_pose_puts_a_target_pixel_on_a_cut():
    """premise of tests/test_hpe_train_gpu.py: no pixel of any target is within 1e-9 relative of 0.0099 or of 1, so an exp that
    differs from numpy's in the last place cannot move a pixel across a cut.  Every case and every pixel is counted, with one
    kind of pixel named apart: a joint exactly on a pixel (a case the issue asks for) has D2 == 0 there, exp(-0.0) is 1.0
    exactly and that IS the upper cut's value - the cut leaves it alone whichever way it is read."""
    for sigma in (5.0, 1.5):
        for h, w in SHAPES:
            for B in BATCHES:
                uv = T.poses(B, 8 * h, 8 * w, SEED)
                margin, on = T.cut_margin(uv, 8 * h, 8 * w, sigma)
                assert margin > 1e-9, (sigma, h, w, B, margin)
                assert on >= 3 * B                       # joints 0, 1, 2 sit on a pixel each
                t = T.target(uv, 8 * h, 8 * w, sigma)
                assert not t[..., 3].any()               # far outside: an all-zero map
                assert t[..., 4].any() and t[..., 4].max() < 1.0 and t[..., 5].any()        # just outside: a clipped bump
                assert np.array_equal(t[..., 6], t[..., 7]) and t[..., 6].any()             # two joints at one point
                assert t[:, 8 * h - 1, 0, 0].tolist() == [1.0] * B and t[:, 0, 8 * w - 1, 1].tolist() == [1.0] * B
                assert (uv[:, 8:] % 1.0 != 0).all()      # fractional coordinates
    # the poses of the trainer's tests
    assert T.cut_margin(T.poses(2, 32, 32, SEED), 32, 32, 5.0)[0] > 1e-9
