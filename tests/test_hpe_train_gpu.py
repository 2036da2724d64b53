"""Training the 2D hand-pose estimator on the device (csrc/hpe_train.hip, mmhand_amd/hpe_train.py, mmhand_amd/train_hpe.py)
against tests/_hpe_train_oracle.py: mmh_heatmap_mse against its float64 definition, the convolution backward on the estimator's
shapes against the exact oracle of tests/_exact.py, the whole network's parameter gradients and three Adam steps against the
float64 graph, and the command line end to end.  All weights are generated: no figure here says anything about a trained
estimator."""
import ctypes as C
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import _exact as E
from tests import _hpe_oracle as O
from tests import _hpe_train_oracle as T

pytestmark = pytest.mark.gpu
SEED = 0
SENTINEL = 12345.0
NARROW = {k: v for k, v in O.NARROW.items() if k != "fc"}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------- mmh_heatmap_mse
def heatmap_mse(dev, heats, uv, sigma, weights, dcs=None):
    """heats: S numpy fp32 [B,h,w,cs] -> (loss float64 [S], dheat S numpy [B,h,w,dcs] filled with SENTINEL before the call, or
    None when dcs is None)"""
    from mmhand_amd import lib as L, ops
    S = len(heats)
    B, h, w, cs = heats[0].shape
    hs = [torch.from_numpy(x).to(dev) for x in heats]
    uvt = torch.from_numpy(np.ascontiguousarray(uv, dtype=np.float64)).to(dev)
    nbytes = L.load().mmh_heatmap_mse_ws_bytes(S, B, h, w)
    assert nbytes > 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    loss = torch.full((S,), -1.0, dtype=torch.float64, device=dev)
    gs = None if dcs is None else [torch.full((B, h, w, dcs), SENTINEL, dtype=torch.float32, device=dev) for _ in range(S)]
    heat = (C.c_void_p * S)(*[t.data_ptr() for t in hs])
    dheat = None if gs is None else (C.c_void_p * S)(*[t.data_ptr() for t in gs])
    L.call("mmh_heatmap_mse", heat, S, B, h, w, cs, ops._ptr(uvt), float(sigma), (C.c_double * S)(*weights), ops._ptr(loss), dheat,
           dcs or 0, ops._ptr(ws), nbytes, ops._stream())
    return loss.cpu().numpy(), None if gs is None else [g.cpu().numpy() for g in gs]


def _heats(S, B, h, w, cs):
    """stage s: values in +-0.6 (a heat map's range and beyond); lanes from 21 up hold NaN - the kernel must not read them"""
    out = []
    for s in range(S):
        x = np.full((B, h, w, cs), np.nan, dtype=np.float32)
        x[..., :21] = (O.hashed(300 + s, B * h * w * 21, SEED).reshape(B, h, w, 21) * 0.6).astype(np.float32)
        out.append(x)
    return out


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [1, 6])
@pytest.mark.parametrize("h,w,cs,dcs", [(4, 4, 24, 24), (5, 3, 152, 24), (3, 5, 21, 152), (32, 32, 152, 24)])
def test_heatmap_mse_equals_its_definition(dev, h, w, cs, dcs, S, B):
    sigma = 5.0
    uv = T.poses(B, 8 * h, 8 * w, SEED)
    heats = _heats(S, B, h, w, cs)
    weights = [1.0, 0.5, 2.0, 0.25, 1.5, 1.0][:S]
    want_loss, want_g, terms = T.heatmap_mse(heats, uv, sigma, weights)
    loss, g = heatmap_mse(dev, heats, uv, sigma, weights, dcs)
    rel = np.abs(loss / want_loss - 1.0).max()
    off = 0
    for s in range(S):
        got = g[s][..., :21].astype(np.float64)
        err = np.abs(got - want_g[s])
        bound = 2.0 ** -24 * np.abs(want_g[s]) + 1e-13 * terms[s]
        off += int((_bits(g[s][..., :21]) != _bits(want_g[s].astype(np.float32))).sum())
        assert (err <= bound).all(), (s, float((err - bound).max()), np.argwhere(err > bound)[:4])
        assert not g[s][..., 21:24].any()                                   # lanes 21..23: zeros
        assert (g[s][..., 24:] == SENTINEL).all()                           # every other lane: untouched
    print("loss rel %.2e; gradient elements not bit-equal to the rounded oracle: %d of %d" % (rel, off, S * B * h * w * 21))
    assert rel <= 1e-12, (loss, want_loss)
    # dheat = NULL: the same loss bits; and a second run: the same bits everywhere
    only, none = heatmap_mse(dev, heats, uv, sigma, weights, None)
    assert none is None and np.array_equal(only.view(np.uint64), loss.view(np.uint64))
    loss2, g2 = heatmap_mse(dev, heats, uv, sigma, weights, dcs)
    assert np.array_equal(loss2.view(np.uint64), loss.view(np.uint64))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(g, g2))


@pytest.mark.parametrize("h,w,sigma", [(4, 4, 5.0), (5, 3, 1.5), (32, 32, 5.0)])
def test_heatmap_mse_of_zero_maps_is_the_mean_squared_target(dev, h, w, sigma):
    """heat = 0, S = 1: up = 0, so loss = mean(t^2) and dheat = the transposed upsample of -2 t / N - this pins the target alone"""
    B = 3
    uv = T.poses(B, 8 * h, 8 * w, SEED)
    t = T.target(uv, 8 * h, 8 * w, sigma).astype(np.float64)
    loss, g = heatmap_mse(dev, [np.zeros((B, h, w, 24), dtype=np.float32)], uv, sigma, [1.0], 24)
    assert abs(loss[0] / np.mean(t * t) - 1.0) <= 1e-12
    n = float(t.size)
    want = np.einsum("oy,px,bopj->byxj", T.tap_matrix(h, 8 * h), T.tap_matrix(w, 8 * w), -2.0 / n * t)
    assert np.abs(g[0][..., :21] - want).max() <= 2.0 ** -23 * np.abs(want).max()
    assert not g[0][..., 3].any()                                           # the far-outside joint: an all-zero target


def test_lane_add_adds_a_lane_range_and_nothing_else(dev):
    from mmhand_amd import lib as L, ops
    x = E.ints((2, 5, 3, 152), 11, lo=-8, hi=8).to(dev)
    y = E.ints((2, 5, 3, 28), 12, lo=-8, hi=8).to(dev)
    want = y.clone()
    want[..., 4:28] += x[..., 24:48]
    L.call("mmh_lane_add", C.c_void_p(x.data_ptr() + 4 * 24), 152, C.c_void_p(y.data_ptr() + 4 * 4), 28, 30, 24, ops._stream())
    assert torch.equal(y, want)


@pytest.mark.parametrize("B,H,W_,Cout,y_cs", [(2, 5, 7, 8, 8), (1, 1, 1, 4, 12), (3, 16, 9, 64, 64), (1, 8, 8, 256, 260), (2, 3, 33, 68, 68)])
def test_first_layer_with_float64_accumulation_is_bit_identical(dev, B, H, W_, Cout, y_cs):
    """mmh_conv3x3_c4_fprop_f64 against its definition in numpy: the same bits (zeros of either sign are one value), with and
    without ReLU, inside a wider buffer whose other lanes stay; 16 pixels and 64 lanes per workgroup pass: 105 and 297 pixels are
    ragged, 68 and 256 lanes take a second pass"""
    from mmhand_amd import lib as L, ops
    x = (O.hashed(400, B * H * W_ * 4, SEED).reshape(B, H, W_, 4)).astype(np.float32)
    x[..., 3] = 0
    w = O.hashed(401, 36 * Cout, SEED).reshape(3, 3, 4, Cout).astype(np.float32)
    b = (O.hashed(402, Cout, SEED) * 0.05).astype(np.float32)
    xt, wt, bt = (torch.from_numpy(a).to(dev) for a in (x, w, b))
    for act in (L.ACT_RELU, L.ACT_NONE):
        y = torch.full((B, H, W_, y_cs), SENTINEL, dtype=torch.float32, device=dev)
        L.call("mmh_conv3x3_c4_fprop_f64", ops._ptr(xt), ops._ptr(wt), ops._ptr(bt), ops._ptr(y), B, H, W_, Cout, y_cs, act,
               ops._stream())
        got = y.cpu().numpy()
        want = T.conv3x3_c4_f64(x, w, b, relu=act == L.ACT_RELU)
        assert np.array_equal(got[..., :Cout], want), np.argwhere(got[..., :Cout] != want)[:4]
        assert (got[..., Cout:] == SENTINEL).all()
        if act == L.ACT_RELU:
            assert (got[..., :Cout] == 0).any() and (got[..., :Cout] > 0).any() or H * W_ == 1


# ------------------------------------------------------------------------------------------------- convolution backward
# (k, Cin, Cout, lanes of the buffer x is read from, x's first lane, lanes of the buffer dy is read from, dy's first lane)
BWD = [pytest.param(7, 152, 128, 152, 0, 128, 0, id="7x7_152_128"), pytest.param(7, 128, 128, 128, 0, 128, 0, id="7x7_128_128"),
       pytest.param(1, 128, 24, 128, 0, 24, 0, id="1x1_128_24"), pytest.param(1, 512, 24, 512, 0, 24, 0, id="1x1_512_24"),
       pytest.param(1, 128, 512, 152, 24, 512, 0, id="1x1_128_512_read_at_a_lane_offset"),
       pytest.param(3, 512, 128, 512, 0, 152, 24, id="3x3_512_128_written_at_a_lane_offset")]


@pytest.mark.parametrize("k,Cin,Cout,x_cs,x_off,y_cs,y_off", BWD)
def test_conv_backward_is_exact_on_the_estimators_shapes(dev, k, Cin, Cout, x_cs, x_off, y_cs, y_off):
    """mmh_conv2d_dgrad / mmh_conv2d_wgrad / mmh_colsum as the trainer calls them (fp32, zero padding, 8 x 8, B = 2), the input
    and the output gradient inside wider buffers where the network has them there; integer data: every element exact"""
    from mmhand_amd import lib as L, ops
    B, H, W_ = 2, 8, 8
    P = E.problem(B, H, W_, Cin, Cout, k, 1, k // 2, False)
    xb = torch.full((B, H, W_, x_cs), SENTINEL, dtype=torch.float32)
    xb[..., x_off:x_off + Cin] = P.x
    gb = torch.full((B, H, W_, y_cs), SENTINEL, dtype=torch.float32)
    gb[..., y_off:y_off + Cout] = P.dy
    xb, gb, w = xb.to(dev), gb.to(dev), P.w.to(dev)
    d = ops.conv_desc(B, H, W_, Cin, Cout, k, 1, k // 2, False, x_cs=x_cs, y_cs=y_cs)
    xp, gp, st = C.c_void_p(xb.data_ptr() + 4 * x_off), C.c_void_p(gb.data_ptr() + 4 * y_off), ops._stream()
    dw = torch.full((k, k, Cin, Cout), SENTINEL, dtype=torch.float32, device=dev)
    ws = ops._ws(L.load().mmh_conv2d_wgrad_ws_bytes(C.byref(d)), dw)
    L.call("mmh_conv2d_wgrad", C.byref(d), xp, gp, ops._ptr(dw), ops._ptr(ws), ws.numel() * 4, 0, 0, st)
    E.assert_exact(dw, P.dw, "wgrad")
    # dx into a wider buffer too: the lanes beside it stay as they were
    dxb = torch.full((B, H, W_, x_cs), SENTINEL, dtype=torch.float32, device=dev)
    L.call("mmh_conv2d_dgrad", C.byref(d), gp, ops._ptr(w), C.c_void_p(dxb.data_ptr() + 4 * x_off), x_cs, st)
    E.assert_exact(dxb[..., x_off:x_off + Cin], P.dx, "dgrad")
    rest = torch.cat((dxb[..., :x_off], dxb[..., x_off + Cin:]), 3)
    assert (rest == SENTINEL).all()
    db = torch.full((Cout,), SENTINEL, dtype=torch.float32, device=dev)
    cw = ops._ws(L.load().mmh_colsum_ws_bytes(B * H * W_, Cout), db)
    L.call("mmh_colsum", gp, B * H * W_, Cout, y_cs, ops._ptr(db), ops._ptr(cw), cw.numel() * 4, 0, L.F32, st)
    E.assert_exact(db, P.db, "bias gradient")


# ------------------------------------------------------------------------------------------------- the whole network
def _case(dev, widths):
    """one forward + loss + backward of the trainer on hashed weights and images (B = 2, 32 x 32), next to the float64 graph and
    PyTorch's fp32 CPU backward of the same graph on the weights the device got"""
    from mmhand_amd import hpe_train, ops
    sd = OrderedDict((k, v.float()) for k, v in O.state_dict("2d", widths, seed=SEED).items())
    img = O.images(2, 32, 32, SEED)
    uv = T.poses(2, 32, 32, SEED)
    tr = hpe_train.Hpm2dTrainer(dev).load_state_dict(sd)
    tr.forward(ops.hpe_normalize(torch.from_numpy(img).to(dev)))
    cats = [c.cpu().numpy() for c in tr._kept["cats"]]
    losses, G = tr.loss(uv)
    tr.backward(G)
    x = torch.from_numpy(O.normalize(img)[..., :3]).permute(0, 3, 1, 2)
    l64, g64 = T.param_grads(sd, x, uv, dtype=torch.float64)
    l32, g32 = T.param_grads(sd, x, uv, dtype=torch.float32)
    return dict(tr=tr, cats=cats, losses=losses.cpu().numpy(), grads=tr.grads(), l64=l64, g64=g64, l32=l32, g32=g32, sd=sd)


@pytest.fixture(scope="module")
def full(dev):
    return _case(dev, O.FULL)


@pytest.fixture(scope="module")
def narrow(dev):
    return _case(dev, O.NARROW)


@pytest.mark.parametrize("which", ["full", "narrow"])
def test_parameter_gradients_stay_within_twice_pytorch_fp32(which, request):
    """relative L1 per parameter tensor against the float64 graph: the median and the maximum over the tensors at most twice
    those of PyTorch's fp32 CPU backward (DESIGN 4.5g's bar: room for another summation order and nothing else).

    Measured on an MI355X.  narrow: device median 1.91e-7 / maximum 7.37e-7, PyTorch 2.20e-7 / 7.56e-7.  full: device median
    7.29e-7 / maximum 1.33e-6 (stage6.conv2.weight), PyTorch 9.55e-7 / 2.40e-6.  With conv1_1's forward on the fp32 direct
    kernel the full maximum was 3.78e-5 at conv1_1.weight: the float64 graph's pre-activation at (b 1, c 12, y 8, x 17) is
    -1.49e-8, inside the fp32 rounding of that 27-term sum, the fp32 kernel landed above zero and that single ReLU mask is worth
    3.71e-5 of sum |dw|; the trainer's first layer accumulates in float64 for that reason (mmh_conv3x3_c4_fprop_f64).  DESIGN 4.5i."""
    c = request.getfixturevalue(which)
    dev_d = np.array([O.rel_l1(c["grads"][k].numpy(), c["g64"][k].numpy()) for k in c["sd"]])
    ref_d = np.array([O.rel_l1(c["g32"][k].numpy(), c["g64"][k].numpy()) for k in c["sd"]])
    print("%s widths, %d tensors: device median %.3e max %.3e; PyTorch fp32 median %.3e max %.3e; losses rel %.2e (PyTorch %.2e)"
          % (which, len(dev_d), np.median(dev_d), dev_d.max(), np.median(ref_d), ref_d.max(),
             np.abs(c["losses"] / c["l64"] - 1).max(), np.abs(c["l32"] / c["l64"] - 1).max()))
    worst = list(c["sd"])[int(dev_d.argmax())]
    print("largest device distance: %s; PyTorch's there %.3e" % (worst, ref_d[int(dev_d.argmax())]))
    assert not any(cat[..., 21:24].any() for cat in c["cats"])
    assert np.abs(c["losses"] / c["l64"] - 1).max() <= 1e-4
    assert np.median(dev_d) <= 2.0 * np.median(ref_d), (np.median(dev_d), np.median(ref_d))
    assert dev_d.max() <= 2.0 * ref_d.max(), (dev_d.max(), ref_d.max(), worst)
    # the gradient buffer's padding is exactly zero
    tr = c["tr"]
    assert not tr.g.cpu()[tr.padding_mask()].any()


def test_three_steps_follow_the_float64_trace_and_keep_the_padding_zero(dev):
    from mmhand_amd import hpe, hpe_train, lib as L
    sd = OrderedDict((k, v.float()) for k, v in O.state_dict("2d", O.NARROW, seed=SEED).items())
    img = O.images(2, 32, 32, SEED)
    uv = T.poses(2, 32, 32, SEED)
    x = torch.from_numpy(O.normalize(img)[..., :3]).permute(0, 3, 1, 2)
    want, want_p = T.adam_trace(sd, x, uv, steps=3, lr=1e-4)
    other = 1 if L.get_option("conv_levels") != 1 else 2
    with E.option("conv_levels", other):
        tr = hpe_train.Hpm2dTrainer(dev, lr=1e-4).load_state_dict(sd)
        images = torch.from_numpy(img).to(dev)
        got = np.stack([tr.step(images, uv).cpu().numpy() for _ in range(3)])
        assert L.get_option("conv_levels") == other                         # put back after every forward
    rel = np.abs(got / want - 1.0)
    print("18 stage losses against the float64 trace: largest relative distance %.2e" % rel.max())
    assert got.shape == (3, 6) and rel.max() <= 1e-3, rel
    assert tr.steps == 3
    mask = tr.padding_mask()
    assert int(mask.sum()) > 0
    for name, buf in (("weights", tr.p), ("gradients", tr.g), ("first moments", tr.m), ("second moments", tr.v)):
        assert not buf.cpu()[mask].any(), name
    assert tr.m.cpu()[~mask].any() and tr.v.cpu()[~mask].any()
    out = tr.state_dict()
    moved = max(float((out[k].double() - want_p[k]).abs().max()) for k in sd)
    print("largest distance of a parameter from the float64 trace after three steps: %.2e (a step is 1e-4)" % moved)
    assert all(not torch.equal(out[k], sd[k]) for k in sd if k.endswith(".weight"))
    # the checkpoint loads into the inference network, whose forward gives the trainer's last stage output for these weights
    net = hpe.Hpm2d(dev).load_state_dict(out)
    assert sorted(net.convs) == sorted(tr.meta)


# ------------------------------------------------------------------------------------------------- the command line
@pytest.fixture
def work_dir():
    """a scratch directory whose PATH does not contain "test" (the loader keys on it)"""
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="mmh_hpt_")
    assert "test" not in d
    yield d
    shutil.rmtree(d, ignore_errors=True)


def test_train_hpe_writes_a_checkpoint_that_evaluate_scores(dev, work_dir, monkeypatch):
    from mmhand_amd import evaluate, hpe, hpe_train, train_hpe
    from tests._dataset_fixture import write_rhd
    root, extra, val = (os.path.join(work_dir, n) for n in ("rhd", "novel", "val"))
    write_rhd(root, n=7, size=32)
    write_rhd(extra, n=3, size=32, seed=9)
    write_rhd(val, n=4, size=32, seed=10)
    monkeypatch.chdir(work_dir)
    monkeypatch.setattr(train_hpe, "INIT_WIDTHS", NARROW)
    seen = []
    step = hpe_train.Hpm2dTrainer.step

    def spy(self, images, uv, layout="nchw", lr=None):
        seen.append((tuple(images.shape), images.dtype, layout, lr, np.array(uv)))
        return step(self, images, uv, layout, lr)

    monkeypatch.setattr(hpe_train.Hpm2dTrainer, "step", spy)
    log = train_hpe.main(["--dataroot", root, "--extra_dataroot", extra, "--dataset", "rhd", "--name", "t", "--niter", "1",
                          "--niter_decay", "1", "--batchSize", "4", "--init_seed", "3", "--val_dataroot", val,
                          "--save_epoch_freq", "2", "--threads", "2"])
    # 10 images in batches of 4, two epochs, the second at half the rate; bytes as the loader reads them
    assert [s[0] for s in seen] == [(4, 32, 32, 3), (4, 32, 32, 3), (2, 32, 32, 3)] * 2
    assert all(s[1] == torch.uint8 and s[2] == "bgr_hwc" for s in seen)
    assert [s[3] for s in seen] == [1e-4] * 3 + [pytest.approx(0.5e-4)] * 3
    assert len(log) == 2 and log[0]["images"] == 10 and len(log[0]["loss"]) == 6 and np.isfinite(log[1]["loss"]).all()
    assert 0.0 <= log[1]["pck2d_auc"] <= 1.0 and log[1]["epe2d_mean"] >= 0.0
    ckpt = os.path.join("checkpoints", "t")
    assert sorted(os.listdir(ckpt)) == ["2_net_Hpm2d.pth", "latest_net_Hpm2d.pth", "train_hpe_log.json"]
    sd = torch.load(os.path.join(ckpt, "latest_net_Hpm2d.pth"), map_location="cpu")
    start = hpe_train.init_state_dict(3, NARROW)
    assert O.keys_and_shapes(sd) == O.keys_and_shapes(start) and not torch.equal(sd["stage6.conv7.weight"], start["stage6.conv7.weight"])
    hpe.Hpm2d(dev).load_state_dict(sd)
    res = evaluate.main(["--pck_images", val, "--dataset", "rhd", "--hpm2d", os.path.join(ckpt, "latest_net_Hpm2d.pth"),
                         "--batchSize", "4", "--results_json", "v.json"])
    assert res["summary"]["n"] == 4 and res["summary"]["pck2d_auc"] == log[1]["pck2d_auc"]
    assert json.load(open("v.json"))["summary"]["epe2d_mean"] == log[1]["epe2d_mean"]
