"""Training the 3D hand-pose estimator on the device (csrc/hpe3d_train.hip, mmhand_amd/hpe_train.py: Hpm3dTrainer,
mmhand_amd/train_hpe.py --net hpm3d) against tests/_hpe3d_train_oracle.py: the four kernels against their float64 definitions,
the whole network's parameter gradients and three Adam steps against the float64 graph, and the command line end to end.  All
weights are generated: no figure here says anything about a trained estimator."""
import functools
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import _hpe_oracle as O
from tests import _hpe_train_oracle as T
from tests import _hpe3d_train_oracle as T3

pytestmark = pytest.mark.gpu
SEED = 0
SENTINEL = 12345.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ulps(a, b):
    """the distance of two fp32 arrays of one sign pattern in units in the last place"""
    return np.abs(_bits(a).astype(np.int64) - _bits(b).astype(np.int64))


# ------------------------------------------------------------------------------------------------- mmh_gauss_heatmaps
@functools.lru_cache(maxsize=None)
def _target(B, H, W_, sigma):
    uv = T.poses(B, H, W_, SEED)
    return uv, T.target(uv, H, W_, sigma)


@pytest.mark.parametrize("cs", [24, 152])
@pytest.mark.parametrize("sigma", [5.0, 1.5])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W_", [(32, 32), (40, 24), (24, 40), (256, 256)])
def test_gauss_heatmaps_are_the_loss_kernels_target(dev, H, W_, B, sigma, cs):
    """Measured on an MI355X: every element of every case bit-equal to the float64 numpy target rounded once."""
    from mmhand_amd import ops
    uv, want = _target(B, H, W_, sigma)
    out = torch.full((B, H, W_, cs), SENTINEL, dtype=torch.float32, device=dev)
    assert ops.gauss_heatmaps(uv, H, W_, sigma, out=out) is out
    got = out.cpu().numpy()
    maps = got[..., :21]
    assert np.array_equal(maps == 0, want == 0)                             # the zero pattern: both cuts and the skipped exp
    assert (maps >= 0).all() and (maps <= 1).all()
    off = int((_bits(maps) != _bits(want)).sum())
    print("elements not bit-equal to the rounded oracle: %d of %d" % (off, want.size))
    assert _ulps(maps, want).max() <= 1
    assert not got[..., 21:24].any() and (got[..., 24:] == SENTINEL).all()  # lanes 21..23 zeros, every other lane untouched
    again = torch.full((B, H, W_, cs), SENTINEL, dtype=torch.float32, device=dev)
    ops.gauss_heatmaps(torch.from_numpy(uv).to(dev), H, W_, sigma, out=again)
    assert torch.equal(again, out)
    if cs == 24:
        assert torch.equal(ops.gauss_heatmaps(uv, H, W_, sigma, device=dev), out)


# ------------------------------------------------------------------------------------------------- mmh_smooth_l1
@pytest.mark.parametrize("beta", [1.0, 0.5])
@pytest.mark.parametrize("ps", [24, 28])
@pytest.mark.parametrize("M", [1, 3, 64])
def test_smooth_l1_equals_its_definition(dev, M, ps, beta):
    from mmhand_amd import lib as L, ops
    n = 21
    pred = np.full((M, ps), np.nan, dtype=np.float32)                       # lanes from 21 up: the kernel must not read them
    pred[:, :n] = (O.hashed(500, M * n, SEED) * 0.5).reshape(M, n)
    target = np.float64(pred[:, :n]) - (O.hashed(501, M * n, SEED) * 1.6 * beta).reshape(M, n)      # both branches
    planted = [0.0, beta, -beta, beta * (1 - 2.0 ** -40), -beta * (1 - 2.0 ** -40), beta * (1 + 2.0 ** -40), -beta * (1 + 2.0 ** -40),
               250.0, -1e6]
    target[0, :len(planted)] = np.float64(pred[0, :len(planted)]) - np.array(planted)
    d = np.float64(pred[:, :n]) - target
    assert (np.abs(d) < beta).any() and (np.abs(d) >= beta).any() and (np.abs(d[0, 1:3]) == beta).all() and d[0, 0] == 0
    for scale in (10.0, 1.0):
        want_loss, want_g = T3.smooth_l1(pred, target, n, beta, scale)
        p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(target).to(dev)
        loss = torch.full((1,), -1.0, dtype=torch.float64, device=dev)
        g = torch.full((M, 28), SENTINEL, dtype=torch.float32, device=dev)
        L.call("mmh_smooth_l1", ops._ptr(p), ps, ops._ptr(t), M, n, beta, scale, ops._ptr(loss), ops._ptr(g), 28, ops._stream())
        got, got_loss = g.cpu().numpy(), float(loss.cpu())
        assert abs(got_loss / want_loss - 1.0) <= 1e-15, (got_loss, want_loss)
        # bit-equal to the definition rounded once (zeros of either sign are one value)
        assert np.array_equal(got[:, :24], want_g.astype(np.float32))
        assert not got[:, 21:24].any() and (got[:, 24:] == SENTINEL).all()
        only = torch.full((1,), -1.0, dtype=torch.float64, device=dev)
        L.call("mmh_smooth_l1", ops._ptr(p), ps, ops._ptr(t), M, n, beta, scale, ops._ptr(only), None, 0, ops._stream())
        assert only.cpu().numpy().view(np.uint64) == loss.cpu().numpy().view(np.uint64)
        l2, g2 = ops.smooth_l1(p, target, n, beta, scale)
        assert l2.cpu().numpy().view(np.uint64) == loss.cpu().numpy().view(np.uint64) and np.array_equal(_bits(g2.cpu().numpy()), _bits(got[:, :24]))
        assert ops.smooth_l1(p, t, n, beta, scale, with_grad=False)[1] is None


# ------------------------------------------------------------------------------------------------- nn.Linear backward
LINEAR = [(1, 4, 4), (3, 384, 16), (64, 515, 24), (5, 512, 512), (33, 24576, 512)]


def _linear(dev, x, dy, wt):
    from mmhand_amd import ops
    xt, gt, wtt = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (x, dy, wt))
    dx = ops.linear_dgrad(gt, wtt)
    dwt = torch.full(tuple(wtt.shape), SENTINEL, dtype=torch.float32, device=dev)
    db = torch.full((wtt.shape[1],), SENTINEL, dtype=torch.float32, device=dev)
    ops.linear_wgrad(xt, gt, dwt, db)
    dwt2, none = ops.linear_wgrad(xt, gt, with_bias=False)
    assert none is None and torch.equal(dwt2, dwt)
    assert torch.equal(ops.linear_dgrad(gt, wtt), dx)                       # a second run: the same bits
    return dx.cpu().numpy(), dwt.cpu().numpy(), db.cpu().numpy()


@pytest.mark.parametrize("M,K,N", LINEAR)
def test_linear_backward_is_exact_on_integers(dev, M, K, N):
    """x, dy, wt integers in [-4, 4]: every product and every partial sum is an integer below 2^14 (512 * 16), so every element
    of dx, dwt and db is exact whatever the order; zero rows of x and zero columns of dy give exact zeros"""
    ints = lambda t, n: np.floor(O.hashed(t, n, SEED) * 4.5 + 0.5)                                  # noqa: E731
    x, dy, wt = ints(600, M * K).reshape(M, K), ints(601, M * N).reshape(M, N), ints(602, K * N).reshape(K, N)
    assert np.abs(x).max() <= 4 and np.abs(wt).max() <= 4 and np.abs(dy).max() <= 4
    x[:, K // 2] = 0                                                        # a padding row of wt's layout
    dy[:, N - 1] = 0                                                        # a padding column
    dx, dwt, db = _linear(dev, x, dy, wt)
    want_dx, _ = T3.linear_dgrad(dy, wt)
    want_dwt, want_db, _, _ = T3.linear_wgrad(x, dy)
    assert np.abs(want_dx).max() < 2 ** 14 and np.abs(want_dwt).max() < 2 ** 14
    assert np.array_equal(dx, want_dx) and np.array_equal(dwt, want_dwt) and np.array_equal(db, want_db)
    assert not dwt[K // 2].any() and not dwt[:, N - 1].any() and db[N - 1] == 0


@pytest.mark.parametrize("M,K,N", LINEAR)
def test_linear_backward_stays_within_one_fma_chains_bound(dev, M, K, N):
    """hashed real data: every element within gamma_L * sum |terms| of float64, L the chain's length (N for dx, M for dwt and
    db): the standard bound of one fma chain"""
    x = O.hashed(610, M * K, SEED).reshape(M, K).astype(np.float32)
    dy = (O.hashed(611, M * N, SEED) * 0.1).reshape(M, N).astype(np.float32)
    wt = (O.hashed(612, K * N, SEED) * 0.05).reshape(K, N).astype(np.float32)
    dx, dwt, db = _linear(dev, x, dy, wt)
    want_dx, tx = T3.linear_dgrad(dy, wt)
    want_dwt, want_db, tw, tb = T3.linear_wgrad(x, dy)
    for name, got, want, terms, chain in (("dx", dx, want_dx, tx, N), ("dwt", dwt, want_dwt, tw, M), ("db", db, want_db, tb, M)):
        err, bound = np.abs(got - want), T3.gamma(chain) * terms
        print("%s: largest error / bound %.3f" % (name, float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all(), (name, float((err - bound).max()))


# ------------------------------------------------------------------------------------------------- two-level dgrad
@pytest.mark.parametrize("k,Cin,Cout", [(7, 152, 128), (7, 128, 128), (3, 512, 128), (1, 128, 24), (3, 68, 8), (3, 64, 128)])
def test_two_level_dgrad_is_exact_on_integers(dev, k, Cin, Cout):
    """mmh_conv2d_dgrad under mmh_set_option("dgrad_levels", 2), as Hpm3dTrainer.backward calls it (fp32, zero padding, 8 x 8,
    B = 2, odd batch of rows: 128 pixels = one row tile; Cin 152 and 68: a ragged column tile): integer data, every element
    exact, written into a wider buffer whose other lanes stay; with 64 input channels the option changes nothing"""
    import ctypes as C
    from mmhand_amd import lib as L, ops
    from tests import _exact as E
    B, H, W_ = 2, 8, 8
    P = E.problem(B, H, W_, Cin, Cout, k, 1, k // 2, False)
    dy, w = P.dy.to(dev), P.w.to(dev)
    d = ops.conv_desc(B, H, W_, Cin, Cout, k, 1, k // 2, False, x_cs=Cin + 8, y_cs=Cout)
    outs = []
    for levels in (1, 2):
        with E.option("dgrad_levels", levels):
            dx = torch.full((B, H, W_, Cin + 8), SENTINEL, dtype=torch.float32, device=dev)
            L.call("mmh_conv2d_dgrad", C.byref(d), ops._ptr(dy), ops._ptr(w), C.c_void_p(dx.data_ptr() + 16), Cin + 8, ops._stream())
        assert L.get_option("dgrad_levels") == 1
        E.assert_exact(dx[..., 4:4 + Cin], P.dx, "dgrad, levels %d" % levels)
        assert (dx[..., :4] == SENTINEL).all() and (dx[..., 4 + Cin:] == SENTINEL).all()
        outs.append(dx)
    assert torch.equal(outs[0], outs[1])


def test_two_level_dgrad_is_closer_to_float64(dev):
    """hashed real data on the Repeat block's 7 x 7 x 128 shape: both summations within the bound of one fp32 chain over the
    6272 terms, gamma_K * sum |terms|; the two-level sum's distance from float64 is printed next to the one-level sum's"""
    import ctypes as C
    from mmhand_amd import lib as L, ops
    from tests import _exact as E
    B, H, W_, Cc, k = 2, 8, 8, 128, 7
    dy = (O.hashed(700, B * H * W_ * Cc, SEED) * 0.1).reshape(B, H, W_, Cc).astype(np.float32)
    w = (O.hashed(701, k * k * Cc * Cc, SEED) * 0.02).reshape(k, k, Cc, Cc).astype(np.float32)                 # RSCK
    want = torch.nn.functional.conv_transpose2d(torch.from_numpy(dy).double().permute(0, 3, 1, 2), torch.from_numpy(w).double().permute(3, 2, 0, 1),
                                                padding=k // 2).permute(0, 2, 3, 1).numpy()
    terms = torch.nn.functional.conv_transpose2d(torch.from_numpy(np.abs(dy)).double().permute(0, 3, 1, 2),
                                                 torch.from_numpy(np.abs(w)).double().permute(3, 2, 0, 1), padding=k // 2).permute(0, 2, 3, 1).numpy()
    d = ops.conv_desc(B, H, W_, Cc, Cc, k, 1, k // 2, False, x_cs=Cc, y_cs=Cc)
    dyt, wt = torch.from_numpy(dy).to(dev), torch.from_numpy(w).to(dev)
    dist = {}
    for levels in (1, 2):
        with E.option("dgrad_levels", levels):
            dx = torch.empty((B, H, W_, Cc), dtype=torch.float32, device=dev)
            L.call("mmh_conv2d_dgrad", C.byref(d), ops._ptr(dyt), ops._ptr(wt), ops._ptr(dx), Cc, ops._stream())
        got = dx.cpu().numpy()
        assert (np.abs(got - want) <= T3.gamma(k * k * Cc) * terms).all()
        dist[levels] = O.rel_l1(got, want)
    print("7 x 7 x 128 dgrad, relative L1 against float64: one level %.3e, two levels %.3e" % (dist[1], dist[2]))


# ------------------------------------------------------------------------------------------------- the whole network
def _sd(widths):
    return OrderedDict((k, v.float()) for k, v in O.state_dict("3d", widths, head_hw=4, seed=SEED).items())


def _case(dev, widths):
    """one forward + loss + backward of the trainer on hashed weights and the fixture's inputs (B = 2, 32 x 32), next to the
    float64 graph and PyTorch's fp32 CPU backward of the same graph on the weights the device got"""
    from mmhand_amd import hpe_train
    sd = _sd(widths)
    heat, z = T3.inputs(SEED)
    x = torch.from_numpy(T3.gauss_heatmaps(T.poses(2, 32, 32, SEED), 32, 32, 5.0)).to(dev)
    tr = hpe_train.Hpm3dTrainer(dev).load_state_dict(sd)
    out = tr.forward(x)
    kept = tr._kept
    loss, g = tr.loss(z)
    tr.backward(g)
    xt, zt = T3.nchw(heat), torch.from_numpy(z)
    l64, o64, g64, none = T3.param_grads(sd, xt, zt, dtype=torch.float64)
    l32, o32, g32, _ = T3.param_grads(sd, xt, zt, dtype=torch.float32)
    return dict(tr=tr, out=out.cpu().numpy(), d=kept["d"].cpu().numpy(), cats=[c.cpu().numpy() for c in kept["cats"]],
                loss=float(loss.cpu()), grads=tr.grads(), l64=l64, o64=o64, g64=g64, l32=l32, o32=o32, g32=g32, none=none, sd=sd)


@pytest.fixture(scope="module")
def full(dev):
    return _case(dev, O.FULL)


@pytest.fixture(scope="module")
def narrow(dev):
    return _case(dev, O.NARROW)


@pytest.mark.parametrize("which", ["full", "narrow"])
def test_parameter_gradients_stay_within_twice_pytorch_fp32(which, request):
    """the 42 outputs and the loss within 1e-4 relative of the float64 graph; relative L1 per parameter tensor with a gradient
    (110) against the float64 graph: the median and the maximum over the tensors at most twice those of PyTorch's fp32 CPU
    backward (DESIGN 4.5g's bar: room for another summation order and nothing else).  PyTorch's side, measured on the CPU:
    narrow median 6.4e-7 / maximum 2.5e-6, full 9.5e-7 / 1.6e-6 (they move with the host's thread count).

    Measured on an MI355X.  narrow: device median 5.19e-7 / maximum 1.01e-6 (conv3_4.weight), PyTorch there 6.80e-7 / 2.26e-6.
    full: device median 9.80e-7 / maximum 1.72e-6 (stage2.conv2.weight), PyTorch there 1.10e-6 / 1.78e-6.  With mmh_conv2d_dgrad's
    one-level sum the full figures were 2.19e-6 / 3.47e-6, growing block by block towards the input: the trainer's backward runs
    under mmh_set_option("dgrad_levels", 2) for that reason.  DESIGN 4.5j."""
    c = request.getfixturevalue(which)
    keys = list(c["g64"])
    assert len(keys) == 110 and set(c["grads"]) == set(keys) and all(k.startswith("stage6.") for k in c["none"])
    assert all(c["g64"][k].abs().sum() > 0 for k in keys)
    dev_d = np.array([O.rel_l1(c["grads"][k].numpy(), c["g64"][k].numpy()) for k in keys])
    ref_d = np.array([O.rel_l1(c["g32"][k].numpy(), c["g64"][k].numpy()) for k in keys])
    out_rel = np.abs(c["out"][:, :21] - c["o64"]).max() / np.abs(c["o64"]).max()
    print("%s widths, %d tensors: device median %.3e max %.3e; PyTorch fp32 median %.3e max %.3e; loss rel %.2e (PyTorch %.2e); "
          "outputs rel %.2e" % (which, len(dev_d), np.median(dev_d), dev_d.max(), np.median(ref_d), ref_d.max(),
                                abs(c["loss"] / c["l64"] - 1), abs(c["l32"] / c["l64"] - 1), out_rel))
    worst = keys[int(dev_d.argmax())]
    print("largest device distance: %s; PyTorch's there %.3e" % (worst, ref_d[int(dev_d.argmax())]))
    assert not c["out"][:, 21:].any() and not c["d"][..., 21:].any() and not any(cat[..., 21:24].any() for cat in c["cats"])
    assert np.abs(c["out"][:, :21] / c["o64"] - 1.0).max() <= 1e-4 and abs(c["loss"] / c["l64"] - 1.0) <= 1e-4
    assert np.median(dev_d) <= 2.0 * np.median(ref_d), (np.median(dev_d), np.median(ref_d))
    assert dev_d.max() <= 2.0 * ref_d.max(), (dev_d.max(), ref_d.max(), worst)
    # the gradient buffer's padding is exactly zero
    tr = c["tr"]
    assert not tr.g.cpu()[tr.padding_mask()].any()


def test_three_steps_follow_the_float64_trace_and_keep_the_padding_zero(dev):
    from mmhand_amd import hpe, hpe_train, lib as L
    from tests import _exact as E
    sd = _sd(O.NARROW)
    heat, z = T3.inputs(SEED)
    want, _ = T3.adam_trace(sd, T3.nchw(heat), torch.from_numpy(z), steps=3, lr=2e-4, beta1=0.5)
    assert np.abs(want - np.array([2.0301, 2.0118, 1.9945])).max() < 1e-4
    uv = T.poses(2, 32, 32, SEED)
    other = 1 if L.get_option("conv_levels") != 1 else 2
    with E.option("conv_levels", other):
        tr = hpe_train.Hpm3dTrainer(dev, lr=2e-4, beta1=0.5).load_state_dict(sd)
        got = np.array([float(tr.step(uv, z).cpu()) for _ in range(3)])     # the input rendered by mmh_gauss_heatmaps
        assert L.get_option("conv_levels") == other                         # put back after every forward
    rel = np.abs(got / want - 1.0)
    print("three losses %s against the float64 trace %s: largest relative distance %.2e" % (got, want, rel.max()))
    assert rel.max() <= 1e-3, rel
    assert tr.steps == 3
    mask = tr.padding_mask()
    assert int(mask.sum()) > 0
    for name, buf in (("weights", tr.p), ("gradients", tr.g), ("first moments", tr.m), ("second moments", tr.v)):
        assert not buf.cpu()[mask].any(), name
    assert tr.m.cpu()[~mask].any() and tr.v.cpu()[~mask].any()
    out = tr.state_dict()
    assert list(out) == list(sd) and all(out[k].shape == sd[k].shape for k in sd)
    for k in sd:
        if k.startswith("stage6."):
            assert torch.equal(out[k], sd[k]), k                            # not run, no gradient: bit for bit
        elif k.endswith(".weight"):
            assert not torch.equal(out[k], sd[k]), k
    net = hpe.Hpm3d(dev).load_state_dict(out)
    x = torch.from_numpy(T3.gauss_heatmaps(uv, 32, 32, 5.0)).to(dev)
    assert torch.equal(tr.inference_net()(x), net(x))
    # a batch the Linear kernels cannot take, and a size depth_fc_1 is not made for
    with pytest.raises(ValueError):
        tr.forward(torch.zeros((65, 32, 32, 24), device=dev))
    with pytest.raises(ValueError):
        tr.forward(torch.zeros((2, 40, 40, 24), device=dev))


# ------------------------------------------------------------------------------------------------- the command line
@pytest.fixture
def work_dir():
    """a scratch directory whose PATH does not contain "test" (the loader keys on it)"""
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="mmh_hp3_")
    assert "test" not in d
    yield d
    shutil.rmtree(d, ignore_errors=True)


def test_train_hpe_hpm3d_writes_a_checkpoint_that_evaluate_scores(dev, work_dir, monkeypatch):
    from mmhand_amd import data, evaluate, hpe, hpe_train, train_hpe
    from tests._dataset_fixture import write_rhd
    root, extra, val = (os.path.join(work_dir, n) for n in ("rhd", "novel", "val"))
    write_rhd(root, n=7, size=32)
    write_rhd(extra, n=3, size=32, seed=9)
    write_rhd(val, n=4, size=32, seed=10)
    monkeypatch.chdir(work_dir)
    monkeypatch.setattr(train_hpe, "INIT_WIDTHS", O.NARROW)
    seen, reads = [], []
    step, read = hpe_train.Hpm3dTrainer.step, data._read_bgr

    def spy(self, x, depth, lr=None):
        seen.append((tuple(x.shape), torch.is_tensor(x), lr, np.array(depth)))
        return step(self, x, depth, lr)

    def read_spy(path):
        reads.append(path)
        return read(path)

    monkeypatch.setattr(hpe_train.Hpm3dTrainer, "step", spy)
    monkeypatch.setattr(data, "_read_bgr", read_spy)
    common = ["--extra_dataroot", extra, "--dataset", "rhd", "--net", "hpm3d", "--niter", "1", "--niter_decay", "1", "--batchSize", "4",
              "--lr", "2e-4", "--beta1", "0.5", "--save_epoch_freq", "2", "--threads", "2", "--dataroot", root]
    # the reference's recipe: maps rendered from the labels, no image file read
    log = train_hpe.main(common + ["--name", "t", "--init_seed", "3"])
    assert reads == []
    assert [s[0] for s in seen] == [(4, 21, 2), (4, 21, 2), (2, 21, 2)] * 2 and not any(s[1] for s in seen)
    assert [s[2] for s in seen] == [2e-4] * 3 + [pytest.approx(1e-4)] * 3
    assert all(100 <= s[3].min() and s[3].max() <= 690 for s in seen)       # rhd: the target is the label's depth itself
    assert len(log) == 2 and log[0]["images"] == 10 and np.isfinite([r["loss"] for r in log]).all()
    ckpt = os.path.join("checkpoints", "t")
    assert sorted(os.listdir(ckpt)) == ["2_net_Hpm3d.pth", "latest_net_Hpm3d.pth", "train_hpe_log.json"]
    sd = torch.load(os.path.join(ckpt, "latest_net_Hpm3d.pth"), map_location="cpu")
    start = hpe_train.init_state_dict_3d(3, O.NARROW, 4)
    assert O.keys_and_shapes(sd) == O.keys_and_shapes(start) and not torch.equal(sd["depth_fc_3.weight"], start["depth_fc_3.weight"])
    assert torch.equal(sd["stage6.conv3.weight"], start["stage6.conv3.weight"])
    # the distribution evaluate hands the network: the 2D machine's maps; validation with the evaluator's 3D figures
    h2 = os.path.join(work_dir, "h2.pth")
    torch.save(hpe_train.init_state_dict(5, {k: v for k, v in O.NARROW.items() if k != "fc"}), h2)
    seen.clear()
    log = train_hpe.main(common + ["--name", "p", "--init_from", os.path.join(ckpt, "latest_net_Hpm3d.pth"), "--heat_source",
                                   "predicted", "--hpm2d", h2, "--val_dataroot", val])
    assert [s[0] for s in seen] == [(4, 32, 32, 24), (4, 32, 32, 24), (2, 32, 32, 24)] * 2 and all(s[1] for s in seen)
    assert len(reads) == 2 * (10 + 2 * 4)                                   # per epoch: the training images, the validation twice
    assert 0.0 <= log[1]["pck3d_auc"] <= 1.0 and log[1]["epe3d_mean"] >= 0.0 and np.isfinite(log[1]["val_L_z"])
    latest = os.path.join("checkpoints", "p", "latest_net_Hpm3d.pth")
    hpe.Hpm3d(dev).load_state_dict(torch.load(latest, map_location="cpu"))
    res = evaluate.main(["--pck_images", val, "--dataset", "rhd", "--hpm2d", h2, "--hpm3d", latest, "--batchSize", "4",
                         "--results_json", "v.json"])
    assert res["summary"]["n"] == 4 and res["summary"]["pck3d_auc"] == log[1]["pck3d_auc"]
    assert json.load(open("v.json"))["summary"]["epe3d_mean"] == log[1]["epe3d_mean"]
    # the default net is unchanged
    monkeypatch.setattr(train_hpe, "INIT_WIDTHS", {k: v for k, v in O.NARROW.items() if k != "fc"})
    log = train_hpe.main(["--dataroot", root, "--dataset", "rhd", "--name", "d", "--niter", "1", "--niter_decay", "0", "--batchSize", "4",
                          "--init_seed", "3", "--threads", "2"])
    assert len(log) == 1 and len(log[0]["loss"]) == 6
    assert sorted(os.listdir(os.path.join("checkpoints", "d"))) == ["latest_net_Hpm2d.pth", "train_hpe_log.json"]
