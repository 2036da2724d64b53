"""The PCK feature's host side: the test oracle (tests/_hpe_oracle.py) against the outputs recorded from the reference's own
estimator code (tests/golden/hpe.npz, hpe_keys.json; tests/golden/make_hpe.py), the checkpoint re-layout of mmhand_amd/hpe.py,
and the host PCK arithmetic.  No GPU."""
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _hpe_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "hpe.npz"))


@pytest.fixture(scope="module")
def full():
    """the oracle's float64 run on the fixture's inputs, once"""
    x = torch.from_numpy(O.normalize(O.images(2, 32, 32, SEED))[..., :3]).permute(0, 3, 1, 2).double()
    heat = O.forward_2d(O.state_dict("2d", O.FULL, seed=SEED), x).numpy()
    return x, heat


def test_generated_weights_are_a_pure_function_of_the_counters():
    a = O.hashed(3, 1000, SEED)
    assert np.array_equal(a, O.hashed(3, 1000, SEED)) and np.array_equal(a[:10], O.hashed(3, 10, SEED))
    assert not np.array_equal(a, O.hashed(4, 1000, SEED)) and not np.array_equal(a, O.hashed(3, 1000, SEED + 1))
    assert -1.0 <= a.min() < -0.9 and 0.9 < a.max() < 1.0 and abs(a.mean()) < 0.1
    # pinned: the same bits on any machine
    assert [v.hex() for v in a[:3].tolist()] == ["-0x1.1a99c39682b1ap-1", "-0x1.8ef622666dac4p-2", "0x1.1f34870611ea4p-2"]
    assert [v.hex() for v in O.hashed(0, 2, 7).tolist()] == ["-0x1.7d00592746404p-2", "-0x1.f8c773c2835aep-1"]
    bits = (O.hashed(0, 4, 0) + 1.0) * float(1 << 52)
    assert np.array_equal(bits, np.floor(bits))


def test_state_dict_keys_and_shapes_are_the_references():
    with open(os.path.join(ROOT, "tests", "golden", "hpe_keys.json")) as fh:
        keys = json.load(fh)
    assert O.keys_and_shapes(O.state_dict("2d", O.FULL, seed=SEED)) == keys["hpm2d"]
    assert O.keys_and_shapes(O.state_dict("3d", O.FULL, head_hw=32, seed=SEED)) == keys["hpm3d"]


def test_oracle_matches_the_reference_networks(gold, full):
    _, heat = full
    assert O.rel_l1(heat, gold["heat"]) < 1e-12
    up, xy, _ = O.upsample_argmax(np.ascontiguousarray(gold["heat"].transpose(0, 2, 3, 1)).astype(np.float32))
    # the fixture's maps are float64; the oracle's upsample of them agrees with the reference's to round-off
    up64 = O.upsample(gold["heat"].transpose(0, 2, 3, 1))
    assert np.abs(up64.transpose(0, 3, 1, 2) - gold["up"]).max() < 1e-13 * np.abs(gold["up"]).max()
    assert np.array_equal(xy, gold["xy"])       # y = index // H, x = index % W: the same pixel on a square map
    depth = O.forward_3d(O.state_dict("3d", O.FULL, head_hw=4, seed=SEED), torch.from_numpy(gold["up"])).numpy()
    assert O.rel_l1(depth, gold["depth"]) < 1e-12


@pytest.mark.parametrize("h,w", [(4, 4), (5, 3), (1, 2)])
def test_upsample_oracle_is_bilinear_align_corners(h, w):
    v = O.hashed(11, 2 * h * w * 21, SEED).reshape(2, h, w, 21)
    want = F.interpolate(torch.from_numpy(v).permute(0, 3, 1, 2), scale_factor=8, mode="bilinear", align_corners=True)
    got = O.upsample(v).transpose(0, 3, 1, 2)
    assert np.abs(got - want.numpy()).max() < 1e-14
    up, xy, peak = O.upsample_argmax(v.astype(np.float32))
    assert up.shape == (2, 8 * h, 8 * w, 24) and not up[..., 21:].any()
    for b in range(2):
        for j in range(21):
            assert up[b, xy[b, j, 1], xy[b, j, 0], j] == peak[b, j] == up[b, :, :, j].max()


def test_normalize_oracle_is_its_formula():
    img = O.images(2, 5, 7, SEED)
    img[1] = 0.25
    out = O.normalize(img)
    mn, mx = float(img[0].min()), float(img[0].max())
    assert out[0, 2, 3, 1] == np.float32((float(img[0, 1, 2, 3]) - mn) / (mx - mn))
    assert out[0, :, :, :3].min() == 0.0 and out[0, :, :, :3].max() == 1.0 and not out[..., 3].any() and not out[1].any()


def _nhwc(x, lanes):
    out = torch.zeros((x.shape[0], x.shape[2], x.shape[3], lanes), dtype=x.dtype)
    out[..., :x.shape[1]] = x.permute(0, 2, 3, 1)
    return out


def _relaid_forward(net, x):
    """the re-laid weights of a mmhand_amd.hpe network run through the buffers its forward uses, with F.conv2d in float64
    on the host: x NHWC [B,H,W,lanes] -> (cat buffer, depths or None)"""
    from mmhand_amd import hpe

    def conv(name, t, relu=True):
        w, b = net.convs[name]
        y = F.conv2d(t.permute(0, 3, 1, 2), w.double().permute(3, 2, 0, 1), b.double(), padding=w.shape[0] // 2)
        return (F.relu(y) if relu else y).permute(0, 2, 3, 1)

    for n in hpe.TRUNK:
        x = F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) if n == "pool" else conv(n, x)
    cat = torch.full(tuple(x.shape[:3]) + (net.cat,), float("nan"), dtype=torch.float64)
    cat[..., hpe.JLANES:] = conv("conv5_3_CPM", x)
    cat[..., :hpe.JLANES] = conv("conv6_2_CPM", conv("conv6_1_CPM", cat[..., hpe.JLANES:]), relu=False)

    def repeat(s):
        t = cat
        for c in hpe.REPEAT[:-1]:
            t = conv(f"{s}.{c}", t)
        return conv(f"{s}.conv7", t, relu=False)

    for s in net.STAGES:
        if s == "depth":
            z = repeat(s).reshape(x.shape[0], -1)
            for wt, b in net.fc:
                z = z @ wt.double() + b.double()
            return cat, z
        cat[..., :hpe.JLANES] = repeat(s)
    return cat, None


@pytest.mark.parametrize("prefix", ["", "module."])
def test_checkpoint_relayout_round_trips(prefix):
    from mmhand_amd import hpe
    sd2 = O.state_dict("2d", O.NARROW, seed=SEED)
    sd3 = O.state_dict("3d", O.NARROW, head_hw=2, seed=SEED)
    x = torch.from_numpy(O.normalize(O.images(2, 16, 16, SEED))[..., :3]).permute(0, 3, 1, 2).double()
    want_heat = O.forward_2d(sd2, x)
    net2 = hpe.Hpm2d("cpu").load_state_dict(OrderedDict((prefix + k, v.float()) for k, v in sd2.items()))
    assert net2.c0 == 8 and net2.cat == 32 and net2.in_nc == 3
    w1 = net2.convs["stage2.conv1"][0]
    assert tuple(w1.shape) == (7, 7, 32, 8) and not w1[:, :, 21:24].any() and w1[:, :, :21].any() and w1[:, :, 24:].any()
    assert tuple(net2.convs["conv6_2_CPM"][0].shape) == (1, 1, 16, 24) and not net2.convs["conv6_2_CPM"][0][..., 21:].any()
    assert not net2.convs["conv6_2_CPM"][1][21:].any()
    cat, _ = _relaid_forward(net2, _nhwc(x, 4))
    # the weights went through fp32 on the way (a checkpoint is fp32): 1e-6, not 1e-12
    assert O.rel_l1(cat[..., :21].permute(0, 3, 1, 2).numpy(), want_heat.numpy()) < 1e-5
    assert not cat[..., 21:24].any() and not torch.isnan(cat).any()

    up = torch.from_numpy(O.upsample(cat[..., :21].numpy())).permute(0, 3, 1, 2)
    want_z = O.forward_3d(sd3, up)
    net3 = hpe.Hpm3d("cpu").load_state_dict(OrderedDict((prefix + k, v.float()) for k, v in sd3.items()))
    assert net3.head_hw == 2 and net3.in_nc == 21 and tuple(net3.fc[0][0].shape) == (2 * 2 * 24, 16)
    assert tuple(net3.fc[2][0].shape) == (16, 24) and not net3.fc[2][0][:, 21:].any()
    _, z = _relaid_forward(net3, _nhwc(up, 24))
    assert O.rel_l1(z[:, :21].numpy(), want_z.numpy()) < 1e-5 and not z[:, 21:].any()


def test_checkpoint_errors():
    from mmhand_amd import hpe
    sd = O.state_dict("2d", O.NARROW, seed=SEED)
    with pytest.raises(KeyError):
        hpe.Hpm3d("cpu").load_state_dict(sd)            # no depth.* / depth_fc_*
    del sd["stage4.conv3.bias"]
    with pytest.raises(KeyError):
        hpe.Hpm2d("cpu").load_state_dict(sd)


def test_pck_measures_equal_evalutil(gold):
    from mmhand_amd.hpe import pck_measures
    d2, _ = O.distances(gold["ev_gt"], gold["ev_pred"])
    for max_px, steps in ((30, 20), (10, 7)):
        rec = gold[f"ev_{max_px}_{steps}"]
        for got in (pck_measures(d2, max_px, steps), dict(zip(("epe_mean", "epe_median", "auc", "curve"),
                                                               O.measures(d2, max_px, steps)))):
            assert abs(got["epe_mean"] - rec[0]) < 1e-12 and abs(got["epe_median"] - rec[1]) < 1e-12
            assert abs(got["auc"] - rec[2]) < 1e-12 and np.abs(np.asarray(got["curve"]) - rec[3:]).max() < 1e-12
            assert len(got["curve"]) == steps


def test_argmax_condition_holds_for_the_seed(full):
    """what tests/test_hpe_gpu.py relies on: with these weights at most 2 of the 42 joints have a top-two gap in the oracle's
    upsampled maps within ten times the distance PyTorch's fp32 forward keeps from float64"""
    x, heat = full
    heat32 = O.forward_2d(O.state_dict("2d", O.FULL, seed=SEED), x.float()).double().numpy()
    dist = O.rel_l1(heat32, heat) * np.abs(heat).mean()            # the distance as an absolute size on the maps
    up = O.upsample(heat.transpose(0, 2, 3, 1))
    gap = O.top_two_gap(up)
    print("fp32 CPU rel-L1 %.2e, abs %.2e; smallest gaps %s" % (O.rel_l1(heat32, heat), dist, np.sort(gap.ravel())[:4]))
    assert (gap <= 10 * dist).sum() <= 2


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from mmhand_amd import lib as L
    lib = L.load()
    assert lib.mmh_linear_chunks(24576) == 96 and lib.mmh_linear_chunks(336) == 2 and lib.mmh_linear_chunks(0) == 0
    assert lib.mmh_linear_fprop_ws_bytes(2, 336, 512) == 2 * 2 * 512 * 4
    assert lib.mmh_linear_fprop_ws_bytes(65, 8, 8) == 0 and lib.mmh_linear_fprop_ws_bytes(1, 8, 6) == 0
    assert lib.mmh_hpe_normalize_ws_bytes(2, 5, 7) == 2 * 1 * 8 and lib.mmh_hpe_normalize_ws_bytes(0, 5, 7) == 0
    assert lib.mmh_heatmap_upsample_argmax_ws_bytes(2, 4, 4) == 2 * 4 * 21 * 8
    assert lib.mmh_heatmap_upsample_argmax_ws_bytes(1, 0, 4) == 0
    assert lib.mmh_linear_fprop(None, None, None, None, 1, 8, 8, 0, None, 0, None) != 0 and b"NULL" in lib.mmh_last_error()
    assert lib.mmh_hpe_normalize(None, 1, 8, 8, None, 0, None, None) != 0
    assert lib.mmh_heatmap_upsample_argmax(None, 1, 4, 4, 24, None, None, None, None, 0, None) != 0


def test_evaluate_flags_parse():
    from mmhand_amd.evaluate import build_parser
    a = build_parser().parse_args(["--pck_images", "D", "--dataset", "rhd", "--pck", "--hpm2d", "a.pth"])
    assert a.pck and a.pck_images == "D" and a.hpm3d is None and a.pck_max == 30 and a.pck_steps == 20
    a = build_parser().parse_args(["--name", "x", "--dataroot", "D", "--dataset", "rhd"])
    assert not a.pck and a.pck_images is None
