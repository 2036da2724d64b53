"""PCK evaluation on the device (csrc/hpe.hip through mmhand_amd/ops.py, mmhand_amd/hpe.py and mmhand_amd/evaluate.py) against
tests/_hpe_oracle.py: the three new passes bit for bit, the two estimators against the float64 forward of the same graph, and
`evaluate --pck` end to end.  All weights are generated (tests/_hpe_oracle.state_dict): no figure here says anything about a
trained estimator."""
import csv
import json
import os
import pickle
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import _hpe_oracle as O

pytestmark = pytest.mark.gpu
SEED = 0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------- normalise
def _norm_images(H, W_, kind):
    """[4,3,H,W]: the largest value in the last pixel of the last channel; the smallest there; a constant image; the
    extremes in the first pixel - as fp32 in [-1, 1) or as bytes"""
    x = O.hashed(31, 4 * 3 * H * W_, SEED).reshape(4, 3, H, W_) * 0.9
    x[0, 2, H - 1, W_ - 1], x[1, 2, H - 1, W_ - 1], x[2], x[3, 0, 0, 0] = 0.99, -0.99, 0.25, 0.95
    if kind == "u8":
        return np.clip(np.round((x + 1) * 127.5), 0, 255).astype(np.uint8)
    return x.astype(np.float32)


# 136 x 128 = 17408 pixels: beyond 64 chunks of 256, where a thread of the min-max pass strides over several pixels
@pytest.mark.parametrize("H,W_", [(8, 8), (5, 7), (40, 50), (136, 128)])
@pytest.mark.parametrize("kind", ["u8", "f32", "f32_nhwc_view", "bf16"])
def test_normalize_is_bit_identical(dev, H, W_, kind):
    from mmhand_amd import ops
    img = _norm_images(H, W_, "u8" if kind == "u8" else "f32")
    if kind == "u8":
        t = torch.from_numpy(np.ascontiguousarray(img.transpose(0, 2, 3, 1)[..., ::-1])).to(dev)       # B,G,R pixels
        got = ops.hpe_normalize(t, "bgr_hwc")
    elif kind == "f32_nhwc_view":
        buf = torch.zeros((4, H, W_, 4), device=dev)
        buf[..., :3] = torch.from_numpy(img).to(dev).permute(0, 2, 3, 1)
        got = ops.hpe_normalize(ops.nhwc_to_nchw_view(buf, 3))
    elif kind == "bf16":
        t = torch.from_numpy(img).to(dev).to(torch.bfloat16)
        img = t.float().cpu().numpy()
        got = ops.hpe_normalize(t)
    else:
        got = ops.hpe_normalize(torch.from_numpy(img).to(dev))
    want = O.normalize(img)
    assert got.shape == (4, H, W_, 4) and np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    assert not want[2].any() and want[0, H - 1, W_ - 1, 2] == 1.0 and want[1, H - 1, W_ - 1, 2] == 0.0


# ------------------------------------------------------------------------------------------------- upsample + arg-max
def _heat(h, w, cs):
    """[2,h,w,cs]: joint 0 peaks at the first pixel, 1 at the last, 2 is negative everywhere, 3 is a plateau (every pixel
    equal: the first one must win), 4 has two equal peaks in opposite corners, 5 is -inf free but tiny; the rest noise"""
    v = (O.hashed(41, 2 * h * w * cs, SEED).reshape(2, h, w, cs) * 0.5).astype(np.float32)
    v[:, 0, 0, 0] = 10.0
    v[:, h - 1, w - 1, 1] = 10.0
    v[..., 2] = -np.abs(v[..., 2]) - 0.125
    v[..., 3] = 1.0
    v[:, 0, w - 1, 4] = v[:, h - 1, 0, 4] = 7.0
    v[..., 5] *= 1e-30
    return v


@pytest.mark.parametrize("h,w,cs", [(4, 4, 24), (5, 3, 152), (32, 32, 24), (3, 5, 21)])
def test_upsample_argmax_is_bit_identical(dev, h, w, cs):
    from mmhand_amd import ops
    heat = _heat(h, w, cs)
    up, xy, peak = ops.heatmap_upsample_argmax(torch.from_numpy(heat).to(dev))
    wup, wxy, wpeak = O.upsample_argmax(heat)
    assert np.array_equal(_bits(up.cpu().numpy()), _bits(wup))
    assert np.array_equal(xy.cpu().numpy(), wxy), (xy.cpu().numpy()[0, :6], wxy[0, :6])
    assert np.array_equal(_bits(peak.cpu().numpy()), _bits(wpeak))
    assert (wxy[:, 0] == [0, 0]).all() and (wxy[:, 1] == [8 * w - 1, 8 * h - 1]).all() and (wpeak[:, 2] < 0).all()
    assert (wxy[:, 3] == [0, 0]).all() and (wxy[:, 4, 1] == 0).all()        # ties: the first pixel in scan order


# ------------------------------------------------------------------------------------------------- linear
@pytest.mark.parametrize("M,K,N", [(1, 336, 512), (2, 24576, 512), (64, 512, 24)])
def test_linear_is_exact_and_grid_independent(dev, M, K, N):
    from mmhand_amd import lib, ops
    # integers: |x| <= 2, |w| <= 3, |b| <= 8 -> every partial sum is below 24576 * 6 + 8 < 2^24, exact in fp32 in any order
    x = np.floor(O.hashed(51, M * K, SEED) * 2.5).reshape(M, K)
    w = np.floor(O.hashed(52, K * N, SEED) * 3.5).reshape(K, N)
    b = np.floor(O.hashed(53, N, SEED) * 8.5)
    want = x.astype(np.int64) @ w.astype(np.int64) + b.astype(np.int64)
    assert np.abs(want).max() < 2 ** 24 and np.abs(want).max() > 50
    xt, wt, bt = (torch.from_numpy(a.astype(np.float32)).to(dev) for a in (x, w, b))
    chunks = lib.load().mmh_linear_chunks(K)
    assert chunks == -(-K // 256)
    for splits in (0, 1, 3):
        got = ops.linear(xt, wt, bt, splits=splits).cpu().numpy()
        assert got.shape == (M, N) and np.array_equal(got.astype(np.int64), want), splits
    assert np.array_equal(ops.linear(xt, wt, None).cpu().numpy().astype(np.int64), want - b.astype(np.int64))
    # real values: the sum is defined by the chunks, not by the grid - every split count gives the same bits
    xr = torch.from_numpy(O.hashed(54, M * K, SEED).reshape(M, K).astype(np.float32)).to(dev)
    wr = torch.from_numpy(O.hashed(55, K * N, SEED).reshape(K, N).astype(np.float32)).to(dev)
    ref = ops.linear(xr, wr, bt, splits=0).cpu().numpy()
    for splits in (1, 2, 5, chunks):
        assert np.array_equal(_bits(ops.linear(xr, wr, bt, splits=splits).cpu().numpy()), _bits(ref)), splits
    want_r = xr.double().cpu().numpy() @ wr.double().cpu().numpy() + b
    assert np.abs(ref - want_r).max() <= 1e-5 * np.sqrt(K) * max(1.0, np.abs(want_r).max())


# ------------------------------------------------------------------------------------------------- the two networks
@pytest.fixture(scope="module")
def nets(dev):
    """both estimators at full width on 32 x 32, B = 2, on the device and in the oracle (float64 and PyTorch's fp32 on the
    CPU), computed once and left alone"""
    from mmhand_amd import hpe, ops
    sd2, sd3 = O.state_dict("2d", O.FULL, seed=SEED), O.state_dict("3d", O.FULL, head_hw=4, seed=SEED)
    img = O.images(2, 32, 32, SEED)
    xn = ops.hpe_normalize(torch.from_numpy(img).to(dev))
    assert np.array_equal(_bits(xn.cpu().numpy()), _bits(O.normalize(img)))
    net2 = hpe.Hpm2d(dev).load_state_dict(OrderedDict((k, v.float()) for k, v in sd2.items()))
    net3 = hpe.Hpm3d(dev).load_state_dict(OrderedDict((k, v.float()) for k, v in sd3.items()))
    cat = net2(xn)
    up, xy, _ = ops.heatmap_upsample_argmax(cat)
    z = net3(up)
    x64 = xn[..., :3].permute(0, 3, 1, 2).double().cpu()
    u64 = up[..., :21].permute(0, 3, 1, 2).double().cpu()
    # a checkpoint is fp32: the oracle reads the weights the device got
    sd2 = OrderedDict((k, v.float().double()) for k, v in sd2.items())
    sd3 = OrderedDict((k, v.float().double()) for k, v in sd3.items())
    return dict(cat=cat.cpu().numpy(), up=up.cpu().numpy(), xy=xy.cpu().numpy(), z=z.cpu().numpy(),
                heat64=O.forward_2d(sd2, x64).numpy(), heat32=O.forward_2d(sd2, x64.float()).double().numpy(),
                z64=O.forward_3d(sd3, u64).numpy(), z32=O.forward_3d(sd3, u64.float()).double().numpy())


def test_estimators_stay_within_twice_pytorch_fp32(nets):
    """relative L1 against the float64 forward of the same graph on the same inputs: at most twice what PyTorch's fp32 CPU
    forward keeps (the factor allows for another summation order and nothing else)"""
    heat = nets["cat"][..., :21].transpose(0, 3, 1, 2)
    got2, ref2 = O.rel_l1(heat, nets["heat64"]), O.rel_l1(nets["heat32"], nets["heat64"])
    got3, ref3 = O.rel_l1(nets["z"][:, :21], nets["z64"]), O.rel_l1(nets["z32"], nets["z64"])
    print("Hpm2d heat maps: device %.3e, PyTorch fp32 %.3e, ratio %.2f" % (got2, ref2, got2 / ref2))
    print("Hpm3d depths:    device %.3e, PyTorch fp32 %.3e, ratio %.2f" % (got3, ref3, got3 / ref3))
    assert not nets["cat"][..., 21:24].any() and not nets["z"][:, 21:].any()
    assert got2 <= 2.0 * ref2, (got2, ref2)
    assert got3 <= 2.0 * ref3, (got3, ref3)


def test_predicted_pixels_equal_the_oracles(nets):
    """every joint whose two best pixels are further apart in the oracle than ten times the fp32 distance of the heat maps
    (PyTorch's relative L1 x the maps' mean size: the distance as a size on the maps) gets the oracle's pixel; at most 2 of
    the 42 joints may be closer than that (tests/test_hpe_cpu.py asserts it for this seed)"""
    h64 = nets["heat64"].transpose(0, 2, 3, 1)
    dist = O.rel_l1(nets["heat32"], nets["heat64"]) * np.abs(nets["heat64"]).mean()
    up64 = O.upsample(h64)
    gap = O.top_two_gap(up64)
    flat = up64.reshape(2, -1, 21).argmax(1)
    want = np.stack([flat % up64.shape[2], flat // up64.shape[2]], -1)
    clear = gap > 10 * dist
    assert (~clear).sum() <= 2
    assert np.array_equal(nets["xy"][clear], want[clear]), (nets["xy"][clear], want[clear])
    # and the kernel's own pass agrees with the oracle's pass on the device's maps, bit for bit
    wup, wxy, _ = O.upsample_argmax(nets["cat"])
    assert np.array_equal(_bits(nets["up"]), _bits(wup)) and np.array_equal(nets["xy"], wxy)


def test_forward_does_not_depend_on_the_winograd_mode(dev, nets):
    from mmhand_amd import hpe, lib, ops
    sd2 = O.state_dict("2d", O.NARROW, seed=SEED, dtype=torch.float32)
    net = hpe.Hpm2d(dev).load_state_dict(sd2)
    x = ops.hpe_normalize(torch.from_numpy(O.images(2, 16, 16, SEED)).to(dev))
    a = net(x).cpu().numpy()
    before = lib.get_option("conv_levels")
    try:
        for mode in ("off", "all"):
            ops.set_winograd_mode(mode)
            assert np.array_equal(_bits(net(x).cpu().numpy()), _bits(a)), mode
            assert lib.get_option("conv_levels") == (2 if mode == "off" else 1)      # put back after the call
    finally:
        ops.set_winograd_mode("all")
        lib.call("mmh_set_option", b"conv_levels", before)


def test_hpm3d_takes_more_rows_than_one_linear_launch(dev):
    """mmh_linear_fprop takes at most 64 rows: a larger batch goes through it in pieces"""
    from mmhand_amd import hpe
    sd3 = O.state_dict("3d", O.NARROW, head_hw=2, seed=SEED, dtype=torch.float32)
    net = hpe.Hpm3d(dev).load_state_dict(sd3)
    up = torch.zeros((66, 16, 16, 24), device=dev)
    up[..., :21] = torch.from_numpy(O.hashed(61, 66 * 16 * 16 * 21, SEED).reshape(66, 16, 16, 21).astype(np.float32)).to(dev)
    z = net(up).cpu().numpy()
    want = O.forward_3d(sd3, up[..., :21].permute(0, 3, 1, 2).double().cpu()).numpy()
    assert z.shape == (66, 24) and not z[:, 21:].any()
    assert np.abs(z[:, :21] - want).max() <= 1e-5 * np.abs(want).max()


# ------------------------------------------------------------------------------------------------- evaluate --pck
@pytest.fixture
def work_dir():
    """a scratch directory whose PATH does not contain "test" (the loader keys on it)"""
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="mmh_pck_")
    assert "test" not in d
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _oracle_scores(fed, sd2, sd3, z_scale=256.0):
    """the oracle pipeline on the batches the estimator was fed: float64 networks, the oracle's passes, EvalUtil's distances.
    Also, from the oracle alone, the joints that are exempt from the pixel comparison: those whose two best pixels are no
    further apart in the float64 maps than ten times the distance PyTorch's fp32 forward keeps from them (relative L1 x the
    maps' mean size, as in test_predicted_pixels_equal_the_oracles)"""
    d2, d3, xys, exempt = [], [], [], []
    for img, layout, uv, depth, _ in fed:
        if layout == "bgr_hwc":
            img = np.ascontiguousarray(img[..., ::-1].transpose(0, 3, 1, 2))
        xn = O.normalize(img)
        x64 = torch.from_numpy(xn[..., :3]).permute(0, 3, 1, 2).double()
        heat = O.forward_2d(sd2, x64)
        dist = O.rel_l1(O.forward_2d(sd2, x64.float()).double().numpy(), heat.numpy()) * float(heat.abs().mean())
        exempt.append(O.top_two_gap(O.upsample(heat.permute(0, 2, 3, 1).numpy())) <= 10 * dist)
        up, xy, _ = O.upsample_argmax(heat.permute(0, 2, 3, 1).float().numpy())
        z = O.forward_3d(sd3, torch.from_numpy(up[..., :21]).permute(0, 3, 1, 2).double()).numpy()
        a, b = O.distances(uv, xy, depth, z, height=img.shape[2], z_scale=z_scale)
        d2.append(a)
        d3.append(b)
        xys.append(xy)
    return np.concatenate(d2), np.concatenate(d3), np.concatenate(xys), np.concatenate(exempt)


def test_evaluate_pck_in_three_modes(dev, work_dir, monkeypatch):
    from PIL import Image
    from mmhand_amd import evaluate, hpe
    from mmhand_amd.networks import Generator
    from tests._dataset_fixture import write_rhd
    root = os.path.join(work_dir, "rhd")
    write_rhd(root, n=6, size=32)
    monkeypatch.chdir(work_dir)
    sd2 = O.state_dict("2d", O.NARROW, seed=SEED, dtype=torch.float32)
    sd3 = O.state_dict("3d", O.NARROW, head_hw=4, seed=SEED, dtype=torch.float32)
    torch.save(OrderedDict(("module." + k, v) for k, v in sd2.items()), "hpm2d.pth")
    torch.save(sd3, "hpm3d.pth")
    sd2 = OrderedDict((k, v.double()) for k, v in sd2.items())
    sd3 = OrderedDict((k, v.double()) for k, v in sd3.items())
    os.makedirs(os.path.join("checkpoints", "ev"))
    torch.manual_seed(5)
    torch.save(Generator([3, 42, 6], 3, 8, "instance", False, 2).state_dict(), os.path.join("checkpoints", "ev", "latest_net_netG.pth"))

    fed = []
    feed = hpe.HPEstimator.feed

    def spy(self, images, uv, depth=None, paths=None, layout="nchw"):
        feed(self, images, uv, depth, paths, layout)
        fed.append((images.detach().float().cpu().numpy() if layout == "nchw" else images.cpu().numpy(), layout,
                    np.array(uv), np.array(depth), self._batches[-1][0].cpu().numpy()))

    monkeypatch.setattr(hpe.HPEstimator, "feed", spy)
    pck = ["--pck", "--hpm2d", "hpm2d.pth", "--hpm3d", "hpm3d.pth"]

    def check(res, js, n):
        d2, d3, xy, exempt = _oracle_scores(fed, sd2, sd3)
        assert d2.shape == (n, 21) and js["summary"]["n"] == n
        rows = res["rows"]
        # the exemption is the oracle's alone and capped at the issue's share, 2 of 42 joints; every other joint must sit on
        # the oracle's pixel.  An exempt joint moves an AUC by at most 1 / (21 n), its share of the curves' mean, and a mean
        # distance by at most 64 / (21 n); with no exempt joint the 2D figures are equal
        n_exempt = int(exempt.sum())
        assert n_exempt <= 2 * (21 * n) // 42, (n_exempt, n)
        off = (np.concatenate([f[4] for f in fed]) != xy).any(2)
        print("exempt joints:", n_exempt, "of", 21 * n, "- off the oracle's pixel:", int(off.sum()))
        assert not (off & ~exempt).any(), np.argwhere(off & ~exempt)
        moved = n_exempt
        share = n_exempt / (21.0 * n) + 1e-12
        s = js["summary"]
        for tag, d in (("2d", d2), ("3d", d3)):
            mean, median, auc, curve, thr = O.measures(d, 30, 20)
            assert abs(s[f"pck{tag}_auc"] - auc) <= share, (tag, s[f"pck{tag}_auc"], auc)
            assert np.abs(np.array(s[f"pck{tag}_curve"]) - curve).max() <= share and len(s[f"pck{tag}_curve"]) == 20
            # the 3D distances carry the fp32 depths: 1e-4 of the image height
            tol = 1e-9 + (1e-4 * 32 if tag == "3d" else 0.0) + moved * 64.0 / (21 * n)
            assert abs(s[f"epe{tag}_mean"] - mean) <= tol, (tag, s[f"epe{tag}_mean"], mean)
        assert np.allclose(s["pck_thresholds"], np.linspace(0, 30, 20))
        if not moved:
            assert np.abs(np.array([r["epe2d"] for r in rows]) - d2.mean(1)).max() <= 1e-9
            assert np.abs(np.array([r["epe3d"] for r in rows]) - d3.mean(1)).max() <= 1e-4 * 32

    # 1. a prepared directory against its own labels
    res = evaluate.main(["--pck_images", root, "--dataset", "rhd", "--batchSize", "4", "--results_json", "p.json",
                         "--per_image_csv", "p.csv"] + pck[1:])
    js = json.load(open("p.json"))
    check(res, js, 6)
    assert [r["target"] for r in res["rows"]] == sorted((r["target"] for r in res["rows"]), key=lambda p: int(os.path.basename(p)[:-4]))
    with open(os.path.join(root, "annotation.pickle"), "rb") as fh:
        ann = pickle.load(fh)
    first = res["rows"][0]["target"]
    assert np.array_equal(fed[0][2][0], np.asarray(ann["color"][os.path.basename(first)]["uv_coord"]))
    assert np.array_equal(fed[0][0][0], np.array(Image.open(first).convert("RGB"))[..., ::-1])
    table = list(csv.reader(open("p.csv")))
    assert table[0] == ["target", "epe2d", "epe3d"] and len(table) == 7
    # only --hpm2d: the 2D figures alone
    fed.clear()
    evaluate.main(["--pck_images", root, "--dataset", "rhd", "--hpm2d", "hpm2d.pth", "--results_json", "q.json"])
    q = json.load(open("q.json"))["summary"]
    assert q["pck2d_auc"] == js["summary"]["pck2d_auc"] and not any(k.startswith(("pck3d", "epe3d")) for k in q)

    # 2. a generator checkpoint: the fake batch goes to the estimator as it lies on the device
    base = ["--name", "ev", "--dataroot", root, "--dataset", "rhd", "--augmentation_ratio", "0.5", "--batchSize", "2"]
    fed.clear()
    random.seed(11)
    res = evaluate.main(base + pck + ["--results_json", "g.json", "--per_image_csv", "g.csv"])
    js = json.load(open("g.json"))
    check(res, js, 3)
    assert {"SSIM_avg", "pck2d_auc", "pck3d_auc", "epe2d_mean", "epe2d_median", "epe3d_mean", "epe3d_median"} <= set(js["summary"])
    assert js["options"]["hpm2d"] == "hpm2d.pth" and fed[0][1] == "nchw"
    assert list(csv.reader(open("g.csv")))[0] == ["target", "source", "ssim", "l1", "psnr", "epe2d", "epe3d"]
    for (uv, depth), r in zip([(u, d) for f in fed for u, d in zip(f[2], f[3])], res["rows"]):
        lab = ann["color"][os.path.basename(r["target"])]           # the TARGET pose's labels
        assert np.array_equal(uv, np.asarray(lab["uv_coord"])) and np.array_equal(depth, np.asarray(lab["depth"]))
    # without --pck the files are what they were: no new key anywhere
    fed.clear()
    random.seed(11)
    plain = evaluate.main(base + ["--results_json", "n.json", "--per_image_csv", "n.csv"])
    n = json.load(open("n.json"))
    assert not fed and set(n["summary"]) == {"SSIM_avg", "SSIM_std", "L1_avg", "PSNR_avg", "n"}
    assert not set(n["options"]) & set(evaluate.PCK_FLAGS)
    assert list(csv.reader(open("n.csv")))[0] == ["target", "source", "ssim", "l1", "psnr"]
    assert [r["ssim"] for r in plain["rows"]] == [r["ssim"] for r in res["rows"]]

    # 3. a directory of generated PNGs
    for r in res["rows"]:
        os.makedirs(os.path.join("gen", "color"), exist_ok=True)
        rs = np.random.RandomState(len(r["target"]))
        Image.fromarray(rs.randint(0, 256, size=(32, 32, 3), dtype=np.uint8)).save(os.path.join("gen", "color", os.path.basename(r["target"])))
    fed.clear()
    random.seed(11)
    res = evaluate.main(["--generated", "gen", "--dataroot", root, "--dataset", "rhd", "--augmentation_ratio", "0.5",
                         "--batchSize", "3", "--results_json", "d.json"] + pck)
    check(res, json.load(open("d.json")), 3)
    assert fed[0][1] == "bgr_hwc"
