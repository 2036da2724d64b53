"""The Inception score on the device (csrc/inception.hip and mmh_conv2d_fprop_rect through mmhand_amd/ops.py,
mmhand_amd/inception.py and mmhand_amd/evaluate.py) against tests/_inception_oracle.py: the rectangular convolution and the
pools exactly on integers, the preprocess bit for bit against PIL's arithmetic plus the lookup table, the score within 1e-12 of
float64 numpy, the network against the float64 forward of the same graph, and `evaluate --inception` end to end.  All weights
are generated (tests/_inception_oracle.state_dict): no figure here says anything about real images."""
import csv
import json
import os
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _exact as E
from tests import _inception_oracle as O
from tests._hpe_oracle import hashed

pytestmark = pytest.mark.gpu
SEED = 0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -77.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module", autouse=True)
def _give_memory_back():
    """this module keeps four full Inception-v3 weight sets, batches of 66 and float64 work buffers alive for a while: when
    it ends (set up first, so torn down after the module's other fixtures) the cached blocks go back to the driver, and the
    modules after it start from the allocator they would have found without this one"""
    yield
    import gc
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------- rectangular convolution
RECT = [(1, 7, 0, 3), (7, 1, 3, 0), (1, 3, 0, 1), (3, 1, 1, 0)]


def _conv64(x, w, b, stride, pad, act):
    """float64 NHWC conv of integer tensors (x [B,H,W,Cin], w RSCK) with padding (pad_h, pad_w)"""
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(3, 2, 0, 1), b.double(), stride, pad)
    y = y.relu() if act else y
    assert float(y.abs().max()) <= E.CAP_F32 and float(y.abs().max()) >= 1
    return y.permute(0, 2, 3, 1).contiguous()


# 2 x 17 x 17 = 578 rows: more than one 128-row tile and a ragged last one; 5 x 4 and 2 x 1: images smaller than a kernel,
# where a 1x7 window hangs over both sides at once; 128 -> 192 and 768 -> 160: two-level and 256-free column tiles, 160 = 128 + 32;
# 4 -> 32: the flat k order of a 4-lane input
@pytest.mark.parametrize("kh,kw,ph,pw", RECT)
@pytest.mark.parametrize("H,W_", [(5, 4), (2, 1), (17, 17)])
@pytest.mark.parametrize("cin,cout", [(128, 192), (768, 160), (4, 32)])
def test_rect_conv_is_exact_into_a_lane_window(dev, kh, kw, ph, pw, H, W_, cin, cout):
    from mmhand_amd import lib, ops
    from mmhand_amd.hpe import direct_two_level
    x = E.ints((2, H, W_, cin), E.SEED_X)
    w = E.ints((kh, kw, cin, cout), E.SEED_W, E.W_DENSITY)
    b = E.ints((cout,), E.SEED_B, lo=-3, hi=3)
    want = _conv64(x, w, b, 1, (ph, pw), 1)
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    E.assert_exact(ops.conv_fprop_direct(xd, wd, bd, ph, pw, act=lib.ACT_RELU), want, "rect fprop")
    with direct_two_level():
        E.assert_exact(ops.conv_fprop_direct(xd, wd, bd, ph, pw, act=lib.ACT_RELU), want, "rect fprop, conv_levels 2")
    # read from lane 8 of a wider input, written at lane 12 of a wider output whose other lanes keep their sentinel
    xw = torch.full((2, H, W_, cin + 12), 5.0, device=dev)
    xw[..., 8:8 + cin] = xd
    out = torch.full((2, H, W_, cout + 20), SENTINEL, device=dev)
    got = ops.conv_fprop_direct(xw, wd, bd, ph, pw, act=lib.ACT_RELU, x_off=8, out=out, y_off=12)
    assert got is out
    E.assert_exact(out[..., 12:12 + cout], want, "rect fprop into a window")
    assert bool((out[..., :12] == SENTINEL).all()) and bool((out[..., 12 + cout:] == SENTINEL).all())


@pytest.mark.parametrize("k,pad,stride,H,W_,cin,cout", [(3, 1, 1, 9, 7, 96, 96), (5, 2, 1, 7, 7, 48, 64), (3, 0, 2, 11, 9, 288, 384),
                                                       (1, 0, 1, 5, 4, 768, 192)])
def test_rect_conv_with_equal_pads_has_the_bits_of_fprop(dev, k, pad, stride, H, W_, cin, cout):
    from mmhand_amd import lib, ops
    x = torch.from_numpy(hashed(71, 2 * H * W_ * cin, SEED).reshape(2, H, W_, cin).astype(np.float32)).to(dev)
    w = torch.from_numpy((hashed(72, k * k * cin * cout, SEED) * 0.1).reshape(k, k, cin, cout).astype(np.float32)).to(dev)
    b = torch.from_numpy(hashed(73, cout, SEED).astype(np.float32)).to(dev)
    a = ops.conv_fprop_direct(x, w, b, pad, pad, stride, lib.ACT_RELU, rect=True).cpu().numpy()
    c = ops.conv_fprop_direct(x, w, b, pad, pad, stride, lib.ACT_RELU, rect=False).cpu().numpy()
    assert a.shape == c.shape and np.array_equal(_bits(a), _bits(c)) and np.abs(a).max() > 0.1
    want = F.conv2d(x.double().cpu().permute(0, 3, 1, 2), w.double().cpu().permute(3, 2, 0, 1), b.double().cpu(), stride, pad).relu()
    assert np.abs(a - want.permute(0, 2, 3, 1).numpy()).max() <= 1e-5 * float(want.abs().max())


def test_rect_conv_refuses_what_it_cannot_do(dev):
    from mmhand_amd import lib, ops
    x, w = torch.zeros((1, 5, 4, 8), device=dev), torch.zeros((1, 7, 8, 8), device=dev)
    ops.conv_fprop_direct(x, w, None, 0, 3)
    d = lib.ConvDesc(1, 5, 4, 8, 8, 1, 7, 1, 0, lib.PAD_ZERO, 5, 5, 8, 8, lib.F32)          # Wo is 4 with pad_w 3
    import ctypes as C
    args = (ops._ptr(x), ops._ptr(w), None, ops._ptr(x), lib.ACT_NONE, ops._stream())
    assert lib.load().mmh_conv2d_fprop_rect(C.byref(d), 0, 3, *args) != 0 and b"Ho/Wo" in lib.load().mmh_last_error()
    d = lib.ConvDesc(1, 5, 4, 8, 8, 1, 7, 1, 0, lib.PAD_REFLECT, 5, 4, 8, 8, lib.F32)
    assert lib.load().mmh_conv2d_fprop_rect(C.byref(d), 0, 3, *args) != 0
    d = lib.ConvDesc(1, 5, 4, 8, 8, 1, 7, 1, 0, lib.PAD_ZERO, 5, 4, 8, 8, lib.BF16)
    assert lib.load().mmh_conv2d_fprop_rect(C.byref(d), 0, 3, *args) != 0


# ------------------------------------------------------------------------------------------------- preprocess
def _pre_images(H, W_, kind):
    """[2,3,H,W]: the oracle's images with the range's ends, values beyond it and exact rounding ties in the first pixels"""
    img = O.images(2, H, W_, SEED)
    img[0, :, 0, :6] = np.array([-1.0, 1.0, -1.5, 1.25, 1.0 / 255.0, -1.0 + 3.0 / 255.0], dtype=np.float32)     # the last one is a tie: 1.5 -> 2
    if kind == "u8":
        return O.to_bytes(img)
    return img


# up at 75, up to 299 from the paper's size, down (five taps), both non-square orientations (a crop window off the left / top)
@pytest.mark.parametrize("H,W_,size", [(64, 64, 75), (256, 256, 299), (512, 512, 299), (40, 50, 299), (50, 40, 299), (8, 8, 75)])
@pytest.mark.parametrize("kind", ["u8", "f32", "f32_nhwc_view", "bf16"])
def test_preprocess_is_bit_identical_to_pil_and_the_table(dev, H, W_, size, kind):
    from mmhand_amd import inception, ops
    img = _pre_images(H, W_, "u8" if kind == "u8" else "f32")
    tables = inception.PreprocessTables(H, W_, size, dev)
    if kind == "u8":
        t = torch.from_numpy(np.ascontiguousarray(img.transpose(0, 2, 3, 1)[..., ::-1])).to(dev)       # B,G,R pixels
        got, u8 = ops.inception_preprocess(t, "bgr_hwc", tables), img
    elif kind == "f32_nhwc_view":
        buf = torch.zeros((2, H, W_, 4), device=dev)
        buf[..., :3] = torch.from_numpy(img).to(dev).permute(0, 2, 3, 1)
        got, u8 = ops.inception_preprocess(ops.nhwc_to_nchw_view(buf, 3), "nchw", tables), O.to_bytes(img)
    elif kind == "bf16":
        t = torch.from_numpy(img).to(dev).to(torch.bfloat16)
        got, u8 = ops.inception_preprocess(t, "nchw", tables), O.to_bytes(t.float().cpu().numpy())
    else:
        got, u8 = ops.inception_preprocess(torch.from_numpy(img).to(dev), "nchw", tables), O.to_bytes(img)
    want = O.preprocess(np.ascontiguousarray(u8.transpose(0, 2, 3, 1)), size)
    got = got.cpu().numpy()
    assert got.shape == (2, size, size, 4) and not got[..., 3].any()
    assert np.array_equal(_bits(got), _bits(want))
    if (H, W_, size) == (40, 50, 299):      # once, against PIL itself: the oracle is the numpy model tests/test_inception_cpu.py pins
        from PIL import Image
        r = np.asarray(Image.fromarray(np.ascontiguousarray(u8[1].transpose(1, 2, 0))).resize((373, 299), Image.BILINEAR))[:, 37:336]
        assert np.array_equal(_bits(got[1, :, :, 0]), _bits(O.lut()[0][r[:, :, 0]]))


# ------------------------------------------------------------------------------------------------- pools
def _pool_input(B, H, W_, C, seed):
    return np.floor(hashed(seed, B * H * W_ * C, SEED).reshape(B, H, W_, C) * 9.0)        # integers -9 .. 8


@pytest.mark.parametrize("H,W_,C", [(7, 7, 64), (6, 5, 4), (3, 3, 288)])
def test_max_pool_is_exact(dev, H, W_, C):
    from mmhand_amd import ops
    x = _pool_input(2, H, W_, C, 81)
    x[:, :3, :3, 0] = -np.arange(1, 10).reshape(3, 3)              # an all-negative window: no zero may leak in
    want = O.max_pool(x)
    xd = torch.from_numpy(x.astype(np.float32)).to(dev)
    got = ops.pool3x3(xd, "max").cpu().numpy()
    assert got.shape == (2, (H - 3) // 2 + 1, (W_ - 3) // 2 + 1, C) and np.array_equal(got.astype(np.float64), want)
    assert want[0, 0, 0, 0] == -1.0
    xw = torch.full((2, H, W_, C + 8), 99.0, device=dev)
    xw[..., 4:4 + C] = xd
    out = torch.full(got.shape[:3] + (C + 12,), SENTINEL, device=dev)
    ops.pool3x3(xw, "max", c=C, x_off=4, out=out, y_off=8)
    assert np.array_equal(out[..., 8:8 + C].cpu().numpy().astype(np.float64), want)
    assert bool((out[..., :8] == SENTINEL).all()) and bool((out[..., 8 + C:] == SENTINEL).all())


@pytest.mark.parametrize("H,W_", [(1, 1), (2, 1), (5, 4), (35, 35)])
@pytest.mark.parametrize("C", [4, 288])
def test_avg_pool_is_exact_and_always_divides_by_nine(dev, H, W_, C):
    from mmhand_amd import ops
    x = _pool_input(2, H, W_, C, 82)
    x[0, 0, 0, :] = 7.0
    # the window sum is an integer: float64 sum / 9 rounded once to fp32 is the correctly rounded fp32 quotient
    want = O.avg_pool(x).astype(np.float32)
    xd = torch.from_numpy(x.astype(np.float32)).to(dev)
    got = ops.pool3x3(xd, "avg").cpu().numpy()
    assert got.shape == (2, H, W_, C) and np.array_equal(_bits(got), _bits(want))
    if (H, W_) == (1, 1):
        assert got[0, 0, 0, 0] == np.float32(7.0 / 9.0)             # one pixel inside, eight of padding: still / 9
    xw = torch.full((2, H, W_, C + 8), 99.0, device=dev)
    xw[..., 4:4 + C] = xd
    out = torch.full((2, H, W_, C + 12), SENTINEL, device=dev)
    ops.pool3x3(xw, "avg", c=C, x_off=4, out=out, y_off=8)
    assert np.array_equal(_bits(out[..., 8:8 + C].cpu().numpy()), _bits(want))
    assert bool((out[..., :8] == SENTINEL).all()) and bool((out[..., 8 + C:] == SENTINEL).all())


@pytest.mark.parametrize("H,W_", [(8, 8), (2, 1)])
def test_global_avgpool_is_exact(dev, H, W_):
    from mmhand_amd import ops
    x = _pool_input(3, H, W_, 2048, 83)
    want = (x.reshape(3, H * W_, 2048).sum(1) / float(H * W_)).astype(np.float32)      # integer sums, dyadic divisors: exact
    got = ops.global_avgpool(torch.from_numpy(x.astype(np.float32)).to(dev)).cpu().numpy()
    assert got.shape == (3, 2048) and np.array_equal(_bits(got), _bits(want)) and np.abs(want).max() > 1


# ------------------------------------------------------------------------------------------------- score
@pytest.mark.parametrize("n", [1, 3, 64, 70])
def test_score_is_float64(dev, n):
    from mmhand_amd import ops
    z = (hashed(91, n * 1000, SEED).reshape(n, 1000) * 80.0).astype(np.float32)          # logits spanning +-80
    z[:, 1000 - 8:] = 0.0
    if n >= 3:
        # row 2 = log of the mean of the softmaxes of rows 0 and 1: its softmax is (up to the fp32 logits) the mean row of
        # the three, so its terms cancel
        z[:3] *= 0.1
        p = np.exp(z[:2].astype(np.float64))
        p /= p.sum(1, keepdims=True)
        z[2] = np.log(p.mean(0)).astype(np.float32)
    cs = 1008
    buf = np.full((n, cs), 1e30, dtype=np.float32)                                       # lanes beyond `classes` are not read
    buf[:, :1000] = z
    kl, py = ops.inception_score(torch.from_numpy(buf).to(dev), classes=1000)
    kl, py = kl.cpu().numpy(), py.cpu().numpy()
    wkl, wpy, ws = O.score(z)
    assert kl.dtype == np.float64 and kl.shape == (n,) and py.shape == (1000,)
    assert np.abs(py - wpy).max() <= 1e-12 * wpy.max() and np.all(np.abs(py - wpy) <= 1e-12 * wpy + 1e-300)
    # a row's kl is a sum of about 1000 terms pyx log(pyx / py) of both signs.  A term's error is a few ulp of its own size (the
    # product) plus pyx times a few ulp of 1 (the quotient's rounding moves the logarithm by that much, however small the
    # logarithm is); summed: 1e-12 of (sum |term| + sum pyx) = size + 1.  For an ordinary row that is 1e-12 relative; for the row
    # that equals py, whose kl is 1e-15 by cancellation, it is the only bound any float64 implementation can meet.
    e = np.exp(z.astype(np.float64) - z.astype(np.float64).max(1, keepdims=True))
    pyx = e / e.sum(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        size = np.where(pyx > 0, np.abs(pyx * np.log(pyx / wpy)), 0.0).sum(1)
    assert np.all(np.abs(kl - wkl) <= 1e-12 * (size + 1.0)), np.abs(kl - wkl).max()
    assert np.all(np.abs(kl - wkl)[wkl > 1e-3] <= 1e-12 * wkl[wkl > 1e-3])
    assert abs(float(np.exp(np.mean(kl))) - ws) <= 1e-12 * ws
    if n == 1:
        assert kl[0] == 0.0 and float(np.exp(np.mean(kl))) == 1.0            # py is the row itself: log(1) = 0
    else:
        assert ws > 1.05
    if n == 3:      # only there is row 2 the mean of ALL rows
        assert abs(wkl[2]) < 1e-6 and abs(kl[2]) < 1e-6
    # the same rows again: the same bits (no atomics, a fixed order)
    kl2, py2 = ops.inception_score(torch.from_numpy(buf).to(dev), classes=1000)
    assert np.array_equal(kl2.cpu().numpy(), kl) and np.array_equal(py2.cpu().numpy(), py)


# ------------------------------------------------------------------------------------------------- the network
@pytest.fixture(scope="module")
def sd32():
    """the generated checkpoint as a file would hold it: fp32"""
    return OrderedDict((k, v.float() if v.is_floating_point() else v) for k, v in O.state_dict(SEED).items())


@pytest.fixture(scope="module")
def net(dev, sd32):
    from mmhand_amd import inception
    return inception.InceptionV3(dev).load_state_dict(sd32)


@pytest.fixture(scope="module")
def runs(dev, net, sd32):
    """the two golden inputs through the device network and through the oracle (float64, and PyTorch's fp32 on the CPU) on the
    weights the device got, computed once and left alone"""
    sd64 = OrderedDict((k, v.double()) for k, v in sd32.items() if v.is_floating_point())
    out = []
    for shape, index in (((2, 3, 75, 75), 0), ((1, 3, 107, 91), 1)):
        x = O.net_inputs(shape, SEED, index).astype(np.float32)
        xd = torch.zeros((shape[0], shape[2], shape[3], 4), device=dev)
        xd[..., :3] = torch.from_numpy(x).to(dev).permute(0, 2, 3, 1)
        out.append(dict(x=xd, got=net(xd).cpu().numpy(), f64=O.forward(sd64, x.astype(np.float64)).numpy(),
                        f32=O.forward(sd64, x, torch.float32).double().numpy()))
    return out


def _rel_l1(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).sum() / np.abs(b).sum())


def test_network_stays_within_twice_pytorch_fp32(runs):
    """relative L1 of the logits against the float64 forward of the same graph on the same inputs and weights: at most twice
    what PyTorch's fp32 CPU forward keeps (the factor allows for another summation order and nothing else).  The second input
    ends on a 2 x 1 grid with 5 x 4 in Mixed_6: swapped 1x7 / 7x1 paddings cannot pass."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "inception.npz"))
    for r, key in zip(runs, ("logits_a", "logits_b")):
        got, ref = _rel_l1(r["got"], r["f64"]), _rel_l1(r["f32"], r["f64"])
        print("%s: device %.3e, PyTorch fp32 %.3e, ratio %.2f" % (key, got, ref, got / ref))
        assert r["got"].shape == r["f64"].shape == gold[key].shape
        assert got <= 2.0 * ref, (key, got, ref)
        assert _rel_l1(r["f64"], gold[key]) < 1e-5          # fp32-rounded weights and inputs against the recorded float64 run


def test_forward_does_not_depend_on_the_winograd_mode(net, runs):
    from mmhand_amd import lib, ops
    before = lib.get_option("conv_levels")
    try:
        for mode in ("off", "all"):
            ops.set_winograd_mode(mode)
            assert np.array_equal(_bits(net(runs[1]["x"]).cpu().numpy()), _bits(runs[1]["got"])), mode
            assert lib.get_option("conv_levels") == (2 if mode == "off" else 1)      # put back after the call
    finally:
        ops.set_winograd_mode("all")
        lib.call("mmh_set_option", b"conv_levels", before)


def test_network_takes_more_rows_than_one_linear_launch(dev, net, runs):
    """mmh_linear_fprop takes at most 64 rows: a batch of 66 goes through it in two pieces"""
    x = runs[0]["x"]
    big = x[:1].repeat(66, 1, 1, 1).contiguous()
    big[65] = x[1]
    got = net(big).cpu().numpy()
    assert got.shape == (66, 1000) and np.isfinite(got).all()
    scale = np.abs(runs[0]["f64"]).max()
    for row, want in ((0, 0), (63, 0), (64, 0), (65, 1)):
        assert np.abs(got[row] - runs[0]["f64"][want]).max() <= 1e-4 * scale, row
    assert np.abs(got[65] - got[64]).max() > 1e-2 * scale


# ------------------------------------------------------------------------------------------------- evaluate --inception
@pytest.fixture
def work_dir():
    """a scratch directory whose PATH does not contain "test" (the loader keys on it)"""
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="mmh_is_")
    assert "test" not in d
    yield d
    shutil.rmtree(d, ignore_errors=True)


def test_evaluate_inception_in_three_modes(dev, net, sd32, work_dir, monkeypatch):
    from PIL import Image
    from mmhand_amd import evaluate, inception, ops
    from mmhand_amd.networks import Generator
    from tests._dataset_fixture import write_rhd
    root = os.path.join(work_dir, "rhd")
    write_rhd(root, n=6, size=32)
    monkeypatch.chdir(work_dir)
    torch.save(OrderedDict(("module." + k, v) for k, v in sd32.items()), "inception.pth")
    os.makedirs(os.path.join("checkpoints", "ev"))
    torch.manual_seed(5)
    torch.save(Generator([3, 42, 6], 3, 8, "instance", False, 2).state_dict(), os.path.join("checkpoints", "ev", "latest_net_netG.pth"))

    fed = []
    feed = inception.InceptionScorer.feed

    def spy(self, images, layout="nchw", paths=None):
        feed(self, images, layout, paths)
        fed.append((images.detach().float().cpu().numpy() if layout == "nchw" else images.cpu().numpy(), layout,
                    self._logits[-1].cpu().numpy()))

    monkeypatch.setattr(inception.InceptionScorer, "feed", spy)
    flags = ["--inception", "inception.pth", "--is_group", "4"]

    def check(res, js, n):
        """the JSON's figures = the oracle's score of the logits that InceptionV3 gives for the oracle's preprocess of the
        same bytes: order, grouping, quantisation and resize plumbing (closeness of the network is the tests' above)"""
        logits, u8s = [], []
        for img, layout, got in fed:
            u8 = np.ascontiguousarray(img[..., ::-1]) if layout == "bgr_hwc" else np.ascontiguousarray(O.to_bytes(img).transpose(0, 2, 3, 1))
            lg = net(torch.from_numpy(O.preprocess(u8, 299)).to(dev)).cpu().numpy()
            assert np.array_equal(_bits(lg), _bits(got))
            logits.append(lg)
            u8s.append(u8)
        logits = np.concatenate(logits)
        avg, std, all_, groups, kl = O.grouped(logits, 4)
        s = js["summary"]
        assert logits.shape == (n, 1000) and s["n"] == n and s["is_groups"] == groups == -(-n // 4)
        for key, want in (("IS_avg", avg), ("IS_std", std), ("IS_all", all_)):
            assert abs(s[key] - want) <= 1e-12 * max(want, 1.0), (key, s[key], want)
        assert np.abs(np.array([r["is_kl"] for r in res["rows"]]) - kl).max() <= 1e-12 * max(kl.max(), 1.0)
        return np.concatenate(u8s), s

    # 1. a generator checkpoint: the fake batch goes to the scorer as it lies on the device
    base = ["--name", "ev", "--dataroot", root, "--dataset", "rhd", "--batchSize", "4"]
    random.seed(11)
    res = evaluate.main(base + flags + ["--results_json", "g.json", "--per_image_csv", "g.csv"])
    js = json.load(open("g.json"))
    u8_gen, s_gen = check(res, js, 6)
    assert fed[0][1] == "nchw" and [len(f[0]) for f in fed] == [4, 2]
    assert {"SSIM_avg", "IS_avg", "IS_std", "IS_all", "is_groups"} <= set(s_gen) and js["options"]["inception"] == "inception.pth"
    assert list(csv.reader(open("g.csv")))[0] == ["target", "source", "ssim", "l1", "psnr", "is_kl"]
    # without --inception the files are what they were: no new key anywhere, nothing fed
    fed.clear()
    random.seed(11)
    plain = evaluate.main(base + ["--results_json", "n.json", "--per_image_csv", "n.csv"])
    n = json.load(open("n.json"))
    assert not fed and set(n["summary"]) == {"SSIM_avg", "SSIM_std", "L1_avg", "PSNR_avg", "n"}
    assert not set(n["options"]) & set(evaluate.IS_FLAGS)
    assert list(csv.reader(open("n.csv")))[0] == ["target", "source", "ssim", "l1", "psnr"]
    assert [r["ssim"] for r in plain["rows"]] == [r["ssim"] for r in res["rows"]]

    # 2. the same images as the PNGs aug would write: --generated, and identical IS figures
    for r, u8 in zip(res["rows"], u8_gen):
        os.makedirs(os.path.join("gen", "color"), exist_ok=True)
        Image.fromarray(u8).save(os.path.join("gen", "color", os.path.basename(r["target"])))
    fed.clear()
    random.seed(11)
    res_d = evaluate.main(["--generated", "gen", "--dataroot", root, "--dataset", "rhd", "--batchSize", "3", "--results_json", "d.json"] + flags)
    u8_dir, s_dir = check(res_d, json.load(open("d.json")), 6)
    assert fed[0][1] == "bgr_hwc" and np.array_equal(u8_dir, u8_gen)
    assert [r["target"] for r in res_d["rows"]] == [r["target"] for r in res["rows"]]
    assert s_dir["IS_all"] == s_gen["IS_all"] and s_dir["IS_avg"] == s_gen["IS_avg"] and s_dir["IS_std"] == s_gen["IS_std"]

    # 3. any directory of PNGs, no labels: the real images of the prepared directory, in sorted order
    fed.clear()
    res_i = evaluate.main(["--is_images", os.path.join(root, "color"), "--batchSize", "4", "--results_json", "i.json", "--per_image_csv", "i.csv"] + flags)
    u8_img, s_img = check(res_i, json.load(open("i.json")), 6)
    names = sorted(os.listdir(os.path.join(root, "color")))
    assert [os.path.basename(r["target"]) for r in res_i["rows"]] == names
    assert np.array_equal(u8_img[0], np.array(Image.open(os.path.join(root, "color", names[0])).convert("RGB")))
    assert set(s_img) == {"n", "IS_avg", "IS_std", "IS_all", "is_groups"} and s_img["IS_all"] >= 1.0
    table = list(csv.reader(open("i.csv")))
    assert table[0] == ["target", "is_kl"] and len(table) == 7
