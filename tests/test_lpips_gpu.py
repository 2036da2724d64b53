"""LPIPS on the device (csrc/lpips.hip, mmhand_amd/lpips.py and `evaluate --lpips`) against tests/_lpips_oracle.py: the scaling
layer bit for bit, the layer distance within a bound derived for float64 arithmetic in any order, closed-form cases, determinism,
independence of the batch and symmetry bit for bit, and the scorer end to end.  All weights are generated: no figure here says
anything about images."""
import csv
import ctypes as C
import json
import os
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import _lpips_oracle as O

pytestmark = pytest.mark.gpu
SENTINEL = -77.0
EPS = 1e-10
# |dev - ref| <= REL * sum_p sum_c |w_c| (ah_c - bh_c)^2 / (H W): float64 throughout on fp32 inputs, at most C + H W additions per
# chain and a handful of roundings per term, each 2^-53 relative - about 2e-13 at the largest case here
REL = 1e-12
MAX_CHUNKS, FIN_STEP = 1024, 256            # csrc/lpips.hip: LP_MAX_CHUNKS, LP_FIN_TPB


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _visit_px(c):
    """pixels a workgroup visits at a time: four waves of 64 / G pixels, G = the smallest power of two >= min(C / 4, 64)"""
    g = 1
    while g < min(c // 4, 64):
        g *= 2
    return 4 * (64 // g)


def _chunks(px, c):
    return min(-(-px // _visit_px(c)), MAX_CHUNKS)


@pytest.fixture(scope="module", autouse=True)
def _give_memory_back():
    yield
    import gc
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _maps(shape, seed=0):
    rng = np.random.RandomState(seed)
    a = np.maximum(rng.randn(*shape), 0).astype(np.float32)          # post-ReLU features: non-negative, many zeros
    b = np.maximum(rng.randn(*shape), 0).astype(np.float32)
    w = rng.uniform(-0.25, 1.0, shape[3]).astype(np.float32)
    return a, b, w


def _layer(dev, a, b, w):
    from mmhand_amd import ops
    out = ops.lpips_layer(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(np.asarray(w, dtype=np.float32)).to(dev))
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------- preprocess
def _image(kind, B, H, W_, seed):
    """(host array in the layout's form, torch dtype or None)"""
    rng = np.random.RandomState(seed)
    if kind == "u8":
        return rng.randint(0, 256, (B, H, W_, 3)).astype(np.uint8)
    return rng.uniform(-1, 1, (B, 3, H, W_)).astype(np.float32)


@pytest.mark.parametrize("B,H,W_", [(2, 16, 16), (1, 5, 7)])
@pytest.mark.parametrize("kind", ["f32", "bf16", "f16", "u8"])
def test_preprocess_is_the_oracle_rounded_once(dev, kind, B, H, W_):
    from mmhand_amd import ops
    host = _image(kind, B, H, W_, 3)
    layout = "bgr_hwc" if kind == "u8" else "nchw"
    t = torch.from_numpy(host)
    if kind in ("bf16", "f16"):
        t = t.to(torch.bfloat16 if kind == "bf16" else torch.float16)
        host = t.float().numpy()                                                        # the values the device reads
    got = ops.lpips_preprocess(t.to(dev), layout)
    want = O.preprocess(host, layout)
    assert got.shape == (B, H, W_, 4) and got.dtype == torch.float32
    g = got.cpu().numpy()
    assert np.array_equal(g.view(np.uint32), want.view(np.uint32))
    assert (g[..., 3].view(np.uint32) == 0).all()                                       # lane 3: +0.0 exactly
    # a non-contiguous view of the same values: every second column of a wider buffer (nchw), a BGR view of BGRA pixels (hwc)
    if layout == "nchw":
        wide = torch.zeros((B, 3, H, 2 * W_), dtype=t.dtype)
        wide[..., ::2] = t
        view = wide.to(dev)[..., ::2]
    else:
        wide = torch.zeros((B, H, W_, 4), dtype=torch.uint8)
        wide[..., :3] = t
        view = wide.to(dev)[..., :3]
    assert not view.is_contiguous()
    assert torch.equal(ops.lpips_preprocess(view, layout), got)


def test_preprocess_of_an_nhwc_buffers_nchw_view(dev):
    """a generator's output is an NCHW view of an NHWC buffer: channel stride 1"""
    from mmhand_amd import ops
    host = _image("f32", 2, 16, 16, 5)
    view = torch.from_numpy(np.ascontiguousarray(host.transpose(0, 2, 3, 1))).to(dev).permute(0, 3, 1, 2)
    assert view.stride(1) == 1
    got = ops.lpips_preprocess(view, "nchw").cpu().numpy()
    assert np.array_equal(got.view(np.uint32), O.preprocess(host, "nchw").view(np.uint32))
    with pytest.raises(ValueError):
        ops.lpips_preprocess(view[:, :2], "nchw")
    with pytest.raises(ValueError):
        ops.lpips_preprocess(view, "rgb")


# ------------------------------------------------------------------------------------------------- layer against the oracle
# the issue's shapes; (2,367,359,8): 131753 pixels at 128 per visit = 1030 visits > the 1024-workgroup cap (the last six
# workgroups' second visit is the ragged tail) and 1024 partials per image = four steps of the finishing workgroup;
# (1,9,11,24): six quads on eight lanes, two idle; (1,3,5,260): the second quad per lane ragged
SHAPES = [(1, 1, 1, 64), (3, 5, 7, 64), (2, 16, 16, 128), (1, 33, 31, 256), (2, 3, 3, 512), (2, 2, 2, 4),
          (2, 367, 359, 8), (1, 9, 11, 24), (1, 3, 5, 260)]


@pytest.mark.parametrize("shape", SHAPES)
def test_layer_within_the_derived_bound(dev, shape):
    from mmhand_amd import lib as L
    B, H, W_, c = shape
    assert L.load().mmh_lpips_layer_ws_bytes(B, H, W_, c) == 8 * B * _chunks(H * W_, c)
    if shape == (2, 367, 359, 8):
        assert _chunks(H * W_, c) == MAX_CHUNKS > FIN_STEP and -(-H * W_ // _visit_px(c)) > MAX_CHUNKS
    a, b, w = _maps(shape, seed=sum(shape))
    ref, scale = O.layer(a, b, w)
    got = _layer(dev, a, b, w)
    err = np.abs(got - ref)
    print("shape %s: max |dev - ref| / scale = %.3e (ref %s)" % (shape, (err / scale).max(), ref[:2]))
    assert np.isfinite(got).all() and (err <= REL * scale).all(), (got, ref, scale)
    ones, ones_scale = O.layer(a, b, np.ones(c))
    got1 = _layer(dev, a, b, np.ones(c))
    assert (np.abs(got1 - ones) <= REL * ones_scale).all() and (got1 > 0).all()


# ------------------------------------------------------------------------------------------------- closed forms
def test_one_differing_pixel_and_channel(dev):
    """the maps agree everywhere but at pixel (2, 3): a = (3, 4, 0 ...), b = (3, 0, 0 ...): lengths 5 and 3 exactly"""
    shape = (1, 4, 4, 64)
    a, _, w = _maps(shape, seed=1)
    b = a.copy()
    a[0, 2, 3, :], b[0, 2, 3, :] = 0, 0
    a[0, 2, 3, 0], a[0, 2, 3, 1], b[0, 2, 3, 0] = 3, 4, 3
    w = w.astype(np.float64)
    t0, t1 = 3.0 / (5.0 + EPS) - 3.0 / (3.0 + EPS), 4.0 / (5.0 + EPS)
    want, scale = (w[0] * t0 * t0 + w[1] * t1 * t1) / 16.0, (abs(w[0]) * t0 * t0 + abs(w[1]) * t1 * t1) / 16.0
    got = _layer(dev, a, b, w)[0]
    assert abs(got - want) <= 8 * 2.0 ** -53 * scale, (got, want)
    # a one-hot head sees its own channel alone, and a head that is zero on both channels sees nothing
    for ch, t in ((0, t0), (1, t1)):
        hot = np.zeros(64)
        hot[ch] = 1.0
        assert abs(_layer(dev, a, b, hot)[0] - t * t / 16.0) <= 4 * 2.0 ** -53 * t * t / 16.0
    blind = np.ones(64)
    blind[:2] = 0
    assert _layer(dev, a, b, blind)[0] == 0.0
    # negative heads: the exact negative, bit for bit
    pos, neg = _layer(dev, a, b, np.abs(w)), _layer(dev, a, b, -np.abs(w))
    assert pos[0] > 0 and np.array_equal(_bits64(-neg), _bits64(pos))
    one = np.zeros(64)
    one[1] = -0.5
    assert abs(_layer(dev, a, b, one)[0] + 0.5 * t1 * t1 / 16.0) <= 4 * 2.0 ** -53 * 0.5 * t1 * t1 / 16.0


def test_zero_vectors_give_what_eps_gives(dev):
    """pixel (0, 0): a all zero, b = 2 in one channel -> (0 / 1e-10 - 2 / (2 + 1e-10))^2; pixel (1, 1): zero in both -> 0"""
    shape = (2, 2, 2, 128)
    a, _, _ = _maps(shape, seed=2)
    b = a.copy()
    a[:, 0, 0, :], b[:, 0, 0, :] = 0, 0
    b[:, 0, 0, 77] = 2
    a[:, 1, 1, :], b[:, 1, 1, :] = 0, 0
    w = np.full(128, 0.5)
    t = 2.0 / (2.0 + EPS)
    want = 0.5 * t * t / 4.0
    got = _layer(dev, a, b, w)
    assert np.isfinite(got).all() and (np.abs(got - want) <= 4 * 2.0 ** -53 * want).all(), (got, want)
    both = _layer(dev, np.zeros(shape, np.float32), np.zeros(shape, np.float32), w)
    assert np.array_equal(_bits64(both), _bits64(np.zeros(2)))


def test_a_equal_twice_b_leaves_the_eps_term(dev):
    """b = 0.5 in four channels (length 1), a = 2 b (length 2) at every pixel: ah - bh = 1 / (2 + eps) - 0.5 / (1 + eps), about
    eps / 4 = 2.5e-11 - the lengths are exact in any order and division is correctly rounded, so the term is this float64 expression"""
    shape = (1, 4, 8, 256)
    b = np.zeros(shape, np.float32)
    b[..., [3, 64, 130, 255]] = 0.5
    a = 2 * b
    t = 1.0 / (2.0 + EPS) - 0.5 / (1.0 + EPS)
    assert 2.4e-11 < t < 2.6e-11
    want = 4 * t * t
    got = _layer(dev, a, b, np.ones(256))[0]
    assert abs(got - want) <= REL * want, (got, want)
    assert _layer(dev, a, a, np.ones(256))[0] == 0.0


# ------------------------------------------------------------------------------------------------- determinism, independence
@pytest.mark.parametrize("shape", [(3, 5, 7, 64), (3, 33, 31, 256), (3, 3, 3, 512), (3, 150, 150, 4)])
def test_bit_equal_runs_batches_and_argument_order(dev, shape):
    from mmhand_amd import ops
    a, b, w = _maps(shape, seed=7)
    ta, tb, tw = (torch.from_numpy(x).to(dev) for x in (a, b, w))
    first = ops.lpips_layer(ta, tb, tw)
    assert torch.equal(first, ops.lpips_layer(ta, tb, tw))
    assert torch.equal(first, ops.lpips_layer(tb, ta, tw))
    for i in range(shape[0]):
        alone = ops.lpips_layer(ta[i:i + 1].contiguous(), tb[i:i + 1].contiguous(), tw)
        assert torch.equal(alone, first[i:i + 1]), i
    assert (ops.lpips_layer(ta, ta, tw) == 0).all()


def test_guards_and_refusals(dev):
    from mmhand_amd import lib as L
    from mmhand_amd import ops
    shape = (3, 9, 9, 64)
    a, b, w = _maps(shape, seed=9)
    ta, tb, tw = (torch.from_numpy(x).to(dev) for x in (a, b, w))
    n = L.load().mmh_lpips_layer_ws_bytes(*shape) // 8
    assert n == 3 * _chunks(81, 64)
    g = 32
    obuf = torch.full((3 + 2 * g,), SENTINEL, dtype=torch.float64, device=dev)
    wbuf = torch.full((n + 2 * g,), SENTINEL, dtype=torch.float64, device=dev)
    out = ops.lpips_layer(ta, tb, tw, out=obuf[g:g + 3], ws=wbuf[g:g + n])
    assert torch.equal(out, ops.lpips_layer(ta, tb, tw))
    o, s = obuf.cpu().numpy(), wbuf.cpu().numpy()
    assert (o[:g] == SENTINEL).all() and (o[g + 3:] == SENTINEL).all() and (s[:g] == SENTINEL).all() and (s[g + n:] == SENTINEL).all()
    assert (s[g:g + n] != SENTINEL).all()                                                # every partial is written
    # refused: nothing is launched, the output keeps its sentinel
    keep = torch.full((3,), SENTINEL, dtype=torch.float64, device=dev)
    ws = torch.empty((4096,), dtype=torch.float64, device=dev)

    def raw(c, ws_bytes, x=ta, y=tb):
        return L.load().mmh_lpips_layer(ops._ptr(x), ops._ptr(y), ops._ptr(tw), 3, 9, 9, c, ops._ptr(keep), ops._ptr(ws), ws_bytes,
                                        ops._stream())

    assert raw(6, 4096 * 8) != 0 and b"C=6" in L.load().mmh_last_error()
    assert raw(516, 4096 * 8) != 0
    assert raw(64, n * 8 - 8) != 0 and b"workspace" in L.load().mmh_last_error()
    assert raw(64, n * 8, x=None) != 0
    torch.cuda.synchronize()
    assert (keep.cpu().numpy() == SENTINEL).all()
    assert raw(64, n * 8) == 0 and torch.equal(keep, out)
    six = torch.zeros((1, 2, 2, 6), device=dev)
    with pytest.raises(ValueError, match="refused"):
        ops.lpips_layer(six, six, torch.ones(6, device=dev))
    with pytest.raises(ValueError):
        ops.lpips_layer(ta, tb[:2].contiguous(), tw)
    with pytest.raises(ValueError):
        ops.lpips_layer(ta, tb, tw[:32].contiguous())
    with pytest.raises(ValueError):
        ops.lpips_layer(ta, tb.double(), tw)
    with pytest.raises(RuntimeError, match="workspace"):
        ops.lpips_layer(ta, tb, tw, ws=wbuf[:n - 1])


# ------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def weights():
    return O.vgg16_state_dict(0), O.lin_state_dict(1)


@pytest.fixture(scope="module")
def net(dev, weights):
    from mmhand_amd import lpips
    return lpips.Vgg16Lpips(dev).load_state_dict(weights[0])


def _table_distance(v, ref, scale):
    """the distance of a [B,5] table of layer scores to the float64 one: sum |v - ref| over sum of the |w| form"""
    return float(np.abs(v - ref).sum() / scale.sum())


@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_scorer_against_float64_and_torch_fp32(dev, net, weights, kind):
    """LpipsScorer on two 32 x 32 pairs against the float64 oracle.  The bar is what fp32 convolutions cost: the same graph
    with torch in fp32 on the CPU - the same rounded input, F.conv2d / relu / max_pool2d in fp32, the layer distance of its
    taps in float64 as the device takes it - has its own distance to float64, and the device may be at most twice as far.
    Measured on one MI355X: nchw fp32 device 2.4e-08 against torch 9.9e-08; bgr_hwc bytes device 1.7e-08
    against torch 5.7e-08."""
    from mmhand_amd import lpips
    sd, lin = weights
    layout = "bgr_hwc" if kind == "u8" else "nchw"
    pred, target = _image(kind, 2, 32, 32, 11), _image(kind, 2, 32, 32, 12)
    sc = lpips.LpipsScorer(net, lin, device=dev)
    sc.feed(torch.from_numpy(pred).to(dev), layout, torch.from_numpy(target).to(dev), layout, [{"target": "p0"}, {"target": "p1"}])
    got = sc.layers()
    ref, scale = O.lpips(pred, layout, target, layout, sd, lin)
    cpu32, _ = O.lpips(pred, layout, target, layout, sd, lin, dtype=torch.float32)
    d_dev, d_cpu = _table_distance(got, ref, scale), _table_distance(cpu32, ref, scale)
    print("%s: device %.3e, torch fp32 CPU %.3e of the |w| scale; LPIPS %s" % (layout, d_dev, d_cpu, ref.sum(1)))
    assert got.shape == (2, 5) and np.isfinite(got).all() and d_cpu > 0
    assert d_dev <= 2 * d_cpu, (d_dev, d_cpu)
    res, rows = sc.results(), sc.rows()
    assert set(res) == {"LPIPS_avg", "LPIPS_layers", "lpips_lin", "n"} and res["n"] == 2 and res["lpips_lin"] == "custom"
    assert [r["target"] for r in rows] == ["p0", "p1"]
    assert [r["lpips"] for r in rows] == sc.total(got).tolist() and res["LPIPS_avg"] == float(np.mean(sc.total(got)))
    assert res["LPIPS_layers"] == got.mean(0).tolist()
    # uniform heads: the package's lpips=False form
    un = lpips.LpipsScorer(net, "uniform", device=dev)
    un.feed(torch.from_numpy(pred).to(dev), layout, torch.from_numpy(target).to(dev), layout)
    uref, uscale = O.lpips(pred, layout, target, layout, sd, "uniform")
    ucpu, _ = O.lpips(pred, layout, target, layout, sd, "uniform", dtype=torch.float32)
    assert _table_distance(un.layers(), uref, uscale) <= 2 * _table_distance(ucpu, uref, uscale)
    assert un.results()["lpips_lin"] == "uniform" and (un.layers() > 0).all()
    # an image against itself: exactly zero
    me = lpips.LpipsScorer(net, lin, device=dev)
    me.feed(torch.from_numpy(pred).to(dev), layout, torch.from_numpy(pred).to(dev).clone(), layout)
    assert np.array_equal(_bits64(me.layers()), _bits64(np.zeros((2, 5)))) and me.results()["LPIPS_avg"] == 0.0


def test_scorer_chunks_mixed_layouts_and_refusals(dev, net, weights, monkeypatch):
    """a batch cut into trunk passes gives the bits of the whole batch; bytes against floats of the same image give zero"""
    from mmhand_amd import lpips, ops
    sd, lin = weights
    pred, target = _image("u8", 3, 16, 32, 21), _image("u8", 3, 16, 32, 22)
    tp, tt = torch.from_numpy(pred).to(dev), torch.from_numpy(target).to(dev)
    sc = lpips.LpipsScorer(net, lin, device=dev)
    whole = sc.distances(tp, "bgr_hwc", tt, "bgr_hwc")
    monkeypatch.setattr(lpips.LpipsScorer, "chunk_size", staticmethod(lambda H, W_: 2))
    assert torch.equal(sc.distances(tp, "bgr_hwc", tt, "bgr_hwc"), whole)
    taps = net.forward_taps(ops.lpips_preprocess(tp, "bgr_hwc"))
    assert [tuple(t.shape) for t in taps] == [(3, 16, 32, 64), (3, 8, 16, 128), (3, 4, 8, 256), (3, 2, 4, 512), (3, 1, 2, 512)]
    # the same image as bytes and as fp32 values: the inputs differ by one fp32 rounding (6e-8), the distance by its square
    as_float = torch.from_numpy(O.rgb_pm1(pred, "bgr_hwc").transpose(0, 3, 1, 2).copy()).float().to(dev)
    assert (sc.distances(tp, "bgr_hwc", as_float, "nchw").abs() <= 1e-9).all()
    with pytest.raises(ValueError, match="multiples of 16"):
        sc.distances(tp[:, :, :24], "bgr_hwc", tt[:, :, :24], "bgr_hwc")
    with pytest.raises(ValueError):
        sc.distances(tp, "bgr_hwc", tt[:2], "bgr_hwc")
    with pytest.raises(ValueError):
        sc.feed(tp, "bgr_hwc", tt, "bgr_hwc", paths=[{}])


# ------------------------------------------------------------------------------------------------- evaluate
@pytest.fixture
def work_dir():
    """a scratch directory whose PATH does not contain "test" (the loader keys on it)"""
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="mmh_lpips_")
    assert "test" not in d
    yield d
    shutil.rmtree(d, ignore_errors=True)


def test_evaluate_lpips_in_three_modes(dev, net, weights, work_dir, tmp_path, monkeypatch):
    from PIL import Image
    from mmhand_amd import evaluate, lpips
    from mmhand_amd.networks import Generator
    from tests._dataset_fixture import write_rhd
    sd, lin = weights
    root = os.path.join(work_dir, "rhd")
    write_rhd(root, n=6, size=32)
    monkeypatch.chdir(work_dir)
    vgg_path, lin_path = os.path.join(tmp_path, "vgg16.pth"), os.path.join(tmp_path, "lin.pth")
    torch.save(OrderedDict(("module." + k, v) for k, v in sd.items()), vgg_path)
    torch.save(lin, lin_path)
    os.makedirs(os.path.join("checkpoints", "ev"))
    torch.manual_seed(5)
    torch.save(Generator([3, 42, 6], 3, 8, "instance", False, 2).state_dict(), os.path.join("checkpoints", "ev", "latest_net_netG.pth"))

    fed = []
    feed = lpips.LpipsScorer.feed

    def spy(self, pred, pred_layout, target, target_layout, paths=None):
        fed.append((pred.clone(), pred_layout, target.clone(), target_layout))
        return feed(self, pred, pred_layout, target, target_layout, paths)

    monkeypatch.setattr(lpips.LpipsScorer, "feed", spy)

    def direct(lin_src):
        sc = lpips.LpipsScorer(net, lin_src, device=dev)
        for args in fed:
            feed(sc, *args)
        return sc

    keys = {"LPIPS_avg", "LPIPS_layers", "lpips_lin"}
    # 1. a generator checkpoint: the fake batches against their targets
    base = ["--name", "ev", "--dataroot", root, "--dataset", "rhd", "--batchSize", "4"]
    flags = ["--lpips", vgg_path, "--lpips_lin", lin_path]
    random.seed(11)
    res = evaluate.main(base + flags + ["--results_json", "g.json", "--per_image_csv", "g.csv"])
    doc = json.load(open("g.json"))
    s_gen = doc["summary"]
    assert keys <= set(s_gen) and s_gen["n"] == 6 and s_gen["lpips_lin"] == lin_path and set(evaluate.LPIPS_FLAGS) <= set(doc["options"])
    assert [f[1] for f in fed] == ["nchw", "nchw"] and [f[0].shape[0] for f in fed] == [4, 2]
    want = direct(lin_path)
    assert s_gen["LPIPS_avg"] == want.results()["LPIPS_avg"] and s_gen["LPIPS_layers"] == want.results()["LPIPS_layers"]
    assert len(s_gen["LPIPS_layers"]) == 5 and s_gen["LPIPS_avg"] > 0
    table = list(csv.reader(open("g.csv")))
    assert table[0] == ["target", "source", "ssim", "l1", "psnr", "lpips"] and len(table) == 7
    assert [float(r[5]) for r in table[1:]] == [r["lpips"] for r in want.rows()] == [r["lpips"] for r in res["rows"]]
    # the float64 oracle on the very tensors the scorer was fed: the pipeline is the definition's
    got = want.layers()
    ref = np.concatenate([O.lpips(p.cpu().numpy(), pl, t.cpu().numpy(), tl, sd, lin)[0] for p, pl, t, tl in fed])
    cpu = np.concatenate([O.lpips(p.cpu().numpy(), pl, t.cpu().numpy(), tl, sd, lin, dtype=torch.float32)[0] for p, pl, t, tl in fed])
    assert np.abs(got - ref).sum() <= 2 * np.abs(cpu - ref).sum()
    # without the flags the files are what they were
    fed.clear()
    random.seed(11)
    plain = evaluate.main(base + ["--results_json", "n.json", "--per_image_csv", "n.csv"])
    n = json.load(open("n.json"))
    assert set(n["summary"]) == {"SSIM_avg", "SSIM_std", "L1_avg", "PSNR_avg", "n"} and not set(n["options"]) & set(evaluate.LPIPS_FLAGS)
    assert open("n.csv").readline().strip() == "target,source,ssim,l1,psnr" and not fed
    assert [r["ssim"] for r in plain["rows"]] == [r["ssim"] for r in res["rows"]] and "lpips" not in plain["rows"][0]
    assert {k: v for k, v in s_gen.items() if k not in keys} == n["summary"]

    # 2. a directory of PNGs under the targets' names: --generated, uniform heads
    os.makedirs(os.path.join("gen", "color"), exist_ok=True)
    rng = np.random.RandomState(4)
    for r in res["rows"]:
        Image.fromarray(rng.randint(0, 256, size=(32, 32, 3), dtype=np.uint8)).save(os.path.join("gen", "color", os.path.basename(r["target"])))
    random.seed(11)
    out = evaluate.main(["--generated", "gen", "--dataroot", root, "--dataset", "rhd", "--batchSize", "3", "--results_json", "d.json",
                         "--lpips", vgg_path, "--lpips_lin", "uniform"])
    s_dir = json.load(open("d.json"))["summary"]
    assert [f[1] for f in fed] == ["bgr_hwc"] * 2 and fed[0][0].dtype == torch.uint8 and s_dir["lpips_lin"] == "uniform"
    want = direct("uniform")
    assert s_dir["LPIPS_avg"] == want.results()["LPIPS_avg"] and [r["lpips"] for r in out["rows"]] == [r["lpips"] for r in want.rows()]
    by_name = {os.path.basename(r["target"]): r["lpips"] for r in out["rows"]}

    # 3. two directories, no labels: the same pairs by relative name give the same values
    fed.clear()
    os.makedirs(os.path.join("ref", "color"))
    for name in by_name:
        Image.open(os.path.join(root, "color", name)).save(os.path.join("ref", "color", name))
    two = evaluate.main(["--lpips_images", "gen", "--lpips_ref", "ref", "--lpips", vgg_path, "--lpips_lin", "uniform", "--batchSize", "4",
                         "--results_json", "t.json", "--per_image_csv", "t.csv"])
    s_two = json.load(open("t.json"))
    assert set(s_two["summary"]) == keys | {"n"} and s_two["summary"]["n"] == 6 and s_two["generator"] is None
    assert not set(s_two["options"]) & set(evaluate.FID_FLAGS + evaluate.IS_FLAGS + evaluate.PCK_FLAGS)
    assert {os.path.basename(r["target"]): r["lpips"] for r in two["rows"]} == by_name
    assert open("t.csv").readline().strip() == "target,lpips"
    # an unpaired file is an error
    Image.fromarray(np.zeros((32, 32, 3), np.uint8)).save(os.path.join("ref", "color", "extra.png"))
    with pytest.raises(SystemExit, match="extra.png"):
        evaluate.main(["--lpips_images", "gen", "--lpips_ref", "ref", "--lpips", vgg_path, "--lpips_lin", "uniform"])
