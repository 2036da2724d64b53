"""The LPIPS feature's host side: the premises of the test oracle (tests/_lpips_oracle.py), the key mapping and width checks of
mmhand_amd.lpips's two loaders, the ABI of the three new entry points and the argument handling of mmhand_amd/evaluate.py.
No GPU."""
import fnmatch
import os
import re
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import _lpips_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mmh_lpips_preprocess", "mmh_lpips_layer_ws_bytes", "mmh_lpips_layer")


def _maps(shape, seed=0):
    rng = np.random.RandomState(seed)
    a = np.maximum(rng.randn(*shape), 0).astype(np.float32)          # post-ReLU features: non-negative, many zeros
    b = np.maximum(rng.randn(*shape), 0).astype(np.float32)
    w = rng.uniform(-0.25, 1.0, shape[3]).astype(np.float32)
    return a, b, w


# ------------------------------------------------------------------------------------------------- oracle premises
@pytest.mark.parametrize("shape", [(1, 1, 1, 64), (3, 5, 7, 64), (2, 3, 3, 512), (2, 2, 2, 4)])
def test_oracle_agrees_with_the_packages_formulation(shape):
    a, b, w = _maps(shape)
    got, scale = O.layer(a, b, w)
    alt = O.layer_conv_form(a, b, w)
    # two float64 evaluations of one expression: a few roundings per term, C + H W additions per chain
    assert (np.abs(got - alt) <= 1e-13 * scale).all() and (scale >= np.abs(got)).all() and (scale > 0).all()
    zero, _ = O.layer(a, a, w)
    assert (zero == 0.0).all()
    back, _ = O.layer(b, a, w)
    assert np.array_equal(got, back)
    ones, ones_scale = O.layer(a, b, np.ones(shape[3]))
    assert np.array_equal(ones, ones_scale)


def test_oracle_preprocess_and_constants():
    assert O.SHIFT[0] == float(np.float32(-.030)) and O.SHIFT[0] != -.030 and O.SCALE[2] == float(np.float32(.450))
    u8 = np.array([[[[0, 128, 255]]]], dtype=np.uint8)                                       # one B,G,R pixel
    out = O.preprocess(u8, "bgr_hwc")
    assert out.shape == (1, 1, 1, 4) and out.dtype == np.float32 and out[0, 0, 0, 3] == 0
    want = [np.float32((v - s) / c) for v, s, c in zip((1.0, 128 / 255.0 * 2.0 - 1.0, -1.0), O.SHIFT, O.SCALE)]
    assert out[0, 0, 0, :3].tolist() == want
    f = np.array([0.25, -0.5, 1.0], dtype=np.float32).reshape(1, 3, 1, 1)
    assert O.preprocess(f, "nchw")[0, 0, 0, :3].tolist() == [np.float32((v - s) / c) for v, s, c in zip(f.ravel().astype(np.float64), O.SHIFT, O.SCALE)]


def test_generated_weights_keep_the_relus_alive():
    sd = O.vgg16_state_dict(0)
    rng = np.random.RandomState(2)
    taps = O.trunk(O.preprocess(rng.uniform(-1, 1, (1, 3, 32, 32)).astype(np.float32), "nchw"), sd)
    assert [t.shape for t in taps] == [(1, 32, 32, 64), (1, 16, 16, 128), (1, 8, 8, 256), (1, 4, 4, 512), (1, 2, 2, 512)]
    for t in taps:
        assert 0.2 < (t > 0).mean() < 0.8 and np.isfinite(t).all()
    lin = O.lin_vectors(O.lin_state_dict(1))
    assert all(w.min() < 0 < w.max() and w.min() >= -0.25 and w.max() <= 1.0 for w in lin)


# ------------------------------------------------------------------------------------------------- loaders
def test_vgg16_key_mapping_and_refusals():
    from mmhand_amd import lpips
    sd = O.vgg16_state_dict(0)
    net = lpips.Vgg16Lpips(device="cpu").load_state_dict(sd)
    assert sorted(net.convs) == [n for n, _, _ in O.CONVS]
    w, b = net.convs[0]
    assert tuple(w.shape) == (3, 3, 4, 64) and tuple(b.shape) == (64,) and (w[:, :, 3] == 0).all()
    assert torch.equal(w[:, :, :3], sd["features.0.weight"].permute(2, 3, 1, 0))
    assert tuple(net.convs[28][0].shape) == (3, 3, 512, 512)
    # module. prefix, classifier.* and unrelated keys are ignored
    noisy = OrderedDict(("module." + k, v) for k, v in sd.items())
    noisy["module.classifier.0.weight"] = torch.zeros(2, 2)
    noisy["module.scaling_layer.shift"] = torch.zeros(1, 3, 1, 1)
    other = lpips.Vgg16Lpips(device="cpu").load_state_dict(noisy)
    assert all(torch.equal(other.convs[n][0], net.convs[n][0]) and torch.equal(other.convs[n][1], net.convs[n][1]) for n in net.convs)
    # the slice layout: net.slice{K}.{N}
    slices = {0: 1, 2: 1, 5: 2, 7: 2, 10: 3, 12: 3, 14: 3, 17: 4, 19: 4, 21: 4, 24: 5, 26: 5, 28: 5}
    sl = OrderedDict((re.sub(r"features\.(\d+)", lambda m: f"net.slice{slices[int(m.group(1))]}.{m.group(1)}", k), v)
                     for k, v in sd.items())
    assert "net.slice3.14.bias" in sl
    third = lpips.Vgg16Lpips(device="cpu").load_state_dict(sl)
    assert all(torch.equal(third.convs[n][0], net.convs[n][0]) for n in net.convs)
    assert set(lpips.map_keys(sl)) == set(sd)
    wrong = OrderedDict(sl)
    wrong["net.slice2.14.weight"] = wrong.pop("net.slice3.14.weight")
    with pytest.raises(ValueError, match="slice"):
        lpips.Vgg16Lpips(device="cpu").load_state_dict(wrong)
    # a missing key is named
    short = OrderedDict(sd)
    del short["features.19.bias"]
    with pytest.raises(KeyError, match=r"features\.19\.bias"):
        lpips.Vgg16Lpips(device="cpu").load_state_dict(short)
    # a 19-layer file: convolutions where VGG-16 has none
    v19 = OrderedDict(sd)
    for n in (16, 23, 25, 30, 32, 34):
        v19[f"features.{n}.weight"], v19[f"features.{n}.bias"] = torch.zeros(512, 512, 3, 3), torch.zeros(512)
    with pytest.raises(ValueError, match="19-layer"):
        lpips.Vgg16Lpips(device="cpu").load_state_dict(v19)
    # a width that is not VGG-16's
    thin = OrderedDict(sd)
    thin["features.5.weight"] = torch.zeros(96, 64, 3, 3)
    with pytest.raises(ValueError, match=r"features\.5\.weight"):
        lpips.Vgg16Lpips(device="cpu").load_state_dict(thin)
    with pytest.raises(AssertionError):
        lpips.Vgg16Lpips(device="cpu").forward_taps(torch.zeros(1, 16, 16, 4))              # nothing loaded


def test_load_lin(tmp_path):
    from mmhand_amd import lpips
    uni = lpips.load_lin("uniform")
    assert [tuple(w.shape) for w in uni] == [(c,) for c in O.WIDTHS] and all((w == 1).all() and w.dtype == torch.float32 for w in uni)
    sd = O.lin_state_dict(1)
    path = os.path.join(tmp_path, "lin.pth")
    torch.save(sd, path)
    got = lpips.load_lin(path)
    assert all(torch.equal(g, sd[f"lin{l}.model.1.weight"].reshape(-1)) for l, g in enumerate(got))
    full = OrderedDict((k.replace("lin", "lins.", 1), v) for k, v in sd.items())            # a whole LPIPS state dict's names
    assert "lins.3.model.1.weight" in full
    assert all(torch.equal(a, b) for a, b in zip(lpips.load_lin(full), got))
    short = OrderedDict(sd)
    del short["lin2.model.1.weight"]
    with pytest.raises(KeyError, match=r"lin2\.model\.1\.weight"):
        lpips.load_lin(short)
    alex = OrderedDict(sd)
    alex["lin1.model.1.weight"] = torch.zeros(1, 192, 1, 1)                                  # AlexNet's second head
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight"):
        lpips.load_lin(alex)
    assert lpips.LpipsScorer.chunk_size(512, 512) < 64 <= lpips.LpipsScorer.chunk_size(256, 256)
    n = lpips.LpipsScorer.chunk_size(512, 512)
    assert n * 514 * 514 * 64 < 2 ** 30 <= (n + 1) * 514 * 514 * 64


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
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert name in declared and getattr(lib, name) is not None
        assert any(fnmatch.fnmatchcase(name, p.strip(";")) for p in patterns), name
        proto = re.search(r"(?:int|size_t) %s\((.*?)\);" % name, bare, re.S).group(1)
        assert len(L.SIGNATURES[name][1]) == len(proto.split(",")), name
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert f"({len(L.SIGNATURES)} entry points" in fh.read()
    with open(os.path.join(ROOT, "mmhand_amd", "csrc", "Makefile")) as fh:
        assert "lpips.hip" in fh.read()
    # refused shapes ask for no workspace (no device is touched)
    assert lib.mmh_lpips_layer_ws_bytes(2, 16, 16, 64) == 2 * 16 * 8         # 16 lanes per pixel: 16 pixels per visit, 16 workgroups
    for B, H, W, C in ((1, 4, 4, 6), (1, 4, 4, 516), (1, 4, 4, 0), (0, 4, 4, 64), (1, 0, 4, 64), (1, 4, 0, 64), (8, 1024, 1024, 256)):
        assert lib.mmh_lpips_layer_ws_bytes(B, H, W, C) == 0, (B, H, W, C)


def test_argument_parser():
    from mmhand_amd import evaluate
    p = evaluate.build_parser()
    a = p.parse_args(["--name", "x", "--dataroot", "d", "--dataset", "rhd"])
    assert a.lpips is None and a.lpips_lin is None and a.lpips_images is None and a.lpips_ref is None
    a = p.parse_args(["--lpips_images", "g", "--lpips_ref", "r", "--lpips", "v.pth", "--lpips_lin", "uniform"])
    assert a.lpips_images == "g" and a.lpips_ref == "r" and a.lpips_lin == "uniform" and a.dataset is None
    with pytest.raises(SystemExit):
        p.parse_args(["--lpips_images", "g", "--generated", "h"])                           # one source at a time
    for bad in (["--name", "x", "--dataroot", "d", "--dataset", "rhd", "--lpips", "v.pth"],                  # no --lpips_lin
                ["--name", "x", "--dataroot", "d", "--dataset", "rhd", "--lpips_lin", "uniform"],           # no --lpips
                ["--lpips_images", "g", "--lpips", "v.pth", "--lpips_lin", "uniform"],                       # no reference
                ["--lpips_images", "g", "--lpips_ref", "r", "--lpips", "v.pth"],
                ["--name", "x", "--dataroot", "d", "--dataset", "rhd", "--lpips", "v.pth", "--lpips_lin", "uniform", "--lpips_ref", "r"],
                ["--is_images", "g", "--inception", "w.pth", "--lpips", "v.pth", "--lpips_lin", "uniform"]):
        with pytest.raises(SystemExit) as e:
            evaluate.main(bad)
        assert e.value.code == 2, bad                                                        # the parser's own refusal
    assert set(evaluate.LPIPS_FLAGS) == {"lpips", "lpips_lin", "lpips_images", "lpips_ref"}
    assert not set(evaluate.LPIPS_FLAGS) & set(evaluate.FID_FLAGS + evaluate.IS_FLAGS + evaluate.PCK_FLAGS)
    help_text = p.format_help()
    for flag in evaluate.LPIPS_FLAGS:
        assert "--" + flag in help_text, flag
    assert "AlexNet" in evaluate.__doc__ and "--lpips_lin" in evaluate.__doc__


def test_evaluate_imports_nothing_of_lpips_without_its_flags():
    """a fresh interpreter: importing evaluate, building its parser and walking main() up to the first missing file leaves
    mmhand_amd.lpips unimported"""
    code = ("import sys\n"
            "from mmhand_amd import evaluate\n"
            "evaluate.build_parser().parse_args(['--name', 'x', '--dataroot', 'd', '--dataset', 'rhd'])\n"
            "try:\n"
            "    evaluate.main(['--name', 'no_such_checkpoint', '--dataroot', 'd', '--dataset', 'rhd'])\n"
            "except SystemExit as e:\n"
            "    assert 'no checkpoint' in str(e), e\n"
            "assert hasattr(evaluate, 'LPIPS_FLAGS')\n"
            "assert 'mmhand_amd.lpips' not in sys.modules, sorted(m for m in sys.modules if m.startswith('mmhand_amd'))\n"
            "print('clean')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("clean"), out.stderr[-2000:]
