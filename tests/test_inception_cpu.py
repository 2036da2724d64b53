"""The Inception-score feature's host side: the test oracle (tests/_inception_oracle.py) against the outputs recorded from the
reference's own Inception-v3 and score code (tests/golden/inception.npz, inception_keys.json; tests/golden/make_inception.py),
the numpy resize model and the product's tables against PIL, the lookup table against torch, and the size, crop, group,
state-dict and argument arithmetic of mmhand_amd/inception.py and mmhand_amd/evaluate.py.  No GPU."""
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import _inception_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0
# (H, W) -> (resized height, resized width) for a target size: up, up at 75, down (more taps), tiny, the two non-square
# orientations, and a short side that already has the size
RESIZE_CASES = [((256, 256), 299, (299, 299)), ((64, 64), 75, (75, 75)), ((512, 512), 299, (299, 299)), ((8, 8), 75, (75, 75)),
                ((40, 50), 299, (299, 373)), ((50, 40), 299, (373, 299)), ((300, 299), 299, (300, 299))]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "inception.npz"))


@pytest.fixture(scope="module")
def sd():
    return O.state_dict(SEED)


def _rel_l1(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).sum() / np.abs(b).sum())


def test_state_dict_keys_and_shapes_are_the_references():
    with open(os.path.join(ROOT, "tests", "golden", "inception_keys.json")) as fh:
        keys = json.load(fh)["inception_v3"]
    assert O.keys_and_shapes(O.state_dict(SEED, aux=True)) == keys
    from mmhand_amd import inception
    names = {k for k, _ in keys}
    assert set(inception.expected_keys()) <= names and len(inception.CONVS) == 94
    # the product's table of the 94 convs is the reference's shapes
    shapes = dict((k, v) for k, v in keys)
    for n, (cin, cout, kh, kw, _, _, _) in inception.CONV_SPEC.items():
        assert shapes[n + ".conv.weight"] == [cout, cin, kh, kw], n


def test_oracle_forward_matches_the_reference_module(gold, sd):
    """pins the graph (branch order, paddings of the 1x7 / 7x1 pairs, pools) and the BatchNorm arithmetic"""
    a = O.forward(sd, O.net_inputs((2, 3, 75, 75), SEED)).numpy()
    b = O.forward(sd, O.net_inputs((1, 3, 107, 91), SEED, index=1)).numpy()
    assert a.shape == (2, 1000) and b.shape == (1, 1000)
    assert _rel_l1(a, gold["logits_a"]) < 1e-10 and _rel_l1(b, gold["logits_b"]) < 1e-10


def test_folded_batchnorm_is_the_unfolded_one(sd):
    import torch.nn.functional as F
    from mmhand_amd import inception
    n = "Mixed_6b.branch7x7_2"
    w, b = inception.fold_bn(sd[n + ".conv.weight"], *(sd[f"{n}.bn.{k}"] for k in inception.BN_KEYS))
    x = torch.from_numpy(O.net_inputs((1, 128, 5, 4), SEED, index=2))
    want = F.batch_norm(F.conv2d(x, sd[n + ".conv.weight"], None, 1, (0, 3)), sd[n + ".bn.running_mean"], sd[n + ".bn.running_var"],
                        sd[n + ".bn.weight"], sd[n + ".bn.bias"], False, 0.0, 0.001)
    got = F.conv2d(x, w, b, 1, (0, 3))
    assert w.dtype == torch.float64 and float((got - want).abs().max()) < 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("hw,size,resized", RESIZE_CASES)
def test_resize_models_equal_pil(hw, size, resized):
    from PIL import Image
    from mmhand_amd import inception
    H, W_ = hw
    assert O.resized(H, W_, size) == resized == inception.resize_size(H, W_, size)
    img = np.random.RandomState(H * 1000 + W_).randint(0, 256, size=(H, W_, 3), dtype=np.uint8)
    img[0, 0], img[-1, -1] = 255, 0
    want = np.asarray(Image.fromarray(img).resize((resized[1], resized[0]), Image.BILINEAR))
    assert np.array_equal(O.pil_resize(img, *resized), want)
    # the product's tables, applied with plain integer arithmetic
    out = img.astype(np.int64)
    for axis, n_out in ((1, resized[1]), (0, resized[0])):
        bounds, coef = inception.pil_bilinear_tables(out.shape[axis], n_out)
        assert bounds.dtype == np.int32 and coef.dtype == np.int32 and bounds.shape == (n_out, 2) and coef.shape[0] == n_out
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= out.shape[axis]).all() and (bounds[:, 1] <= coef.shape[1]).all()
        src = np.moveaxis(out, axis, 0)
        rows = []
        for j in range(n_out):
            acc = np.full(src.shape[1:], 1 << 21, dtype=np.int64)
            for t in range(bounds[j, 1]):
                acc = acc + src[bounds[j, 0] + t] * int(coef[j, t])
            rows.append(np.clip(acc >> 22, 0, 255))
        out = np.moveaxis(np.stack(rows), 0, axis)
    assert np.array_equal(out.astype(np.uint8), want)


def test_lookup_table_is_the_torch_chain_bit_for_bit():
    from mmhand_amd import inception
    lut = inception.normalize_lut()
    assert lut.shape == (3, 256) and lut.dtype == torch.float32
    # ToTensor (uint8 HWC -> float CHW / 255) and Normalize (sub_(mean[:, None, None]).div_(std[:, None, None])) on an image
    # holding every byte in every channel
    img = torch.arange(256, dtype=torch.int32).to(torch.uint8).reshape(16, 16, 1).repeat(1, 1, 3)
    t = img.permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    mean, std = torch.as_tensor(inception.MEAN, dtype=torch.float32), torch.as_tensor(inception.STD, dtype=torch.float32)
    t = t.sub_(mean[:, None, None]).div_(std[:, None, None])
    assert np.array_equal(lut.numpy().view(np.uint32), t.reshape(3, 256).numpy().view(np.uint32))
    assert np.array_equal(O.lut().view(np.uint32), lut.numpy().view(np.uint32))


def test_bytes_are_augs():
    x = np.concatenate([np.linspace(-1.2, 1.2, 4001), (np.arange(256) + 0.5) / 127.5 - 1.0]).astype(np.float32)
    t = torch.from_numpy(x)
    want = ((t * 0.5 + 0.5) * 255.0).round().clamp(0, 255).to(torch.uint8).numpy()      # aug.py:142
    assert np.array_equal(O.to_bytes(x), want) and want.min() == 0 and want.max() == 255


def test_size_crop_and_group_arithmetic():
    from mmhand_amd import inception as I
    assert I.resize_size(256, 256) == (299, 299) and I.resize_size(40, 50) == (299, 373) and I.resize_size(50, 40) == (373, 299)
    assert I.resize_size(480, 640) == (299, 398) and I.resize_size(641, 480) == (399, 299)        # int(): 398.67, 399.29
    assert [I.crop_offset(n) for n in (299, 300, 301, 302, 373, 398)] == [0, 0, 1, 2, 37, 50]     # round half to even
    assert I.crop_offset(76, 75) == 0 and I.crop_offset(78, 75) == 2
    t = I.PreprocessTables(40, 50, 299, device="cpu")
    assert (t.rh, t.rw, t.oh, t.ow, t.crop_y, t.crop_x) == (299, 373, 299, 299, 0, 37)
    assert t.hbounds.shape == (373, 2) and t.vbounds.shape == (299, 2) and t.lut.shape == (3, 256)
    assert I.group_bounds(70, 64) == [(0, 64), (64, 70)] and I.group_bounds(128, 64) == [(0, 64), (64, 128)]
    assert I.group_bounds(6, 4) == [(0, 4), (4, 6)] and I.group_bounds(3, 64) == [(0, 3)] and I.group_bounds(0, 64) == []
    with pytest.raises(ValueError):
        I.group_bounds(5, 0)


def test_oracle_score_against_the_reference(gold):
    kl, py, s = O.score(gold["is_logits"])
    assert kl.shape == (70,) and py.shape == (1000,) and abs(py.sum() - 1.0) < 1e-12
    assert abs(s - float(gold["is_f64"])) <= 1e-12 * s
    # the reference's own function rounds the softmax to fp32 before its float64 part
    assert abs(s - float(gold["is_ref"])) <= 1e-6 * s and s > 1.5
    # one image: exactly 1; identical rows: exactly 1
    assert O.score(gold["is_logits"][:1])[2] == 1.0
    assert abs(O.score(np.repeat(gold["is_logits"][:1], 5, 0))[2] - 1.0) < 1e-15
    avg, std, all_, n, kls = O.grouped(gold["is_logits"], 64)
    a, b = O.score(gold["is_logits"][:64])[2], O.score(gold["is_logits"][64:])[2]
    assert n == 2 and avg == np.mean([a, b]) and std == np.std([a, b]) and all_ == s and kls.shape == (70,)


def test_generated_weights_give_a_score_clearly_above_one(sd):
    """the images, weights and sizes of the device tests: the float64 score of the six images is not degenerate"""
    img = O.images(6, 64, 64, SEED)
    assert img.min() >= -1.0 and img.max() <= 1.0
    x = O.preprocess(np.ascontiguousarray(O.to_bytes(img).transpose(0, 2, 3, 1)), 75)
    assert x.shape == (6, 75, 75, 4) and not x[..., 3].any()
    logits = O.forward(sd, x[..., :3].transpose(0, 3, 1, 2)).numpy()
    s = O.score(logits)[2]
    print("float64 Inception score of the six test images on generated weights: %.4f" % s)
    assert 1.5 <= s <= 50.0
    bn = [v for k, v in sd.items() if k.endswith("running_var")]
    assert min(float(v.min()) for v in bn) >= 0.5 and max(float(v.max()) for v in bn) <= 1.5


def test_state_dict_key_handling(sd):
    """needs no device: the key checks run before anything is uploaded"""
    from mmhand_amd import inception as I
    net = I.InceptionV3(device="cpu")
    short = OrderedDict((k, v) for k, v in sd.items() if not k.startswith("Mixed_7c.branch_pool"))
    with pytest.raises(KeyError, match="Mixed_7c.branch_pool.conv.weight"):
        net.load_state_dict(short)
    with pytest.raises(KeyError, match="fc.bias"):
        net.load_state_dict(OrderedDict(("module." + k, v) for k, v in sd.items() if k != "fc.bias"))
    bad = OrderedDict(sd)
    bad["Mixed_6b.branch7x7_2.conv.weight"] = bad["Mixed_6b.branch7x7_2.conv.weight"].permute(0, 1, 3, 2)
    with pytest.raises(ValueError, match="Mixed_6b.branch7x7_2"):
        net.load_state_dict(bad)
    # "module." is stripped, AuxLogits.* and num_batches_tracked are accepted and ignored
    full = OrderedDict(("module." + k, v.float() if v.is_floating_point() else v) for k, v in O.state_dict(SEED, aux=True).items())
    net.load_state_dict(full)
    assert len(net.convs) == 94 and not any(k.startswith("AuxLogits") for k in net.convs)
    w, b = net.convs["Conv2d_1a_3x3"]
    assert tuple(w.shape) == (3, 3, 4, 32) and not w[:, :, 3].any() and w.dtype == torch.float32 and tuple(b.shape) == (32,)
    w, b = net.convs["Mixed_6b.branch7x7_2"]
    assert tuple(w.shape) == (1, 7, 128, 128)
    fw, fb = I.fold_bn(sd["Mixed_6b.branch7x7_2.conv.weight"].float(), *(sd[f"Mixed_6b.branch7x7_2.bn.{k}"].float() for k in I.BN_KEYS))
    assert np.array_equal(w.numpy(), fw.permute(2, 3, 1, 0).float().numpy()) and np.array_equal(b.numpy(), fb.float().numpy())
    assert tuple(net.fc[0].shape) == (2048, 1000) and np.array_equal(net.fc[0].numpy(), sd["fc.weight"].float().t().numpy())


def test_argument_parser():
    from mmhand_amd import evaluate
    p = evaluate.build_parser()
    a = p.parse_args(["--name", "x", "--dataroot", "d", "--dataset", "rhd"])
    assert a.inception is None and a.is_group == 64 and a.is_images is None
    a = p.parse_args(["--generated", "g", "--dataroot", "d", "--dataset", "stb", "--inception", "w.pth", "--is_group", "4"])
    assert a.inception == "w.pth" and a.is_group == 4
    a = p.parse_args(["--is_images", "dir", "--inception", "w.pth"])
    assert a.is_images == "dir" and a.dataset is None
    with pytest.raises(SystemExit):
        p.parse_args(["--is_images", "dir", "--generated", "g"])             # one source at a time
    with pytest.raises(SystemExit):
        evaluate.main(["--is_images", "dir"])                                 # no weights named
    with pytest.raises(SystemExit):
        evaluate.main(["--is_images", "dir", "--inception", "w.pth", "--is_group", "0"])
    with pytest.raises(SystemExit):
        evaluate.main(["--name", "x", "--dataroot", "d"])                     # every other mode still needs --dataset
    assert set(evaluate.IS_FLAGS) == {"inception", "is_group", "is_images"}
