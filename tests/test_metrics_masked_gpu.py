"""mmh_image_metrics_masked (csrc/metrics.hip: image_metrics_masked_kernel; mmhand_amd.metrics.image_metrics(mask=),
hand_mask) on the device against tests/_msssim_oracle.py, and evaluate --ms_ssim --hand_region end to end.

* the whole-image outputs equal image_metrics' bits for every mask, and an all-ones mask returns them as the masked outputs too;
* one-pixel masks read single pixels of the SSIM map - at corners, seams, ragged tiles, the column pairs and row groups of
  tests/_metrics_oracle.py's position lists - and hold them to the float64 map at 1e-6; L1 / MSE bit for bit on grid values;
* mask handling: one mask per image, empty masks, values other than 0 / 1, bool and uint8, sliced masks, C = 1 and 3, symmetry,
  more partials than the final reduction has threads;
* hand_mask equals the render oracle's coverage bit for bit;
* evaluate in both scoring modes at batch sizes 1 and 2, and its files without the flags."""
import csv
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import _metrics_oracle as M
from tests import _msssim_oracle as O
from tests import _render_oracle as R

pytestmark = pytest.mark.gpu
WHOLE = ("ssim", "l1", "mse", "psnr")
HAND = ("ssim_hand", "l1_hand", "mse_hand", "psnr_hand")


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    O.clear_caches()
    M.clear_caches()


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _host(m):
    return {k: v.cpu().numpy() for k, v in m.items()}


def _hashed_mask(shape, seed, share=0.3):
    from tests._hpe_oracle import hashed
    return (hashed(7200, int(np.prod(shape)), seed).reshape(shape) < 2 * share - 1).astype(np.uint8)


@pytest.mark.parametrize("values", ["grid", "off_grid"])
@pytest.mark.parametrize("window", [3, 11, 15])
def test_whole_image_outputs_are_image_metrics_bits(dev, window, values):
    """for an empty, a random and a full mask; off the grid too, where (a - b)^2 is not exact in float64 and the two kernels must
    form their sums with the same instructions"""
    from mmhand_amd.metrics import image_metrics
    from tests._hpe_oracle import hashed
    shape = (3, 3, 67, 45)
    if values == "grid":
        a, b = M.grid_pair(shape, 1)
    else:
        n = int(np.prod(shape))
        a = torch.from_numpy(hashed(7300, n, 1).reshape(shape).astype(np.float32))
        b = torch.from_numpy(hashed(7301, n, 1).reshape(shape).astype(np.float32))
    a, b = a.to(dev), b.to(dev)
    plain = _host(image_metrics(a, b, window=window))
    mask = np.stack([np.zeros((67, 45), np.uint8), _hashed_mask((67, 45), 2), np.ones((67, 45), np.uint8)])
    got = _host(image_metrics(a, b, window=window, mask=torch.from_numpy(mask).to(dev)))
    for k in WHOLE:
        assert np.array_equal(_bits(got[k]), _bits(plain[k])), (k, got[k], plain[k])
    assert got["mask_count"].tolist() == [0.0, float(mask[1].sum()), 67.0 * 45.0]
    for k, w in zip(HAND, WHOLE):
        assert np.isnan(got[k][0]), (k, got[k])
        assert _bits(got[k][2]) == _bits(plain[w][2]), (k, got[k][2], plain[w][2])       # all ones: the whole-image bits


@pytest.mark.parametrize("name,window", list(O.MASK_SEEDS))
def test_one_pixel_masks_read_the_map(dev, name, window):
    """ssim_hand of a one-pixel mask IS the SSIM map at that pixel: |got - float64 map| <= 1e-6 per position; the largest is
    printed.  l1_hand / mse_hand: the oracle's sum * (1.0 / (C * count)) bit for bit.  Measured on an MI355X, the largest per case:
    67 x 45: 1.3e-7 (w = 3), 1.4e-7 (5), 4.5e-7 (11, a corner), 4.3e-7 (15); 33 x 33: 1.8e-7, 2.9e-7, 1.5e-7, 3.5e-7."""
    from mmhand_amd.metrics import image_metrics
    case = O.one_pixel_case(name, window)
    got = _host(image_metrics(case["a"].to(dev), case["b"].to(dev), window=window, mask=torch.from_numpy(case["masks"]).to(dev)))
    err = np.abs(got["ssim_hand"] - case["ref"]["ssim_hand"])
    i = int(np.argmax(err))
    print(f"\n[{name}_w{window}] largest |ssim_hand - map| = {err[i]:.3e} at {case['why'][i]}")
    assert np.all(err <= O.LEVEL_BAR), [(case["why"][j], got["ssim_hand"][j], case["ref"]["ssim_hand"][j]) for j in np.nonzero(err > O.LEVEL_BAR)[0]]
    assert np.all(got["mask_count"] == 1.0)
    for k in ("l1_hand", "mse_hand"):
        assert np.array_equal(_bits(got[k]), _bits(case["ref"][k])), (k, got[k], case["ref"][k])
    assert np.array_equal(_bits(got["psnr_hand"]), _bits((-10.0 * torch.log10(torch.from_numpy(got["mse_hand"]).to(dev))).cpu().numpy()))


@pytest.mark.parametrize("Cc", [1, 3])
def test_masks_per_image_values_types_and_strides(dev, Cc):
    from mmhand_amd.metrics import image_metrics
    shape = (4, Cc, 67, 45)
    a, b = (t.to(dev) for t in M.grid_pair(shape, 2))
    a01, b01 = M.mapped(a, "pm1"), M.mapped(b, "pm1")
    mask = np.stack([_hashed_mask((67, 45), s) for s in (1, 2, 3, 4)])
    mask[1] = 0                                                         # an empty mask in the middle of the batch
    want = O.masked(a01, b01, mask, 5)
    got = _host(image_metrics(a, b, window=5, mask=torch.from_numpy(mask).to(dev)))
    keep = [0, 2, 3]
    assert np.array_equal(got["mask_count"], want["count"]) and got["mask_count"][1] == 0
    assert all(np.isnan(got[k][1]) for k in HAND)
    assert np.abs(got["ssim_hand"][keep] - want["ssim_hand"][keep]).max() <= O.LEVEL_BAR
    for k in ("l1_hand", "mse_hand"):
        assert np.array_equal(_bits(got[k][keep]), _bits(want[k][keep])), k
    # the other images do not see the empty one: each alone gives the batch's bits
    for i in keep:
        alone = _host(image_metrics(a[i:i + 1].clone(), b[i:i + 1].clone(), window=5, mask=torch.from_numpy(mask[i:i + 1]).to(dev)))
        assert all(_bits(alone[k][0]) == _bits(got[k][i]) for k in WHOLE + HAND + ("mask_count",))
    # any non-zero byte is inside; a bool mask; a sliced mask (every other row and column of a larger buffer)
    odd = torch.from_numpy(mask * np.array([255, 1, 2, 128], dtype=np.uint8)[:, None, None]).to(dev)
    big = torch.full((4, 134, 90), 1, dtype=torch.uint8, device=dev)
    big[:, ::2, ::2] = torch.from_numpy(mask).to(dev)
    sliced = big[:, ::2, ::2]
    assert not sliced.is_contiguous() and sliced.stride() == (134 * 90, 180, 2)
    for other in (odd, torch.from_numpy(mask.astype(bool)).to(dev), sliced):
        again = _host(image_metrics(a, b, window=5, mask=other))
        assert all(np.array_equal(_bits(again[k]), _bits(got[k])) for k in WHOLE + HAND + ("mask_count",))
    # symmetry in (a, b)
    ba = _host(image_metrics(b, a, window=5, mask=torch.from_numpy(mask).to(dev)))
    assert all(np.array_equal(_bits(ba[k]), _bits(got[k])) for k in WHOLE + HAND + ("mask_count",))
    with pytest.raises(ValueError, match="mask"):
        image_metrics(a, b, window=5, mask=torch.from_numpy(mask[:3]).to(dev))
    with pytest.raises(ValueError, match="mask"):
        image_metrics(a, b, window=5, mask=torch.from_numpy(mask).float().to(dev))


def test_more_partials_than_final_threads(dev):
    """_metrics_oracle.many_partials_case's shape: 65 channels x 4 tiles = 260 partials per image, a second trip of the masked
    final kernel's loop; masks that cover only channel 64's last tile (partials 256 .. 259) and only the first"""
    from mmhand_amd.metrics import image_metrics
    case = M.many_partials_case(2)
    B, Cc, H, W = case["shape"]
    a, b = case["a"].to(dev), case["b"].to(dev)
    mask = np.zeros((B, H, W), np.uint8)
    mask[0, 32, 32] = 1                 # the one-pixel tile
    mask[1, :32, :32] = 1               # the first tile
    want = O.masked(M.mapped(case["a"], "pm1"), M.mapped(case["b"], "pm1"), mask, case["window"])
    got = _host(image_metrics(a, b, window=case["window"], mask=torch.from_numpy(mask).to(dev)))
    plain = _host(image_metrics(a, b, window=case["window"]))
    assert all(np.array_equal(_bits(got[k]), _bits(plain[k])) for k in WHOLE)
    assert np.array_equal(got["mask_count"], want["count"]) and want["count"].tolist() == [1.0, 1024.0]
    # 65 channels' pixels per image: the per-pixel bar over C * count map values
    assert np.all(np.abs(got["ssim_hand"] - want["ssim_hand"]) <= O.LEVEL_BAR)
    for k in ("l1_hand", "mse_hand"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k


@pytest.mark.parametrize("radius", [0.0, 3.5, 10.0])
def test_hand_mask_is_the_render_oracle_coverage(dev, radius):
    from mmhand_amd.metrics import hand_mask
    # two hashed poses and the oracle's hand-placed one (a bone exactly on a pixel row, which radius 0 covers; non-finite joints)
    xyz = np.concatenate([R.random_joints(2, 64, 48, 7), R.hand_placed()])
    xyz[..., 2] = 0.0
    _, counts = R.render(xyz, 64, 48, radius, bg=255.0, counts=True)
    got = hand_mask(torch.from_numpy(np.ascontiguousarray(xyz[..., :2])).to(dev), (64, 48), radius)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 64, 48) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), (counts > 0).astype(np.uint8))
    assert 0 < int(got.sum()) < got.numel()


# ------------------------------------------------------------------------------------------------- evaluate, end to end
@pytest.fixture
def work_dir():
    """a scratch directory whose PATH does not contain "test" (pytest's tmp_path does; generic_dataset.py:116 keys on it)"""
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="mmh_ev_")
    assert "test" not in d
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _evaluate(argv):
    from mmhand_amd import evaluate
    random.seed(11)                  # the loader's source shuffle (generic_dataset.py:129) draws from Python's random
    return evaluate.main(argv)


def _count_calls(monkeypatch):
    from mmhand_amd import lib as L
    calls, real = {}, L.call

    def counting(name, *args):
        calls[name] = calls.get(name, 0) + 1
        return real(name, *args)

    monkeypatch.setattr(L, "call", counting)
    return calls


FLAG_KEYS = {"MS_SSIM_avg", "MS_SSIM_std", "ms_weights", "SSIM_hand_avg", "SSIM_hand_std", "L1_hand_avg", "PSNR_hand_avg",
             "hand_fraction_avg", "n_hand", "hand_radius"}
FLAG_COLS = ["ms_ssim", "ssim_hand", "l1_hand", "psnr_hand", "hand_fraction"]


def test_evaluate_ms_ssim_and_hand_region(dev, work_dir, monkeypatch):
    """176 x 176 images (the smallest side the five-level rule admits at window 11 is 161), a randomly initialised generator:
    generator and --generated mode, batch sizes 1 and 2, with and without the flags"""
    from tests._dataset_fixture import write_rhd
    from mmhand_amd import aug
    from mmhand_amd.metrics import hand_mask, image_metrics, ms_ssim
    from mmhand_amd.networks import Generator
    root = os.path.join(work_dir, "rhd")
    write_rhd(root, n=6, size=176)
    monkeypatch.chdir(work_dir)
    os.makedirs(os.path.join("checkpoints", "ev"))
    torch.manual_seed(3)
    torch.save(Generator([3, 42, 6], 3, 8, "batch", True, 2).state_dict(), os.path.join("checkpoints", "ev", "latest_net_netG.pth"))
    assert len(aug.main(["ev", root, "gen", "rhd", "0.5", "0"], ngf=8, n_blocks=2)) == 3
    calls = _count_calls(monkeypatch)
    for mode in (["--name", "ev"], ["--generated", "gen"]):
        base = mode + ["--dataroot", root, "--dataset", "rhd", "--augmentation_ratio", "0.5"]
        tag = mode[0].strip("-")
        calls.clear()
        plain = _evaluate(base + ["--batchSize", "2", "--results_json", f"{tag}_plain.json", "--per_image_csv", f"{tag}_plain.csv"])
        assert calls.get("mmh_image_metrics", 0) == 2 and "mmh_image_metrics_masked" not in calls and "mmh_ms_ssim" not in calls
        assert "mmh_render_pose_depth" not in calls
        js = json.load(open(f"{tag}_plain.json"))
        assert list(js["summary"]) == ["SSIM_avg", "SSIM_std", "L1_avg", "PSNR_avg", "n"] and js["summary"]["n"] == 3
        assert not {"ms_ssim", "hand_region", "hand_radius"} & set(js["options"])
        table = list(csv.reader(open(f"{tag}_plain.csv")))
        assert table[0] == ["target", "source", "ssim", "l1", "psnr"] and len(table) == 4
        runs = {}
        for bs in ("1", "2"):
            calls.clear()
            runs[bs] = _evaluate(base + ["--batchSize", bs, "--ms_ssim", "--hand_region", "--results_json", f"{tag}_{bs}.json",
                                         "--per_image_csv", f"{tag}_{bs}.csv"])
            n_batches = 3 if bs == "1" else 2
            assert calls.get("mmh_image_metrics_masked", 0) == n_batches == calls.get("mmh_ms_ssim", 0) and "mmh_image_metrics" not in calls
        rows = runs["2"]["rows"]
        assert [r["target"] for r in rows] == [r["target"] for r in runs["1"]["rows"]] == [r["target"] for r in plain["rows"]]
        for x, y, p in zip(rows, runs["1"]["rows"], plain["rows"]):
            assert x == y or all(x[k] == y[k] or (x[k] != x[k] and y[k] != y[k]) for k in x), (x, y)     # identical across batch sizes
            assert all(_bits(x[k]) == _bits(p[k]) for k in WHOLE), (x, p)                       # and the plain columns' bits
            assert 0.0 < x["hand_fraction"] < 1.0 and 0.0 < x["ms_ssim"] <= 1.0 and x["ssim_hand"] == x["ssim_hand"]
        js = json.load(open(f"{tag}_2.json"))
        assert FLAG_KEYS <= set(js["summary"]) and set(js["summary"]) - FLAG_KEYS == {"SSIM_avg", "SSIM_std", "L1_avg", "PSNR_avg", "n"}
        s = js["summary"]
        assert s["hand_radius"] == 10.0 * 176 / 256 and s["n_hand"] == 3 and s["ms_weights"] == list(O.MS_WEIGHTS)
        assert abs(s["MS_SSIM_avg"] - np.mean([r["ms_ssim"] for r in rows])) < 1e-12
        assert abs(s["SSIM_hand_avg"] - np.mean([r["ssim_hand"] for r in rows])) < 1e-12
        assert abs(s["hand_fraction_avg"] - np.mean([r["hand_fraction"] for r in rows])) < 1e-12
        assert js["options"]["ms_ssim"] is True and js["options"]["hand_region"] is True and js["options"]["hand_radius"] is None
        table = list(csv.reader(open(f"{tag}_2.csv")))
        assert table[0] == ["target", "source", "ssim", "l1", "psnr"] + FLAG_COLS and len(table) == 4
        assert [t[:5] for t in table] == list(csv.reader(open(f"{tag}_plain.csv")))
    # the directory mode's rows against the functions themselves: the PNG pair, the mask from the target's labels
    from PIL import Image
    from mmhand_amd.data import HandFolderLoader
    from mmhand_amd.evaluate import _opt, _pose_labels, build_parser
    args = build_parser().parse_args(["--generated", "gen", "--dataroot", root, "--dataset", "rhd", "--augmentation_ratio", "0.5"])
    loader = HandFolderLoader(_opt(args), device=dev)
    for r in rows:
        g = torch.from_numpy(np.array(Image.open(os.path.join("gen", *r["target"].split("/")[-2:])).convert("RGB"))[None, :, :, ::-1].copy())
        t = torch.from_numpy(np.array(Image.open(r["target"]).convert("RGB"))[None, :, :, ::-1].copy())
        uv, _ = _pose_labels(loader, [r["target"]], None)
        mask = hand_mask(torch.from_numpy(uv).to(dev), (176, 176), 10.0 * 176 / 256)
        m = _host(image_metrics(g.to(dev), t.to(dev), range="u8_bgr_hwc", mask=mask))
        assert m["ssim_hand"][0] == r["ssim_hand"] and m["l1_hand"][0] == r["l1_hand"] and m["mask_count"][0] == r["mask_count"]
        assert float(ms_ssim(g.to(dev), t.to(dev), range="u8_bgr_hwc")["ms_ssim"][0]) == r["ms_ssim"]
        want = O.masked(M.mapped(g, "u8_bgr_hwc"), M.mapped(t, "u8_bgr_hwc"), mask.cpu().numpy(), 11)
        assert abs(r["ssim_hand"] - want["ssim_hand"][0]) <= O.LEVEL_BAR and abs(r["l1_hand"] - want["l1_hand"][0]) <= 1e-13


def test_evaluate_ms_ssim_refuses_small_images_before_scoring(dev, work_dir, monkeypatch):
    from tests._dataset_fixture import write_rhd
    root = os.path.join(work_dir, "rhd")
    write_rhd(root, n=4, size=32)
    os.makedirs(os.path.join(work_dir, "gen"))
    monkeypatch.chdir(work_dir)
    calls = _count_calls(monkeypatch)
    with pytest.raises(SystemExit) as e:
        _evaluate(["--generated", "gen", "--dataroot", root, "--dataset", "rhd", "--augmentation_ratio", "0.5", "--ms_ssim"])
    assert "(window - 1) * 2^(levels - 1) = 160" in str(e.value.code) and "32 x 32" in str(e.value.code)
    assert not calls
