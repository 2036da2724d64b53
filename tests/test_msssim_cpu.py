"""Host side of the multi-scale and hand-region modes of the image metrics (csrc/metrics.hip: mmh_ms_ssim,
mmh_image_metrics_masked; mmhand_amd/metrics.py; evaluate --ms_ssim / --hand_region): the oracle of tests/_msssim_oracle.py
against an independent torch formulation, the premises its bounds rest on (exact pooling on the grid, conditioning of the test
pairs, sensitivity to every planted fault) for exactly the cases the device runs, and the argument checks, file formats and
ABI.  No GPU needed."""
import csv
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _metrics_oracle as M
from tests import _msssim_oracle as O
from tests import _render_oracle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mmh_image_metrics_masked_ws_bytes", "mmh_image_metrics_masked", "mmh_ms_ssim_ws_bytes", "mmh_ms_ssim")


# ------------------------------------------------------------------------------------------------- (i) oracle against torch
def _torch_ms_ssim(a01, b01, window, weights):
    """MS-SSIM with torch's own operators in float64: F.conv2d of the five moment planes with the 2-D window, no padding, and
    F.avg_pool2d(x, 2, padding=(H % 2, W % 2))"""
    a, b = torch.from_numpy(a01), torch.from_numpy(b01)
    B, C = a.shape[:2]
    win = torch.from_numpy(M.window2d(window))[None, None]
    vals = []
    for l in range(len(weights)):
        H, W = a.shape[2:]
        mu1, mu2, e11, e22, e12 = (F.conv2d(p.reshape(B * C, 1, H, W), win).reshape(B, C, H - window + 1, W - window + 1)
                                   for p in (a, b, a * a, b * b, a * b))
        s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
        cs = (2 * s12 + O.C2) / (s1 + s2 + O.C2)
        lum = (2 * mu1 * mu2 + O.C1) / (mu1 * mu1 + mu2 * mu2 + O.C1)
        vals.append((cs * lum if l == len(weights) - 1 else cs).mean(dim=(2, 3)))
        a, b = (F.avg_pool2d(x, 2, padding=(H % 2, W % 2)) for x in (a, b))
    scales = torch.stack(vals, 2)
    ms = torch.prod(scales.clamp(min=0) ** torch.tensor(weights, dtype=torch.float64), dim=2).mean(dim=1)
    return ms.numpy(), scales.numpy()


@pytest.mark.parametrize("H,W,window,levels", [(45, 38, 5, 3), (41, 37, 3, 4), (48, 64, 11, 2), (67, 45, 5, 2)],
                         ids=["odd_x_even", "odd_x_odd", "even_x_even", "probe_shape"])
def test_oracle_equals_torch_formulation(H, W, window, levels):
    a, b = O.perturbed_pair((2, 2, H, W), 3)
    a01, b01 = M.mapped(a, "pm1"), M.mapped(b, "pm1")
    w = O.MS_WEIGHTS[:levels]
    ms, scales = O.ms_ssim(a01, b01, window, w)
    tms, tscales = _torch_ms_ssim(a01, b01, window, w)
    assert scales.shape == tscales.shape == (2, 2, levels)
    assert np.abs(scales - tscales).max() <= 1e-12 and np.abs(ms - tms).max() <= 1e-12, (scales - tscales, ms - tms)


def test_oracle_maps_are_the_metrics_oracle_map():
    """`maps` repeats _metrics_oracle.ssim_map's sums: the same map bit for bit, and cs = 1 exactly where ssim is"""
    case = M.single_probe_case("33x33", 5)
    a01, b01 = M.mapped(case["a"], "pm1"), M.mapped(case["b"], "pm1")
    ssim, cs = O.maps(a01, b01, 5)
    assert np.array_equal(ssim, M.ssim_map(a01, b01, 5))
    assert np.array_equal(cs == 1.0, ssim == 1.0) and (cs == 1.0).any() and (cs != 1.0).any()


def test_masked_oracle_with_all_ones_is_the_whole_image():
    a, b = M.grid_pair((2, 3, 20, 17), 1)
    a01, b01 = M.mapped(a, "pm1"), M.mapped(b, "pm1")
    got = O.masked(a01, b01, np.ones((2, 20, 17), np.uint8), 5)
    _, _, l1, mse = M.sums(a01, b01)
    assert np.array_equal(got["l1_hand"], l1) and np.array_equal(got["mse_hand"], mse) and np.all(got["count"] == 340)
    none = O.masked(a01, b01, np.zeros((2, 20, 17), np.uint8), 5)
    assert np.isnan(none["ssim_hand"]).all() and np.isnan(none["l1_hand"]).all() and np.all(none["count"] == 0)


# ------------------------------------------------------------------------------------------------- (ii) exact pooling
def test_fp32_pooling_is_exact_on_the_grid():
    """four pooled levels of grid values, odd and even sizes: fp32 in the kernel's order == float64, bit for bit, and every
    pooled value is a multiple of 2^-16"""
    x = M.mapped(M.from_grid(M.grid((2, 2, 161, 176), 1)), "pm1")
    x32, x64 = x.astype(np.float32), x
    for level in range(1, 5):
        x32, x64 = O.pool(x32, np.float32), O.pool(x64, np.float64)
        assert x32.dtype == np.float32 and x32.shape == x64.shape == (2, 2) + O.level_sizes(161, 176, 5)[level]
        assert np.array_equal(x32.astype(np.float64), x64)
        assert np.array_equal(x64 * 65536.0, np.rint(x64 * 65536.0))


def test_pooling_is_avg_pool2d_with_front_padding():
    x = M.mapped(M.from_grid(M.grid((1, 2, 7, 9), 2)), "pm1")
    assert np.array_equal(O.pool(x), F.avg_pool2d(torch.from_numpy(x), 2, padding=(1, 1)).numpy())
    assert O.pool(x)[0, 0, 0, 0] == x[0, 0, 0, 0] * 0.25                # one in-image pixel, divisor 4
    assert O.pool(x, fault="divisor")[0, 0, 0, 0] == x[0, 0, 0, 0]
    assert O.pool(x, fault="pad_side")[0, 0, 0, 0] == ((x[0, 0, 0, 0] + x[0, 0, 0, 1]) + (x[0, 0, 1, 0] + x[0, 0, 1, 1])) * 0.25


# ------------------------------------------------------------------------------------------------- (iii) conditioning
@pytest.mark.parametrize("name", list(O.WHOLE_CASES))
def test_whole_value_cases_are_well_conditioned(name):
    """the bound propagates 1e-6 per level through pow(v, w): every level value of the cases the device runs stays far from 0,
    and the case's shape obeys the min-side rule with its last level at least one window wide"""
    case = O.whole_case(name)
    assert case["scales"].min() >= O.FLOOR, case["scales"].min()
    assert np.all(case["ms"] > 0) and np.all(case["bound"] > 0) and np.all(case["bound"] < 2e-6), case["bound"]
    (B, C, H, W), w, L = case["shape"], case["window"], case["levels"]
    assert min(H, W) > (w - 1) * 2 ** (L - 1) and min(O.level_sizes(H, W, L)[-1]) >= w
    M.check_caps(M.mapped(case["a"], "pm1"), M.mapped(case["b"], "pm1"))     # on the grid


def test_five_level_case_is_the_smallest_five_level_shape_and_its_bound_is_1e_6():
    case = O.whole_case("five_levels")
    assert O.level_sizes(161, 176, 5) == [(161, 176), (81, 88), (41, 44), (21, 22), (11, 11)]
    assert min(case["shape"][2:]) == (11 - 1) * 16 + 1
    assert np.all(np.abs(case["bound"] - 1.0e-6) < 1e-7), case["bound"]


def test_many_case_has_more_partials_than_the_final_reduction_has_threads():
    (B, C, H, W), _, _ = O.WHOLE_CASES["many"]
    assert -(-H // M.MT) * -(-W // M.MT) > M.MTPB


# ------------------------------------------------------------------------------------------------- (iv) sensitivity
@pytest.mark.parametrize("name", list(O.WHOLE_CASES))
def test_whole_value_cases_see_every_planted_fault(name):
    case = O.whole_case(name)
    held = [f for f in O.MS_FAULTS if O.whole_fault_applies(name, case, f)]
    assert "same_windows" in held and "weights_reversed" in held
    for fault in held:
        effect = O.whole_fault_effect(case, fault)
        assert np.all(effect >= 10 * case["bound"]), (name, fault, effect / case["bound"])


@pytest.mark.parametrize("name", list(O.PROBE_SHAPES))
def test_probe_cases_see_every_planted_fault(name):
    case = O.probe_case(name)
    assert np.all(case["affected"] >= 1), "every probe reaches every level"
    for fault in ("pad_side", "divisor", "same_windows", "cs_last"):
        applies, bars = O.probe_fault_applies(case, fault), O.probe_fault_effect(case, fault)
        assert applies.any(), fault
        assert np.all(bars[applies] >= 10), (name, fault, [(w, b) for w, b, a in zip(case["why"], bars, applies) if a and b < 10])


def test_seeds_are_the_first_that_satisfy_the_condition():
    """as _metrics_oracle.SEEDS: every seed in the tables is the first one at which the sensitivity tests above hold; the
    tables say 1 throughout, so the tests above are the proof"""
    assert set(O.WHOLE_SEEDS.values()) == set(O.PROBE_SEEDS.values()) == set(O.MASK_SEEDS.values()) == {1}


def test_every_fault_is_held_by_some_case():
    held = set()
    for name in O.WHOLE_CASES:
        held |= {f for f in O.MS_FAULTS if O.whole_fault_applies(name, O.whole_case(name), f)}
    for name in O.PROBE_SHAPES:
        held |= {f for f in O.MS_FAULTS if f != "weights_reversed" and O.probe_fault_applies(O.probe_case(name), f).any()}
    assert held == set(O.MS_FAULTS)


@pytest.mark.parametrize("name,window", list(O.MASK_SEEDS))
def test_one_pixel_masks_see_a_shifted_mask(name, window):
    case = O.one_pixel_case(name, window)
    assert np.all(case["ref"]["count"] == 1)
    for fault in O.MASK_FAULTS:
        effect = O.mask_fault_effect(case, fault)
        assert np.all(effect >= 10 * O.LEVEL_BAR), (name, window, fault, effect)
    # the masked value IS the map's pixel
    a01, b01 = M.mapped(case["a"], "pm1"), M.mapped(case["b"], "pm1")
    pos, _ = O.one_pixel_masks(name, window)
    m = M.ssim_map(a01, b01, window)
    assert np.array_equal(case["ref"]["ssim_hand"], np.array([m[i, 0, y, x] for i, (y, x, _) in enumerate(pos)]))


# ------------------------------------------------------------------------------------------------- (v) host-side checks
def test_hand_mask_rule_is_the_render_oracle_coverage():
    """hand_mask renders with z = 0 and bg = 255 and takes lane 0 < 0: the oracle stores exactly -1 under a bone and +1 elsewhere"""
    xyz = np.concatenate([R.random_joints(2, 64, 48, 7), R.hand_placed()])
    xyz[..., 2] = 0.0
    for radius in (0.0, 3.5, 10.0):
        depth, counts = R.render(xyz, 64, 48, radius, bg=255.0, counts=True)
        assert set(np.unique(depth)) <= {-1.0, 1.0}
        assert np.array_equal(depth < 0, counts > 0)
        assert (counts > 0).any() and (counts == 0).any()


@pytest.fixture(scope="module")
def L():
    from mmhand_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mmhand_amd", "csrc")])
    lib.load()
    return lib


def test_header_signatures_and_readme_count(L):
    with open(os.path.join(ROOT, "include", "mmhand_hip.h")) as fh:
        header = fh.read()
    declared = set(re.findall(r"^(?:int|size_t|int64_t|const char\*)\s+(mmh_\w+)\(", header, re.M))
    assert declared == set(L.SIGNATURES), declared ^ set(L.SIGNATURES)
    lib = L.load()
    for name in NEW:
        assert name in declared and getattr(lib, name) is not None
        proto = re.search(r"(?:int|size_t) %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(L.SIGNATURES[name][1]) == len(proto.split(",")), name
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert f"({len(L.SIGNATURES)} entry points" in fh.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        text = fh.read()
    assert all(f"`{n}`" in text for n in ("mmh_image_metrics_masked", "mmh_ms_ssim"))
    doc = header[header.index("multi-scale SSIM"):header.index("size_t mmh_ms_ssim_ws_bytes")]
    assert "avg_pool2d(x, 2, padding=(H % 2, W % 2))" in doc and "(window - 1) * 2^(L - 1)" in doc and "* 0.25f" in doc


def _src(L, ptr=16):
    return L.ImageSrc(ptr, 0, 0.5, 0.5, 3 * 176 * 176, 176 * 176, 176, 1)


def test_workspaces_and_refused_shapes_without_gpu(L):
    l = L.load()
    f, g = l.mmh_ms_ssim_ws_bytes, l.mmh_image_metrics_masked_ws_bytes
    assert g(2, 3, 67, 45, 11) == 2 * 3 * 6 * 7 * 8 and g(2, 3, 67, 45, 10) == 0 and g(0, 3, 67, 45, 11) == 0
    # 67 x 45 -> 34 x 23: 6 + 2 tiles of two float64 per plane, then the 34 x 23 pair in fp32
    assert f(2, 1, 67, 45, 5, 2) == 2 * (6 + 2) * 2 * 8 + 2 * 2 * 34 * 23 * 4
    assert f(2, 1, 67, 45, 5, 1) == 2 * 6 * 2 * 8
    # the min-side rule: min(H, W) > (window - 1) * 2^(L - 1)
    assert f(1, 3, 161, 176, 11, 5) > 0 and f(1, 3, 160, 176, 11, 5) == 0 and f(1, 3, 176, 160, 11, 5) == 0
    assert f(1, 1, 5, 6, 3, 2) > 0 and f(1, 1, 4, 6, 3, 2) == 0 and f(1, 1, 3, 3, 3, 1) > 0 and f(1, 1, 2, 3, 3, 1) == 0
    assert f(1, 3, 256, 256, 11, 0) == 0 and f(1, 3, 256, 256, 11, 6) == 0 and f(1, 3, 256, 256, 10, 5) == 0
    assert f(0, 3, 256, 256, 11, 5) == 0 and f(1, 3, 1 << 17, 1 << 17, 11, 5) == 0

    from mmhand_amd.metrics import gaussian_taps
    taps = gaussian_taps(11).ctypes.data_as(ctypes.c_void_p)
    w = np.array(O.MS_WEIGHTS)
    a, b = _src(L), _src(L)

    def ms(H=176, W=176, levels=5, weights=w, window=11, ws=16, ws_bytes=1 << 30, scales=16):
        return l.mmh_ms_ssim(ctypes.byref(a), ctypes.byref(b), 1, 3, H, W, window, taps, 1e-4, 9e-4, levels,
                             weights.ctypes.data_as(ctypes.c_void_p) if weights is not None else None, ws, ws_bytes, scales, 16, None)

    def refused(msg, **kw):
        assert ms(**kw) != 0
        assert msg in l.mmh_last_error().decode(), l.mmh_last_error()

    refused("(window - 1) * 2^(levels - 1)", H=160)
    refused("(window - 1) * 2^(levels - 1)", W=33)
    refused("levels", levels=6)
    refused("levels", levels=0)
    refused("weight 1", weights=np.array([0.1, 0.0, 0.1, 0.1, 0.1]))
    refused("weight 4", weights=np.array([0.1, 0.1, 0.1, 0.1, float("nan")]))
    refused("NULL", weights=None)
    refused("NULL", scales=None)
    refused("NULL", ws=None)
    refused("window", window=10)
    refused("workspace", ws_bytes=f(1, 3, 176, 176, 11, 5) - 1)
    refused("aligned", ws=20)

    def masked(mask=16, ws_bytes=1 << 30, window=11, H=176):
        return l.mmh_image_metrics_masked(ctypes.byref(a), ctypes.byref(b), mask, 176 * 176, 176, 1, 1, 3, H, 176, window, taps,
                                          1e-4, 9e-4, 16, ws_bytes, 16, None)

    for kw, msg in ((dict(mask=None), "NULL mask"), (dict(ws_bytes=8), "workspace"), (dict(window=4), "window"),
                    (dict(H=0), "bad shape")):
        assert masked(**kw) != 0
        assert msg in l.mmh_last_error().decode() and "mmh_image_metrics_masked" in l.mmh_last_error().decode()


def test_python_argument_checks():
    from mmhand_amd import metrics
    assert metrics.MS_WEIGHTS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) == O.MS_WEIGHTS
    assert metrics.ms_ssim_min_side(11, 5) == 160 and metrics.ms_ssim_min_side(3, 2) == 4
    x = torch.zeros((1, 3, 176, 176))
    with pytest.raises(ValueError, match="CUDA"):
        metrics.ms_ssim(x, x)
    with pytest.raises(ValueError, match="CUDA"):
        metrics.image_metrics(x, x, mask=torch.ones((1, 176, 176), dtype=torch.bool))
    with pytest.raises(ValueError, match="float64 CUDA"):
        metrics.hand_mask(torch.zeros((1, 21, 2), dtype=torch.float64), (8, 8), 1.0)
    with pytest.raises(ValueError):
        metrics.QualityMeter(window=8, ms_ssim=True)


def test_quality_meter_default_is_what_it_was():
    from mmhand_amd.metrics import QualityMeter
    assert QualityMeter.COLUMNS == ("ssim", "l1", "mse", "psnr")
    plain = QualityMeter()
    assert plain.columns == QualityMeter.COLUMNS and not plain.ms_ssim and not plain.hand
    plain._batches.append((torch.tensor([[0.5, 0.1, 0.01, 20.0], [1.0, 0.0, 0.0, float("inf")]], dtype=torch.float64), None, None))
    res = plain.result()
    assert res["rows"] == [{"ssim": 0.5, "l1": 0.1, "mse": 0.01, "psnr": 20.0}, {"ssim": 1.0, "l1": 0.0, "mse": 0.0, "psnr": float("inf")}]
    assert res["summary"] == {"SSIM_avg": 0.75, "SSIM_std": 0.25, "L1_avg": 0.05, "PSNR_avg": 20.0, "n": 2}
    with pytest.raises(ValueError, match="mask"):
        plain.feed(None, None, mask=torch.ones((1, 2, 2)))
    with pytest.raises(ValueError, match="mask"):
        QualityMeter(hand=True).feed(None, None)


def _stub_meter(ms, hand):
    """a QualityMeter of three images whose values were 'read back' already: image 1's mask is empty"""
    from mmhand_amd.metrics import QualityMeter
    meter = QualityMeter("pm1", 11, ms_ssim=ms, hand=hand)
    nan = float("nan")
    cols = {"ssim": [0.5, 0.7, 0.9], "l1": [0.1, 0.2, 0.3], "mse": [0.01, 0.04, 0.09], "psnr": [20.0, 13.98, 10.46],
            "ssim_hand": [0.25, nan, 0.75], "l1_hand": [0.2, nan, 0.4], "mse_hand": [0.1, nan, 0.0],
            "psnr_hand": [10.0, nan, float("inf")], "mask_count": [100.0, 0.0, 300.0], "ms_ssim": [0.6, 0.8, 1.0]}
    paths = [{"target": f"d/t{i}.png", "source": f"d/s{i}.png"} for i in range(3)]
    meter._batches.append((torch.tensor([cols[k] for k in meter.columns], dtype=torch.float64).T.contiguous(), paths,
                           1000 if hand else None))
    meter.hand_radius = 6.875
    return meter


@pytest.mark.parametrize("ms,hand", [(False, False), (True, False), (False, True), (True, True)])
def test_json_and_csv_keys_with_and_without_the_flags(tmp_path, monkeypatch, ms, hand):
    from mmhand_amd import evaluate
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)
    seen = {}

    def score(args, dev):
        seen["args"] = args
        return _stub_meter(args.ms_ssim, args.hand_region), {}, None, None, None, None, None

    monkeypatch.setattr(evaluate, "_score_directory", score)
    out, rows_csv = tmp_path / "r.json", tmp_path / "r.csv"
    argv = ["--generated", str(tmp_path), "--dataroot", str(tmp_path), "--dataset", "rhd", "--results_json", str(out),
            "--per_image_csv", str(rows_csv)] + (["--ms_ssim"] if ms else []) + (["--hand_region"] if hand else [])
    evaluate.main(argv)
    res = json.load(open(out))
    base = ["SSIM_avg", "SSIM_std", "L1_avg", "PSNR_avg", "n"]
    want = base + (["MS_SSIM_avg", "MS_SSIM_std"] if ms else []) + \
        (["SSIM_hand_avg", "SSIM_hand_std", "L1_hand_avg", "PSNR_hand_avg", "hand_fraction_avg", "n_hand"] if hand else []) + \
        (["ms_weights"] if ms else []) + (["hand_radius"] if hand else [])
    assert list(res["summary"]) == want
    assert ("ms_ssim" in res["options"]) == ms and ("hand_region" in res["options"]) == hand == ("hand_radius" in res["options"])
    header = next(csv.reader(open(rows_csv)))
    assert header == ["target", "source", "ssim", "l1", "psnr"] + (["ms_ssim"] if ms else []) + \
        (["ssim_hand", "l1_hand", "psnr_hand", "hand_fraction"] if hand else [])
    s = res["summary"]
    if ms:
        assert s["MS_SSIM_avg"] == pytest.approx(0.8) and s["ms_weights"] == list(O.MS_WEIGHTS)
    if hand:        # over the two images with a non-empty mask; PSNR over the finite one
        assert s["n_hand"] == 2 and s["SSIM_hand_avg"] == 0.5 and s["SSIM_hand_std"] == 0.25 and s["L1_hand_avg"] == pytest.approx(0.3)
        assert s["PSNR_hand_avg"] == 10.0 and s["hand_fraction_avg"] == pytest.approx(0.2) and s["hand_radius"] == 6.875
    if not ms and not hand:
        assert res == {"summary": {"SSIM_avg": pytest.approx(0.7), "SSIM_std": s["SSIM_std"], "L1_avg": pytest.approx(0.2),
                                   "PSNR_avg": s["PSNR_avg"], "n": 3},
                       "options": res["options"], "generator": None, "domain": "[0, 1]: generator output (x + 1) / 2, PNG pixels u8 / 255"}
        assert not set(res["options"]) & set(evaluate.REGION_FLAGS)


def test_cli_argument_checks(tmp_path, capsys):
    from mmhand_amd import evaluate
    base = ["--generated", str(tmp_path), "--dataroot", str(tmp_path), "--dataset", "rhd"]
    for extra, msg in ((["--hand_radius", "5"], "--hand_radius belongs to --hand_region"),
                       (["--hand_region", "--hand_radius", "-1"], "--hand_radius must be finite and >= 0"),
                       (["--hand_region", "--hand_radius", "nan"], "--hand_radius must be finite and >= 0")):
        with pytest.raises(SystemExit) as e:
            evaluate.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err
    for flag in ("--ms_ssim", "--hand_region"):
        with pytest.raises(SystemExit) as e:
            evaluate.main(["--is_images", str(tmp_path), "--inception", "x.pth", flag])
        assert e.value.code == 2 and "with --name or --generated only" in capsys.readouterr().err
    help_text = " ".join(evaluate.build_parser().format_help().split())
    assert "10 * H / 256" in help_text and "gaps in the palm between the metacarpals" in help_text and "larger radius closes them" in help_text
    assert "mask-SSIM" in evaluate.__doc__ and "multiplies both images by the mask" in evaluate.__doc__


def test_ms_ssim_size_rule_ends_the_run_before_scoring():
    from types import SimpleNamespace
    from mmhand_amd import evaluate
    args = SimpleNamespace(ms_ssim=True, window=11, hand_radius=None)
    with pytest.raises(SystemExit) as e:
        evaluate._check_ms_size(args, SimpleNamespace(out_size=160, image_target=[]))
    assert "(window - 1) * 2^(levels - 1) = 160" in str(e.value.code) and "160 x 160" in str(e.value.code)
    evaluate._check_ms_size(args, SimpleNamespace(out_size=161, image_target=[]))
    evaluate._check_ms_size(SimpleNamespace(ms_ssim=False, window=11), SimpleNamespace(out_size=32, image_target=[]))
    assert evaluate.hand_radius(args, 256) == 10.0 and evaluate.hand_radius(args, 176) == 6.875
    assert evaluate.hand_radius(SimpleNamespace(hand_radius=3.0), 176) == 3.0
