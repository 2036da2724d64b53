"""Host side of the image quality metrics (mmhand_amd/metrics.py, mmhand_amd/evaluate.py, csrc/metrics.hip): argument
checks before any launch, the workspace plan, a spill-free build, the checkpoint -> Generator configuration inference and
the CLI's refusals.  No GPU needed."""
import ctypes
import json
import os
import re
import subprocess
from collections import OrderedDict

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def L():
    from mmhand_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mmhand_amd", "csrc")])
    lib.load()
    return lib


def _src(L, dtype=0, ptr=16):
    return L.ImageSrc(ptr, dtype, 0.5, 0.5, 3 * 64 * 64, 64 * 64, 64, 1)


def test_image_metrics_refuses_bad_arguments_without_gpu(L):
    from mmhand_amd.metrics import gaussian_taps
    l = L.load()
    taps = gaussian_taps(11)
    tp = taps.ctypes.data_as(ctypes.c_void_p)
    a, b = _src(L), _src(L)
    ws = l.mmh_image_metrics_ws_bytes(2, 3, 64, 64, 11)
    good = dict(B=2, C=3, H=64, W=64, window=11, taps=tp, ws=16, ws_bytes=ws, out=16)

    def call(a=a, b=b, **kw):
        k = dict(good, **kw)
        return l.mmh_image_metrics(ctypes.byref(a) if a is not None else None, ctypes.byref(b) if b is not None else None,
                                   k["B"], k["C"], k["H"], k["W"], k["window"], k["taps"], 1e-4, 9e-4, k["ws"],
                                   k["ws_bytes"], k["out"], None)

    def refused(msg, **kw):
        assert call(**kw) != 0
        assert msg in l.mmh_last_error().decode(), l.mmh_last_error()

    refused("NULL", a=None)
    refused("NULL", b=_src(L, ptr=0))
    refused("NULL", ws=None)
    refused("NULL", out=None)
    for w in (10, 1, 17, 2):
        refused("window", window=w)
    refused("bad shape", H=0)
    refused("bad shape", W=0)
    refused("bad shape", B=0)
    refused("bad shape", H=1 << 20, W=1 << 20)              # 2^30 tiles: more work-items than a grid dimension takes
    refused("unknown dtype", b=_src(L, dtype=4))
    refused("unknown dtype", a=_src(L, dtype=-1))
    refused("workspace", ws_bytes=ws - 1)
    refused("taps", taps=None)
    bad = np.array(taps) * 2
    refused("tap", taps=bad.astype(np.float32).ctypes.data_as(ctypes.c_void_p))


def test_workspace_is_a_pure_function_of_the_shape(L):
    l = L.load()
    f = l.mmh_image_metrics_ws_bytes
    assert f(64, 3, 256, 256, 11) == 64 * 3 * 64 * 3 * 8              # 8 x 8 tiles of 32 x 32, 3 float64 per tile
    assert f(1, 3, 67, 45, 11) == 3 * (3 * 2) * 3 * 8
    assert f(1, 3, 9, 9, 11) == f(1, 3, 9, 9, 3) == 3 * 3 * 8
    assert f(5, 1, 16, 16, 7) == 5 * 3 * 8
    assert all(f(2, 3, 40, 70, w) == f(2, 3, 40, 70, 11) for w in (3, 5, 7, 9, 13, 15))
    assert f(2, 3, 40, 70, 11) == f(2, 3, 40, 70, 11)
    assert f(2, 3, 40, 70, 10) == 0 and f(0, 3, 40, 70, 11) == 0 and f(2, 3, 0, 70, 11) == 0
    assert f(1, 3, 1 << 17, 1 << 17, 11) == 0 and f(1, 1, 1 << 16, 1 << 16, 11) > 0     # tiles * 256 < 2^32


def test_taps_are_the_reference_window():
    """pytorch_ssim.gaussian (:7-9) restated: exp in float64, fp32, divided by torch's fp32 sum"""
    import math
    from mmhand_amd.metrics import gaussian_taps
    for w in (3, 7, 11, 15):
        g = torch.Tensor([math.exp(-(x - w // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(w)])
        assert np.array_equal(gaussian_taps(w), (g / g.sum()).numpy())
        assert gaussian_taps(w).dtype == np.float32


def test_metrics_kernels_compile_without_scratch():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "--offload-arch=gfx950", "-Wall",
                          "-Wno-unused-function", "-Wno-inline-asm", "-Rpass-analysis=kernel-resource-usage", "-c",
                          "metrics.hip", "-o", os.devnull],
                         cwd=os.path.join(ROOT, "mmhand_amd", "csrc"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "warning:" not in out.stderr, out.stderr[-2000:]
    name, seen = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            seen[name] = int(m.group(1))
    tiles = [k for k in seen if "image_metrics_tile_kernel" in k]
    assert len(tiles) == 7 and any("image_metrics_final_kernel" in k for k in seen), seen
    assert all(v == 0 for v in seen.values()), seen


@pytest.mark.parametrize("norm", ["batch", "instance"])
def test_generator_config_from_reference_keys(norm):
    from mmhand_amd.evaluate import infer_generator_config
    keys = json.load(open(os.path.join(G, "keys.json")))[norm]
    assert infer_generator_config(keys["G"]) == (64, 9, norm, True)
    assert infer_generator_config(keys["G_nodrop"]) == (64, 9, norm, False)
    prefixed = OrderedDict(("module." + k, v) for k, v in keys["G_nodrop"].items())
    assert infer_generator_config(prefixed) == (64, 9, norm, False)


@pytest.mark.parametrize("norm", ["batch", "instance"])
def test_generator_config_from_a_built_generator(norm):
    from mmhand_amd.evaluate import infer_generator_config, strip_module
    from mmhand_amd.networks import Generator
    for drop in (False, True):
        sd = Generator([3, 42, 6], 3, 8, norm, drop, 2).state_dict()
        assert infer_generator_config(sd) == (8, 2, norm, drop)
        wrapped = OrderedDict(("module." + k, v) for k, v in sd.items())
        assert infer_generator_config(wrapped) == (8, 2, norm, drop)
        assert list(strip_module(wrapped)) == list(sd)
        Generator([3, 42, 6], 3, 8, norm, drop, 2).load_state_dict(strip_module(wrapped))
    with pytest.raises(ValueError):
        infer_generator_config({"model.1.weight": torch.zeros(1)})


def test_cli_refuses_even_window_and_missing_checkpoint(tmp_path, capsys):
    from mmhand_amd import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--name", "x", "--dataroot", str(tmp_path), "--dataset", "rhd", "--window", "10"])
    assert e.value.code == 2 and "--window 10" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--name", "nope", "--checkpoints_dir", str(tmp_path), "--dataroot", str(tmp_path), "--dataset", "rhd"])
    assert "no checkpoint" in str(e.value.code) and "latest_net_netG.pth" in str(e.value.code)
    with pytest.raises(SystemExit):
        evaluate.main(["--name", "x", "--generated", str(tmp_path), "--dataroot", str(tmp_path), "--dataset", "rhd"])
    help_text = evaluate.build_parser().format_help()
    assert "[0, 1]" in help_text and "(x + 1) / 2" in help_text and "u8 / 255" in help_text


def test_quality_meter_summary_keys():
    from mmhand_amd.metrics import QualityMeter
    rows = [{"ssim": 0.5, "l1": 0.1, "mse": 0.01, "psnr": 20.0}, {"ssim": 1.0, "l1": 0.0, "mse": 0.0, "psnr": float("inf")}]
    s = QualityMeter.summarize(rows)
    assert s == {"SSIM_avg": 0.75, "SSIM_std": 0.25, "L1_avg": 0.05, "PSNR_avg": 20.0, "n": 2}
    with pytest.raises(ValueError):
        QualityMeter(window=8)
