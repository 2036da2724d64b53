"""Image quality metrics on the device (csrc/metrics.hip through mmhand_amd/metrics.py and mmhand_amd/evaluate.py)
against float64: the reference's own SSIM in float64 (tests/golden/ssim.npz) and an in-test float64 restatement of it."""
import csv
import json
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-6

pytestmark = pytest.mark.gpu


def oracle(a01, b01, window=11):
    """pytorch_ssim._ssim (:17-37) in float64 with the reference's fp32 window (create_window: fp32 taps, fp32 outer
    product), per image; plus mean |a-b| and mean (a-b)^2.  a01, b01: [B,C,H,W] in [0, 1]."""
    from mmhand_amd.metrics import gaussian_taps
    a01, b01 = a01.double().cpu(), b01.double().cpu()
    g = torch.from_numpy(gaussian_taps(window)).unsqueeze(1)
    C = a01.shape[1]
    win = g.mm(g.t()).float().double().expand(C, 1, window, window).contiguous()

    def f(x):
        return F.conv2d(x, win, padding=window // 2, groups=C)

    mu1, mu2 = f(a01), f(b01)
    s1, s2, s12 = f(a01 * a01) - mu1 ** 2, f(b01 * b01) - mu2 ** 2, f(a01 * b01) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))
    d = a01 - b01
    return m.mean((1, 2, 3)).numpy(), d.abs().mean((1, 2, 3)).numpy(), (d * d).mean((1, 2, 3)).numpy()


def test_ssim_matches_reference_float64_golden(dev):
    from mmhand_amd.metrics import ssim
    from tests.ssim_cases import cases
    gold = np.load(os.path.join(ROOT, "tests", "golden", "ssim.npz"))
    names = list(gold["names"])
    worst = {}
    for name, a, b, w in cases():
        i = names.index(name)
        got = ssim(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), window=w).cpu().numpy()
        err = np.abs(got - gold["f64"][i]).max()
        worst[name] = err
        assert err <= BAR, (name, err, got, gold["f64"][i])
    print("worst |kernel - reference float64|: %.2e (%s)" % max((v, k) for k, v in worst.items()))
    # the flat and saturated cases are the ones where the reference's own fp32 misses float64 by >= 2e-5 (E[x^2] - mu^2
    # cancels against C2); the kernel stays within the bar there as well
    for kind in ("flat", "saturated"):
        i = names.index(f"{kind}_3x256x256_w11")
        assert np.abs(gold["f32"][i] - gold["f64"][i]).max() >= 2e-5 > 20 * worst[names[i]], (kind, worst[names[i]])


def _rel(got, want):
    return np.abs(got - want) / np.maximum(np.abs(want), 1e-30)


@pytest.mark.parametrize("layout", ["nchw", "nhwc_view", "u8_bgr", "bf16", "fp16"])
def test_layouts_against_float64_oracle(dev, layout):
    from mmhand_amd.metrics import image_metrics
    rs = np.random.RandomState({"nchw": 1, "nhwc_view": 2, "u8_bgr": 3, "bf16": 4, "fp16": 5}[layout])
    for trial in range(4):
        B, C = int(rs.randint(1, 5)), int(rs.choice([1, 3]))
        H, W = int(rs.randint(5, 90)), int(rs.randint(5, 90))
        window = int(rs.choice([3, 5, 7, 9, 11, 13, 15]))
        if layout == "u8_bgr":
            C = 3
            a = torch.from_numpy(rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8))
            b = torch.from_numpy(np.clip(a.numpy().astype(int) + rs.randint(-20, 21, (B, H, W, 3)), 0, 255).astype(np.uint8))
            m = image_metrics(a.to(dev), b.to(dev), range="u8_bgr_hwc", window=window)
            rgb = lambda t: t.flip(-1).permute(0, 3, 1, 2).double() / 255.0            # noqa: E731
            want = oracle(rgb(a), rgb(b), window)
        else:
            a = torch.from_numpy(rs.uniform(-1, 1, (B, C, H, W)).astype(np.float32))
            b = torch.from_numpy(np.clip(a.numpy() + 0.2 * rs.standard_normal((B, C, H, W)), -1, 1).astype(np.float32))
            if layout in ("bf16", "fp16"):
                a, b = (a.bfloat16(), b.bfloat16()) if layout == "bf16" else (a.half(), b.half())
                da, db = a.to(dev), b.to(dev)
            elif layout == "nhwc_view":
                def view(t):
                    buf = torch.zeros((B, H, W, 4), dtype=torch.float32, device=dev)
                    buf[..., :C] = t.permute(0, 2, 3, 1).to(dev)
                    return buf.permute(0, 3, 1, 2)[:, :C]
                da, db = view(a), view(b)
                assert not da.is_contiguous()
            else:
                da, db = a.to(dev), b.to(dev)
            m = image_metrics(da, db, range="pm1", window=window)
            want = oracle((a.double() + 1) / 2, (b.double() + 1) / 2, window)
        got = [m[k].cpu().numpy() for k in ("ssim", "l1", "mse")]
        assert got[0].dtype == np.float64 and got[0].shape == (B,)
        assert np.abs(got[0] - want[0]).max() <= BAR, (layout, B, C, H, W, window, got[0], want[0])
        assert _rel(got[1], want[1]).max() <= BAR and _rel(got[2], want[2]).max() <= BAR, (layout, got[1:], want[1:])
        assert torch.equal(m["psnr"].cpu(), -10 * torch.log10(m["mse"].cpu()))


def test_identity_and_symmetry_are_exact(dev):
    from mmhand_amd.metrics import image_metrics
    from tests.ssim_cases import make_case
    for kind in ("uniform", "flat", "saturated", "smooth"):
        a, b = make_case(kind, (3, 67, 45))
        a, b = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        m = image_metrics(a, a)
        assert (m["ssim"] == 1.0).all() and (m["l1"] == 0).all() and (m["mse"] == 0).all()
        assert torch.isinf(m["psnr"]).all() and (m["psnr"] > 0).all()
        ab, ba = image_metrics(a, b), image_metrics(b, a)
        for k in ("ssim", "l1", "mse", "psnr"):
            assert torch.equal(ab[k], ba[k]), (kind, k)


def test_batch_independent_and_deterministic(dev):
    from mmhand_amd.metrics import image_metrics
    rs = np.random.RandomState(7)
    a = torch.from_numpy(rs.uniform(-1, 1, (7, 3, 70, 50)).astype(np.float32)).to(dev)
    b = torch.from_numpy(rs.uniform(-1, 1, (7, 3, 70, 50)).astype(np.float32)).to(dev)
    full, again = image_metrics(a, b), image_metrics(a, b)
    alone = image_metrics(a[5:6].clone(), b[5:6].clone())
    for k in ("ssim", "l1", "mse"):
        assert torch.equal(full[k], again[k])
        assert torch.equal(full[k][5:6], alone[k])


def _train(root, name, norm):
    from mmhand_amd import train
    train.main(["--name", name, "--dataroot", root, "--dataset", "rhd", "--augmentation_ratio", "0.5", "--batchSize", "2",
                "--ngf", "8", "--ndf", "8", "--G_n_blocks", "2", "--n_layers_D", "2", "--norm", norm, "--fineSize", "32",
                "--niter", "1", "--niter_decay", "0", "--print_freq", "2", "--vgg_random_init", "--checkpoints_dir",
                "checkpoints", "--pool_size", "2"])


def _generator_oracle(root, name, dev, bf16=False):
    """per target path: fp64 oracle (ssim, l1) of the generator's output against H2, recomputed with InferenceGenerator"""
    from mmhand_amd.data import HandFolderLoader
    from mmhand_amd.evaluate import infer_generator_config, strip_module
    from mmhand_amd.inference import InferenceGenerator
    from mmhand_amd.networks import Generator
    from mmhand_amd.options import default_train_opt
    sd = strip_module(torch.load(os.path.join("checkpoints", name, "latest_net_netG.pth"), map_location="cpu"))
    ngf, nb, norm, drop = infer_generator_config(sd)
    net = Generator([3, 42, 6], 3, ngf, norm, drop, nb)
    net.load_state_dict(sd)
    gen = InferenceGenerator(net.to(dev).eval(), use_graph=True, bf16=bf16)
    opt = default_train_opt(batchSize=2, local_rank=0, isTrain=False)
    opt.dataroot, opt.dataset, opt.augmentation_ratio, opt.distributed = root, "rhd", 0.5, False
    random.seed(11)
    out = {}
    for s in HandFolderLoader(opt, device=dev, decoded=True):
        fake = gen([s["H1"], torch.cat((s["P1"], s["P2"]), 1), torch.cat((s["D1"], s["D2"]), 1)])
        ss, l1, _ = oracle((fake.double() + 1) / 2, (s["H2"].double() + 1) / 2)
        for i, t in enumerate(s["H2_path"]):
            out[t] = (ss[i], l1[i], s["H1_path"][i])
    return out


def _evaluate(argv):
    from mmhand_amd import evaluate
    random.seed(11)                  # the loader's source shuffle (generic_dataset.py:129) draws from Python's random
    return evaluate.main(argv)


@pytest.fixture
def work_dir():
    """a scratch directory whose PATH does not contain "test" (pytest's tmp_path does; generic_dataset.py:116 keys on it)"""
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="mmh_ev_")
    assert "test" not in d
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("norm", ["batch", "instance"])
def test_evaluate_generator_and_directory_modes(dev, work_dir, monkeypatch, norm):
    from PIL import Image
    from tests._dataset_fixture import write_rhd
    from mmhand_amd import aug
    root = os.path.join(work_dir, "rhd")
    names = write_rhd(root, n=10, size=32)
    monkeypatch.chdir(work_dir)
    _train(root, "ev", norm)
    want = _generator_oracle(root, "ev", dev)
    assert len(want) == 5
    base = ["--name", "ev", "--dataroot", root, "--dataset", "rhd", "--augmentation_ratio", "0.5"]
    res = _evaluate(base + ["--batchSize", "2", "--results_json", "r.json", "--per_image_csv", "r.csv"])
    rows = res["rows"]
    assert [r["target"] for r in rows] == list(want)
    for r in rows:
        s, l1, src = want[r["target"]]
        assert abs(r["ssim"] - s) <= BAR and abs(r["l1"] - l1) <= BAR * max(l1, 1.0) and r["source"] == src, (r, want[r["target"]])
    for bs in ("1", "3"):
        other = _evaluate(base + ["--batchSize", bs, "--results_json", f"r{bs}.json"])["rows"]
        assert [r["target"] for r in other] == list(want)
        assert max(abs(x["ssim"] - y["ssim"]) for x, y in zip(rows, other)) <= BAR
        assert max(abs(x["l1"] - y["l1"]) for x, y in zip(rows, other)) <= BAR
    # the generator's 16-bit mode: the same pairs, scored against what InferenceGenerator(bf16=True) makes of them
    want16 = _generator_oracle(root, "ev", dev, bf16=True)
    rows16 = _evaluate(base + ["--batchSize", "2", "--bf16", "--results_json", "r16.json"])["rows"]
    assert [r["target"] for r in rows16] == list(want16)
    for r in rows16:
        s, l1, _ = want16[r["target"]]
        assert abs(r["ssim"] - s) <= BAR and abs(r["l1"] - l1) <= BAR * max(l1, 1.0), (r, want16[r["target"]])
    assert json.load(open("r16.json"))["options"]["bf16"] is True
    js = json.load(open("r.json"))
    assert set(js["summary"]) == {"SSIM_avg", "SSIM_std", "L1_avg", "PSNR_avg", "n"} and js["summary"]["n"] == 5
    assert js["options"]["name"] == "ev" and js["generator"] == {"ngf": 8, "n_blocks": 2, "norm": norm, "use_dropout": True}
    ss = np.array([r["ssim"] for r in rows])
    assert abs(js["summary"]["SSIM_avg"] - ss.mean()) < 1e-12 and abs(js["summary"]["SSIM_std"] - ss.std()) < 1e-12
    with open("r.csv") as fh:
        table = list(csv.reader(fh))
    assert table[0] == ["target", "source", "ssim", "l1", "psnr"] and len(table) == 6
    assert [t[0] for t in table[1:]] == list(want)
    if norm != "batch":
        return
    # directory mode on aug.py's PNGs (aug.py builds the batch-norm generator with dropout, as trained here)
    written = aug.main(["ev", root, "gen", "rhd", "0.5", "0"], ngf=8, n_blocks=2)
    assert len(written) == 5
    res = _evaluate(["--generated", "gen", "--dataroot", root, "--dataset", "rhd", "--augmentation_ratio", "0.5",
                     "--batchSize", "3", "--per_image_csv", "g.csv"])
    assert os.path.isfile(os.path.join("gen", "eval_rhd.json"))
    for r in res["rows"]:
        g = np.array(Image.open(os.path.join("gen", *r["target"].split("/")[-2:])).convert("RGB"))
        t = np.array(Image.open(r["target"]).convert("RGB"))
        to = lambda x: torch.from_numpy(x).permute(2, 0, 1)[None].double() / 255.0    # noqa: E731
        s, l1, mse = oracle(to(g), to(t))
        assert abs(r["ssim"] - s[0]) <= BAR and abs(r["l1"] - l1[0]) <= BAR * l1[0], (r, s, l1)
        # the PNGs are the generator's output quantised: close to the tensor scores
        assert abs(r["ssim"] - want[r["target"]][0]) < 0.05
    assert len(list(csv.reader(open("g.csv")))) == 6
    assert sorted(names)            # the fixture wrote its images
