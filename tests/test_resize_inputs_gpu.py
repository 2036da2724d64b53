"""--resize_inputs on the device: mmh_decode_inputs_resized against the float64 restatement of its sampling rule
(tests/_resize_oracle.py, pinned to F.interpolate by test_resize_inputs_cpu.py), the identity size, and the flag end to end
through train, the step, --graph_step and aug on a prepared directory whose files are 32 x 32."""
import os
import random
import shutil
import tempfile

import numpy as np
import pytest
import torch

from oracle import mmhand_ref as O
from tests import _resize_oracle as RO
from tests.golden import recipe as RC

pytestmark = pytest.mark.gpu
S = RC.SMALL
B, HS, WS = 2, 12, 10               # H != W: a transposed index shows
# three small targets (up 2x, independent ratios, down) + one large enough for the kernel's grid-stride loop to
# come round (more than 4096 blocks x 256 lanes / 15 lanes per pixel = 69,905 output pixels)
TARGETS = [(24, 20), (20, 28), (8, 4), (192, 200)]


def _raw_batch():
    rs = np.random.RandomState(7)
    imgs = [rs.randint(0, 256, size=(B, HS, WS, 3)).astype(np.uint8) for _ in range(2)]
    deps = [rs.randint(0, 256, size=(B, HS, WS, 3)).astype(np.uint8) for _ in range(2)]
    for d in deps:
        d[..., 1] = rs.randint(0, 3, size=(B, HS, WS))          # realistic range: depth < 700
        # neighbours that straddle a G boundary, along x and along y: (G, R) = (0, 255) next to (1, 0)
        d[:, 3, 4, 1:] = (0, 255)
        d[:, 3, 5, 1:] = (1, 0)
        d[:, 4, 4, 1:] = (1, 0)
    # joints as tests/_dataset_fixture.py draws them (uniform over the image and 4 pixels beyond it), then one off the image
    # and two on its border in every set
    uvs = [np.stack([rs.uniform(-4, WS + 4, size=(B, 21)), rs.uniform(-4, HS + 4, size=(B, 21))], -1) for _ in range(2)]
    for uv in uvs:
        uv[:, 0] = (-3.25, HS + 2.5)
        uv[:, 1] = (WS - 1.0, 0.0)
        uv[:, 2] = (0.0, 5.5)
    return imgs, deps, uvs


@pytest.fixture(scope="module")
def raw():
    return _raw_batch()


@pytest.fixture(scope="module")
def expected(raw):
    """the float64 oracle per target, computed once: colour [B,Ho,Wo,3] RGB and depth [B,Ho,Wo] per side as float64, pose
    maps [B,Ho,Wo,42] fp32 from oracle.pose_heatmaps on the scaled joints, and that no Gaussian sits on the threshold"""
    imgs, deps, uvs = raw
    out = {}
    for Ho, Wo in TARGETS:
        e = {"h": [], "d": [], "p": None}
        for s in range(2):
            hd = [RO.decode_resized(imgs[s][b], deps[s][b], Ho, Wo) for b in range(B)]
            e["h"].append(np.stack([h.transpose(1, 2, 0) for h, _ in hd]))
            e["d"].append(np.stack([d for _, d in hd]))
        scaled = [RO.scale_joints(uv, (HS, WS), (Ho, Wo)) for uv in uvs]
        e["p"] = np.stack([np.concatenate([O.pose_heatmaps(scaled[0][b], Ho, Wo), O.pose_heatmaps(scaled[1][b], Ho, Wo)], 0)
                           for b in range(B)]).transpose(0, 2, 3, 1)
        # the support mask is compared bit for bit: no pixel's Gaussian may sit within rounding of the 0.0099 threshold
        gy, gx = np.mgrid[0:Ho, 0:Wo]
        margin = np.inf
        for sc in scaled:
            for u, v in sc.reshape(-1, 2):
                g = np.exp(-((gx - u) ** 2 + (gy - v) ** 2) / 2.0 / 6.0 / 6.0)
                margin = min(margin, float(np.abs(g - 0.0099).min()))
        e["margin"] = margin
        out[(Ho, Wo)] = e
    return out


def _dev(raw, dev):
    imgs, deps, uvs = raw
    t = lambda a: torch.from_numpy(a).to(dev)                     # noqa: E731
    return t(imgs[0]), t(imgs[1]), t(deps[0]), t(deps[1]), t(uvs[0]), t(uvs[1])


def _assert_f32(got, want64, what):
    w32, tol = RO.f32_tolerance(want64)
    err = np.abs(got.astype(np.float64) - w32.astype(np.float64))
    worst = float((err / tol).max())
    print(f"{what}: max |got - fp32(float64)| = {err.max():.3e}, worst error / tolerance = {worst:.3f}")
    assert (err <= tol).all(), (what, float(err.max()), worst)


def _check_against_oracle(x, e, Ho, Wo, tag):
    xh1, xh2, xp, xd = (t.cpu().numpy() for t in x)
    assert xh1.shape == (B, Ho, Wo, 4) and xh2.shape == (B, Ho, Wo, 4) and xp.shape == (B, Ho, Wo, 44) and xd.shape == (B, Ho, Wo, 8)
    _assert_f32(xh1[..., :3], e["h"][0], tag + " colour 1")
    _assert_f32(xh2[..., :3], e["h"][1], tag + " colour 2")
    for c in range(3):
        _assert_f32(xd[..., c], e["d"][0], tag + " depth 1")
        _assert_f32(xd[..., 3 + c], e["d"][1], tag + " depth 2")
    assert np.array_equal(xd[..., 0], xd[..., 1]) and np.array_equal(xd[..., 0], xd[..., 2])
    # pad lanes
    assert not xh1[..., 3].any() and not xh2[..., 3].any() and not xd[..., 6:].any() and not xp[..., 42:].any()
    # pose maps: the support mask bit for bit, values within 1 ulp (as test_pointwise_gpu.py holds mmh_decode_inputs)
    assert e["margin"] > 1e-9, e["margin"]
    assert np.array_equal(xp[..., :42] > 0, e["p"] > 0)
    ulp = np.abs(xp[..., :42].view(np.int32).astype(np.int64) - e["p"].view(np.int32).astype(np.int64))
    assert ulp.max() <= 1
    assert (e["p"] > 0).any()
    if Ho * Wo >= 400:
        assert not (e["p"] > 0).all()                             # the threshold is in play at this size


@pytest.mark.parametrize("out", TARGETS, ids=lambda s: "%dx%d" % s)
def test_resized_decode_vs_float64_oracle(out, raw, expected, dev):
    """colour and depth within 1 ulp of the float64 result rounded to fp32 (RO.f32_tolerance), pose maps from
    oracle.pose_heatmaps on the scaled joints with an identical support mask, pad lanes zero; through ops.decode_inputs,
    which scales the joints"""
    from mmhand_amd import ops
    x = ops.decode_inputs(*_dev(raw, dev), out_size=out)
    _check_against_oracle(x, expected[out], out[0], out[1], "%dx%d" % out)


def test_identity_size(raw, dev):
    """out_size equal to the source takes the existing call, bit for bit; the new entry point called at Ho = Hs, Wo = Ws
    samples every pixel with weight 0 - within 1 ulp of the old kernel, pose maps identical"""
    from mmhand_amd import lib as L
    from mmhand_amd import ops
    t = _dev(raw, dev)
    plain = ops.decode_inputs(*t)
    same = ops.decode_inputs(*t, out_size=(HS, WS))
    for a, b in zip(plain, same):
        assert torch.equal(a, b)
    outs = [torch.full((B, HS, WS, c), float("nan"), dtype=torch.float32, device=dev) for c in (4, 4, 44, 8)]
    L.call("mmh_decode_inputs_resized", *[ops._ptr(a) for a in t], B, HS, WS, HS, WS, 6.0, *[ops._ptr(o) for o in outs],
           ops._stream())
    for name, a, b in zip(("x_h1", "x_h2", "x_p", "x_d"), plain, outs):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.isfinite(b).all(), name
        if name == "x_p":
            assert np.array_equal(a, b)
        else:
            assert (np.abs(a.astype(np.float64) - b) <= np.spacing(np.abs(a))).all(), name


# ----------------------------------------------------------------------------- end to end on a prepared directory
def _opt(**kw):
    from mmhand_amd.options import default_train_opt
    args = dict(batchSize=2, ngf=S["ngf"], ndf=S["ndf"], n_layers_D=S["n_layers_D"], G_n_blocks=S["n_blocks"], norm="instance",
                no_dropout=True, no_dropout_D=True, pool_size=2, name="resize", checkpoints_dir="/tmp/mmh_resize_ckpt",
                local_rank=0, dataset="rhd", augmentation_ratio=1.0, nThreads=2, resize_inputs=64)
    args.update(kw)
    return default_train_opt(**args)


@pytest.fixture(scope="module")
def rhd_dir():
    """a prepared directory of 32 x 32 files (its path must not contain "test": generic_dataset.py:116 keys on that)"""
    from tests._dataset_fixture import write_rhd
    d = tempfile.mkdtemp(prefix="mmh_rs_")
    root = os.path.join(d, "rhd")
    names = write_rhd(root, n=8, size=32)
    yield d, root, names
    shutil.rmtree(d, ignore_errors=True)


def _oracle_batch(b, size):
    """the batch dict of decoded tensors (H1, P1, D1, H2, P2, D2: NCHW fp32 on the host) the float64 oracle makes of a raw
    batch at size x size"""
    out = {}
    for s in ("1", "2"):
        img, dep, uv = (b[k + s].cpu().numpy() for k in ("img", "dep", "uv"))
        n, hs, ws, _ = img.shape
        hd = [RO.decode_resized(img[j], dep[j], size, size) for j in range(n)]
        out["H" + s] = torch.from_numpy(np.stack([h for h, _ in hd]).astype(np.float32))
        out["D" + s] = torch.from_numpy(np.stack([np.stack([d, d, d]) for _, d in hd]).astype(np.float32))
        sc = RO.scale_joints(uv, (hs, ws), (size, size))
        out["P" + s] = torch.from_numpy(np.stack([O.pose_heatmaps(sc[j], size, size) for j in range(n)]))
    return out


def test_step_with_the_flag_equals_step_on_oracle_resized_tensors(rhd_dir, dev):
    """one optimize_parameters() on a raw 32 x 32 batch under --resize_inputs 64 == the same step fed the tensors the
    float64 oracle resize produces, to the tolerance test_model_gpu.py holds "a step on the raw batch == a step on the
    decoded tensors" to (rtol 1e-6 on the six losses); C1 / C2 arrive scaled, depth untouched"""
    from mmhand_amd.data import HandFolderLoader
    from mmhand_amd.mmhand_model import MMHandModel
    _, root, _ = rhd_dir
    opt = _opt(dataroot=root)
    random.seed(5)
    ld = HandFolderLoader(opt, device=dev)
    b = list(ld)[1]
    assert tuple(b["img1"].shape) == (2, 32, 32, 3)                # the raw batch stays at the files' size
    model = MMHandModel(opt)
    model.set_input(b)
    assert tuple(model.input_H1.shape) == (2, 3, 64, 64) and tuple(model.input_P2.shape) == (2, 21, 64, 64)
    assert tuple(model.x_D.shape) == (2, 64, 64, 8)
    want_c = RO.scale_joints(b["C1"].cpu().numpy(), (32, 32), (64, 64))
    assert np.array_equal(model.input_C1.cpu().numpy(), want_c) and np.array_equal(want_c[..., 2], b["C1"].cpu().numpy()[..., 2])
    random.seed(9)
    model.optimize_parameters()
    l_flag = [float(v) for v in model.get_current_errors().values()]
    # the decoded form of the loader resizes too, and hands the scaled joints on
    dec = HandFolderLoader(opt, device=dev, decoded=True)
    dec.image_source, dec.image_target = ld.image_source, ld.image_target
    db = list(dec)[1]
    assert tuple(db["H2"].shape) == (2, 3, 64, 64) and torch.equal(db["H2"], model.input_H2)
    assert np.array_equal(db["C2"].cpu().numpy(), RO.scale_joints(b["C2"].cpu().numpy(), (32, 32), (64, 64)))
    model2 = MMHandModel(_opt(dataroot=root, resize_inputs=0))
    model2.set_input(_oracle_batch(b, 64))
    random.seed(9)
    model2.optimize_parameters()
    l_orc = [float(v) for v in model2.get_current_errors().values()]
    print("losses with the flag", l_flag, "on the oracle's tensors", l_orc)
    assert np.allclose(l_flag, l_orc, rtol=1e-6), (l_flag, l_orc)
    assert all(np.isfinite(l_flag))


def _run_graph(opt, batches, n_iter, capture, monkeypatch):
    """tests/test_graph_step_gpu.py's _run on raw batches of the prepared directory"""
    from mmhand_amd.mmhand_model import MMHandModel
    monkeypatch.setenv("MMH_GRAPH_CAPTURE", "1" if capture else "0")
    random.seed(17)
    model = MMHandModel(opt)
    losses = []
    for it in range(n_iter):
        model.set_input(batches[it % len(batches)])
        model.optimize_parameters()
        losses.append([float(v) for v in model.get_current_errors().values()])
    model._settle_overflow(drain=True)
    torch.cuda.synchronize()
    state = {n: getattr(model, n).flat_param.detach().clone() for n in ("netG", "netD_PB", "netD_PP")}
    state["fake"] = model.fake_p2.detach().clone()
    return model, losses, state


def test_graph_step_with_the_flag_is_the_eager_form_bit_for_bit(rhd_dir, dev, monkeypatch):
    """--graph_step --resize_inputs 64 on raw 32 x 32 batches, dropout on, a pool of three: captured-and-replayed == the
    same form run eagerly, all losses, weights and the generated image to the bit.  Six iterations: the first four end
    with the capture itself; the two behind it go through set_input's replay branch, the second decode site"""
    from mmhand_amd.data import HandFolderLoader
    _, root, _ = rhd_dir
    kw = dict(dataroot=root, graph_step=True, no_dropout=False, no_dropout_D=False, pool_size=3, name="resize_graph")
    random.seed(5)
    batches = list(HandFolderLoader(_opt(**kw), device=dev))
    assert len(batches) == 4
    eager, l0, s0 = _run_graph(_opt(**kw), batches, 6, False, monkeypatch)
    assert eager._graph is None and eager.graph_replays == 0
    graph, l1, s1 = _run_graph(_opt(**kw), batches, 6, True, monkeypatch)
    assert graph.graph_error is None, graph.graph_error
    assert graph._graph is not None and graph.graph_replays == 6 - graph._graph_warm >= 3
    assert tuple(graph._static_inputs["input_H1"].shape) == (2, 3, 64, 64)
    assert np.array_equal(np.array(l0[:4]), np.array(l1[:4])), (l0[:4], l1[:4])
    assert np.array_equal(np.array(l0), np.array(l1)), (l0, l1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    assert tuple(s1["fake"].shape) == (2, 3, 64, 64) and all(np.isfinite(l1[-1]))


@pytest.fixture(scope="module")
def trained(rhd_dir, dev):
    """`python -m mmhand_amd.train --dataroot DIR --resize_inputs 64` for one epoch of two iterations, once for the module"""
    from mmhand_amd import mmhand_model as MM
    from mmhand_amd import train
    d, root, names = rhd_dir
    seen = {}
    real_init = MM.MMHandModel.__init__

    def spy_init(self, opt):
        real_init(self, opt)
        seen["model"] = self
    cwd = os.getcwd()
    os.chdir(d)
    MM.MMHandModel.__init__ = spy_init
    try:
        train.main(["--name", "files64", "--dataroot", root, "--dataset", "rhd", "--augmentation_ratio", "0.5", "--batchSize", "2",
                    "--ngf", "8", "--ndf", "8", "--G_n_blocks", "2", "--n_layers_D", "2", "--norm", "batch", "--resize_inputs", "64",
                    "--niter", "1", "--niter_decay", "0", "--print_freq", "2", "--vgg_random_init", "--checkpoints_dir",
                    "checkpoints", "--pool_size", "2"])
    finally:
        MM.MMHandModel.__init__ = real_init
        os.chdir(cwd)
    return d, root, names, seen["model"]


def test_train_runs_at_the_resized_size(trained):
    """two iterations on 32 x 32 files at 64 x 64: the networks' inputs (the reference's input_H2, the L1 target) and the
    generated image are 64 wide, losses were logged, a checkpoint was written"""
    d, _, _, model = trained
    assert model.resize_inputs == 64 and model.opt.fineSize == 256          # --fineSize keeps its dead meaning
    assert model.input_H2.shape[-1] == 64 and tuple(model.input_H2.shape) == (2, 3, 64, 64)
    assert tuple(model.fake_p2.shape) == (2, 3, 64, 64)
    assert model.optimizer_G.step_count == 2
    log = open(os.path.join(d, "checkpoints", "files64", "loss_log.txt")).read().strip().splitlines()
    assert len(log) == 2 and all("pair_L1loss" in l for l in log)
    assert os.path.isfile(os.path.join(d, "checkpoints", "files64", "latest_net_netG.pth"))


def test_aug_writes_pngs_at_the_resized_size_and_evaluate_scores_them(trained, monkeypatch):
    """aug with the flag writes one 64 x 64 PNG per target of the generation split to <dst>/<folder>/<name>; evaluate
    --generated on that directory scores them against the targets decoded at 64 x 64, and refuses them without the flag"""
    from PIL import Image
    from mmhand_amd import aug, evaluate
    d, root, names, _ = trained
    monkeypatch.chdir(d)
    written = aug.main(["files64", root, "gen64", "rhd", "0.5", "0", "--resize_inputs", "64"], ngf=8, n_blocks=2)
    ordered = sorted(names, key=lambda x: int(x[:-4]))
    assert [os.path.relpath(p, "gen64") for p in written] == [os.path.join("color", n) for n in ordered[:4]]
    for p in written:
        png = np.asarray(Image.open(p))
        assert png.shape == (64, 64, 3) and png.dtype == np.uint8 and png.std() > 0
    base = ["--generated", "gen64", "--dataroot", root, "--dataset", "rhd", "--augmentation_ratio", "0.5", "--batchSize", "4"]
    res = evaluate.main(base + ["--resize_inputs", "64"])
    assert res["summary"]["n"] == 4 and all(np.isfinite(r["ssim"]) and 0 <= r["l1"] <= 1 for r in res["rows"])
    with pytest.raises(SystemExit, match="generated image"):
        evaluate.main(base)
    with pytest.raises(ValueError, match="resize_inputs"):
        aug.main(["files64", root, "gen30", "rhd", "0.5", "0", "--resize_inputs", "30"], ngf=8, n_blocks=2)
