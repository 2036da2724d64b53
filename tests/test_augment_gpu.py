"""--augment_geom on the device: mmh_decode_inputs_affine against the float64 restatement of its sampling rule
(tests/_affine_oracle.py, pinned to F.grid_sample by test_augment_cpu.py), identity matrices against the resize pass, the
slot-fed entry point against the batch-fed one, and the flag end to end through the loaders and the step on a prepared
directory whose files are 32 x 32."""
import os
import random
import shutil
import tempfile

import numpy as np
import pytest
import torch

from oracle import mmhand_ref as O
from tests import _affine_oracle as AO
from tests.golden import recipe as RC

pytestmark = pytest.mark.gpu
SM = RC.SMALL
B, HS, WS = 2, 12, 10               # H != W: a transposed index shows
# the source's own size, up 2x, down with independent ratios, and one large enough for the kernel's grid-stride loop to
# come round (more than 4096 blocks x 256 lanes / 15 lanes per pixel = 69,905 output pixels)
TARGETS = [(12, 10), (24, 20), (8, 4), (192, 200)]
# one draw per (sample, side), all different, so that a matrix indexed by the wrong b or the wrong side shows:
# identity, an exact quarter turn, a flip, and a general rotation + scale + shift that sends a good share outside
DRAWS = [[(0.0, 1.0, 0.0, 0.0, False), (90.0, 1.0, 0.0, 0.0, False)],
         [(0.0, 1.0, 0.0, 0.0, True), (25.0, 0.8, 0.1, -0.05, False)]]
GENERAL = (1, 1)


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
        assert (256.0 * d[..., 1] + d[..., 2]).max() <= AO.MAX_RAW_DEPTH
    # joints uniform over the image and 4 pixels beyond it, then one off the image and two on its border in every set
    uvs = [np.stack([rs.uniform(-4, WS + 4, size=(B, 21)), rs.uniform(-4, HS + 4, size=(B, 21))], -1) for _ in range(2)]
    for uv in uvs:
        uv[:, 0] = (-3.25, HS + 2.5)
        uv[:, 1] = (WS - 1.0, 0.0)
        uv[:, 2] = (0.0, 5.5)
    return imgs, deps, uvs


@pytest.fixture(scope="module")
def raw():
    return _raw_batch()


def _matrices(dst):
    """-> (fwd [B,2,2,3], xf [B,2,6]) of DRAWS for the target, from the oracle's own builders"""
    fwd = np.array([[AO.forward(*DRAWS[b][s], (HS, WS)) for s in range(2)] for b in range(B)])
    xf = np.array([[AO.inverse(fwd[b, s], (HS, WS), dst) for s in range(2)] for b in range(B)]).reshape(B, 2, 6)
    return fwd, np.ascontiguousarray(xf)


@pytest.fixture(scope="module")
def expected(raw):
    """the float64 oracle per target, computed once: colour [B,Ho,Wo,3] RGB and depth [B,Ho,Wo] per side as float64, pose
    maps [B,Ho,Wo,42] fp32 from oracle.pose_heatmaps on the transformed joints, the distance of the nearest Gaussian value
    from the threshold, and the share of the general matrix's samples that fall outside the source"""
    imgs, deps, uvs = raw
    out = {}
    for Ho, Wo in TARGETS:
        fwd, xf = _matrices((Ho, Wo))
        e = {"h": [], "d": [], "xf": xf, "uv": []}
        for s in range(2):
            hd = [AO.decode_affine(imgs[s][b], deps[s][b], xf[b, s].reshape(2, 3), Ho, Wo) for b in range(B)]
            e["h"].append(np.stack([h.transpose(1, 2, 0) for h, _ in hd]))
            e["d"].append(np.stack([d for _, d in hd]))
            e["uv"].append(np.stack([AO.joints(uvs[s][b], fwd[b, s], (HS, WS), (Ho, Wo)) for b in range(B)]))
        e["p"] = np.stack([np.concatenate([O.pose_heatmaps(e["uv"][0][b], Ho, Wo), O.pose_heatmaps(e["uv"][1][b], Ho, Wo)], 0)
                           for b in range(B)]).transpose(0, 2, 3, 1)
        # the support mask is compared bit for bit: no pixel's Gaussian may sit within rounding of the 0.0099 threshold
        gy, gx = np.mgrid[0:Ho, 0:Wo]
        margin = np.inf
        for sc in e["uv"]:
            for u, v in sc.reshape(-1, 2):
                g = np.exp(-((gx - u) ** 2 + (gy - v) ** 2) / 2.0 / 6.0 / 6.0)
                margin = min(margin, float(np.abs(g - 0.0099).min()))
        e["margin"] = margin
        e["outside"] = AO.outside_share(xf[GENERAL].reshape(2, 3), (HS, WS), (Ho, Wo))
        out[(Ho, Wo)] = e
    return out


def _dev(raw, dev):
    imgs, deps, _ = raw
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)         # noqa: E731
    return t(imgs[0]), t(imgs[1]), t(deps[0]), t(deps[1])


def _assert_f32(got, want64, what):
    w32, tol = AO.f32_tolerance(want64)
    err = np.abs(got.astype(np.float64) - w32.astype(np.float64))
    worst = float((err / tol).max())
    print(f"{what}: max |got - fp32(float64)| = {err.max():.3e}, worst error / tolerance = {worst:.3f}")
    assert (err <= tol).all(), (what, float(err.max()), worst)


@pytest.mark.parametrize("out", TARGETS, ids=lambda s: "%dx%d" % s)
def test_affine_decode_vs_float64_oracle(out, raw, expected, dev):
    """colour and depth within 1 ulp of the float64 result rounded to fp32 (AO.f32_tolerance), the three depth lanes equal,
    pad lanes zero, pose maps from oracle.pose_heatmaps on the transformed joints with an identical support mask and
    values within 1 ulp; the general matrix samples between 5 % and 60 % of its pixels outside the source"""
    from mmhand_amd import ops
    Ho, Wo = out
    e = expected[out]
    print(f"{Ho}x{Wo}: outside share of the general matrix {e['outside']:.3f}, threshold margin {e['margin']:.3e}")
    assert 0.05 <= e["outside"] <= 0.60, e["outside"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)         # noqa: E731
    x = ops.decode_inputs_affine(*_dev(raw, dev), t(e["uv"][0]), t(e["uv"][1]), t(e["xf"]), out_size=out)
    xh1, xh2, xp, xd = (a.cpu().numpy() for a in x)
    assert xh1.shape == (B, Ho, Wo, 4) and xh2.shape == (B, Ho, Wo, 4) and xp.shape == (B, Ho, Wo, 44) and xd.shape == (B, Ho, Wo, 8)
    tag = "%dx%d" % out
    _assert_f32(xh1[..., :3], e["h"][0], tag + " colour 1")
    _assert_f32(xh2[..., :3], e["h"][1], tag + " colour 2")
    for c in range(3):
        _assert_f32(xd[..., c], e["d"][0], tag + " depth 1")
        _assert_f32(xd[..., 3 + c], e["d"][1], tag + " depth 2")
    assert np.array_equal(xd[..., 0], xd[..., 1]) and np.array_equal(xd[..., 0], xd[..., 2])
    assert np.array_equal(xd[..., 3], xd[..., 4]) and np.array_equal(xd[..., 3], xd[..., 5])
    # pad lanes
    assert not xh1[..., 3].any() and not xh2[..., 3].any() and not xd[..., 6:].any() and not xp[..., 42:].any()
    # pose maps: the support mask bit for bit, values within 1 ulp (as test_resize_inputs_gpu.py holds the resize pass)
    assert e["margin"] > 1e-9, e["margin"]
    assert np.array_equal(xp[..., :42] > 0, e["p"] > 0)
    ulp = np.abs(xp[..., :42].view(np.int32).astype(np.int64) - e["p"].view(np.int32).astype(np.int64))
    assert ulp.max() <= 1
    assert (e["p"] > 0).any()
    if Ho * Wo >= 400:
        assert not (e["p"] > 0).all()                             # the threshold is in play at this size
    # the sides differ and the samples differ: a matrix taken from the wrong row would have passed nothing above
    assert not np.array_equal(e["xf"][0, 0], e["xf"][0, 1]) and not np.array_equal(e["xf"][0], e["xf"][1])


def test_identity_matrices_are_the_resize_pass_at_the_source_size_bit_for_bit(raw, dev):
    from mmhand_amd import lib as L
    from mmhand_amd import ops
    _, _, uvs = raw
    src = _dev(raw, dev)
    uv = [torch.from_numpy(u).to(dev) for u in uvs]
    xf = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], dtype=torch.float64, device=dev).repeat(B, 2, 1).contiguous()
    got = ops.decode_inputs_affine(*src, *uv, xf)
    outs = [torch.full((B, HS, WS, c), float("nan"), dtype=torch.float32, device=dev) for c in (4, 4, 44, 8)]
    L.call("mmh_decode_inputs_resized", *[ops._ptr(a) for a in src + tuple(uv)], B, HS, WS, HS, WS, 6.0,
           *[ops._ptr(o) for o in outs], ops._stream())
    for name, g, w in zip(("x_h1", "x_h2", "x_p", "x_d"), got, outs):
        assert tuple(g.shape) == tuple(w.shape) and torch.isfinite(w).all(), name
        assert torch.equal(g, w), name


# ----------------------------------------------------------------------------- slot-fed against batch-fed
S = 7
# slot 0 and slot 6; sample 1 has ONE slot as img1 and img2; slot 6 serves two samples
IDX = [[0, 6, 1, 2], [3, 3, 4, 5], [6, 2, 0, 1]]


@pytest.fixture(scope="module")
def small_store(dev):
    rs = np.random.RandomState(23)
    store = rs.randint(0, 256, size=(S, HS, WS, 3)).astype(np.uint8)
    store[..., 1] = np.where(rs.rand(S, HS, WS) < 0.5, rs.randint(0, 3, size=(S, HS, WS)), store[..., 1])
    uv = np.stack([rs.uniform(-4, 2 * WS + 4, size=(3, 2, 21)), rs.uniform(-4, 2 * HS + 4, size=(3, 2, 21))], -1)
    cases = [(0.0, 1.0, 0.0, 0.0, False), (90.0, 1.0, 0.0, 0.0, False), (0.0, 1.0, 0.0, 0.0, True), (25.0, 0.8, 0.1, -0.05, False),
             (-140.0, 1.3, -0.2, 0.15, True), (7.0, 0.6, 0.0, 0.3, False)]
    fwd = np.array([AO.forward(*c, (HS, WS)) for c in cases]).reshape(3, 2, 2, 3)
    return torch.from_numpy(store).to(dev), torch.from_numpy(uv).to(dev), fwd


def _xf(fwd, dst, dev):
    xf = np.array([[AO.inverse(fwd[b, s], (HS, WS), dst) for s in range(2)] for b in range(3)]).reshape(3, 2, 6)
    return torch.from_numpy(np.ascontiguousarray(xf)).to(dev)


@pytest.mark.parametrize("out", [None, (24, 20), (192, 200)], ids=lambda o: "plain" if o is None else "%dx%d" % o)
def test_slot_fed_is_the_batch_fed_pass_bit_for_bit(dev, small_store, out):
    from mmhand_amd import ops
    store, uv, fwd = small_store
    xf = _xf(fwd, out or (HS, WS), dev)
    idx = torch.tensor(IDX, dtype=torch.int32, device=dev)
    i = [idx[:, j].long() for j in range(4)]
    want = ops.decode_inputs_affine(store[i[0]], store[i[1]], store[i[2]], store[i[3]], uv[:, 0].contiguous(),
                                    uv[:, 1].contiguous(), xf, out_size=out)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    got = ops.decode_inputs_indexed_affine(store, idx, uv, xf, out_size=out, status=status)
    torch.cuda.synchronize()
    assert int(status) == 0
    Ho, Wo = out or (HS, WS)
    for name, g, w, c in zip(("x_h1", "x_h2", "x_p", "x_d"), got, want, (4, 4, 44, 8)):
        assert tuple(g.shape) == (3, Ho, Wo, c) and g.dtype == torch.float32, name
        assert torch.equal(g, w), name
    assert float(got[2].abs().sum()) > 0 and float(got[0].abs().sum()) > 0


@pytest.mark.parametrize("bad", [S, -1, 2 ** 31 - 1], ids=["S", "-1", "int max"])
def test_a_slot_outside_the_store_costs_its_sample_and_a_status_bit(dev, small_store, bad):
    """the sample with the bad slot is zeros in all four outputs, status bit 1 is set, its neighbours are what they were"""
    from mmhand_amd import ops
    store, uv, fwd = small_store
    xf = _xf(fwd, (24, 20), dev)
    idx = torch.tensor(IDX, dtype=torch.int32, device=dev)
    want = ops.decode_inputs_indexed_affine(store, idx, uv, xf, out_size=(24, 20))
    broken = idx.clone()
    broken[1, 2] = bad
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    got = ops.decode_inputs_indexed_affine(store, broken, uv, xf, out_size=(24, 20), status=status)
    torch.cuda.synchronize()
    assert int(status) == 1
    for g, w in zip(got, want):
        assert not g[1].any() and w[1].any()
        assert torch.equal(g[0], w[0]) and torch.equal(g[2], w[2])
    got = ops.decode_inputs_indexed_affine(store, broken, uv, xf, out_size=(24, 20))        # status is optional
    assert not got[2][1].any() and torch.equal(got[2][0], want[2][0])


# ----------------------------------------------------------------------------- end to end on a prepared directory
def _opt(**kw):
    from mmhand_amd.options import default_train_opt
    args = dict(batchSize=2, ngf=SM["ngf"], ndf=SM["ndf"], n_layers_D=SM["n_layers_D"], G_n_blocks=SM["n_blocks"], norm="instance",
                no_dropout=True, no_dropout_D=True, pool_size=2, name="augment", checkpoints_dir="/tmp/mmh_augment_ckpt",
                local_rank=0, dataset="rhd", augmentation_ratio=1.0, nThreads=2, resize_inputs=64, augment_geom=True,
                aug_pair="independent", aug_flip=0.5)
    args.update(kw)
    return default_train_opt(**args)


@pytest.fixture(scope="module")
def rhd_dir():
    """a prepared directory of 32 x 32 files (its path must not contain "test": generic_dataset.py:116 keys on that)"""
    from tests._dataset_fixture import write_rhd
    d = tempfile.mkdtemp(prefix="mmh_ag_")
    root = os.path.join(d, "rhd")
    write_rhd(root, n=8, size=32)
    yield root
    shutil.rmtree(d, ignore_errors=True)


DECODED = ("H1", "H2", "P1", "P2", "D1", "D2", "C1", "C2")


def _loader(root, dev, **kw):
    from mmhand_amd.data import HandFolderLoader
    lkw = {k: kw.pop(k) for k in ("decoded", "resident") if k in kw}
    random.seed(5)
    return HandFolderLoader(_opt(dataroot=root, **kw), device=dev, **lkw)


def _epoch(ld, epoch):
    ld.set_epoch(epoch)
    return [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()} for b in ld]


def test_epochs_differ_and_an_epoch_repeats(rhd_dir, dev):
    ld = _loader(rhd_dir, dev, decoded=True)
    e0, e1, e0_again = _epoch(ld, 0), _epoch(ld, 1), _epoch(ld, 0)
    assert len(e0) == 4 and tuple(e0[0]["H1"].shape) == (2, 3, 64, 64)
    for a, b, c in zip(e0, e1, e0_again):
        assert a["H1_path"] == b["H1_path"] == c["H1_path"]        # the order and the pairs stay what they are
        for k in DECODED:
            assert torch.equal(a[k], c[k]), k
            assert not torch.equal(a[k], b[k]), k
        assert torch.equal(a["C1"][..., 2], b["C1"][..., 2])        # depth is not transformed
    # the raw form carries the matrices, and shared pairs carry one per pair
    raw = _epoch(_loader(rhd_dir, dev, aug_pair="shared"), 0)
    assert tuple(raw[0]["xf"].shape) == (2, 2, 6) and raw[0]["xf"].dtype == torch.float64
    assert tuple(raw[0]["img1"].shape) == (2, 32, 32, 3)            # the raw batch stays at the files' size
    assert all(torch.equal(b["xf"][:, 0], b["xf"][:, 1]) for b in raw)


def test_file_fed_and_resident_loader_agree_bit_for_bit(rhd_dir, dev):
    """the same epoch number through the files and through the store (in the store's second epoch): decoded tensors and
    C1 / C2 to the bit, in the decoded form of the loaders and through MMHandModel.set_input on their raw forms"""
    from mmhand_amd.mmhand_model import MMHandModel
    files = _epoch(_loader(rhd_dir, dev, decoded=True), 1)
    res = _loader(rhd_dir, dev, decoded=True, resident=True)
    assert res.resident_state.startswith("on")
    first = _epoch(res, 0)
    second = _epoch(res, 1)
    assert all(res._batch_is_resident(g) for g in range(4))
    for f, a, b in zip(files, first, second):
        assert f["H1_path"] == b["H1_path"] and f["H2_path"] == b["H2_path"]
        for k in DECODED:
            assert torch.equal(f[k], b[k]), k
            assert not torch.equal(a[k], b[k]), k                  # the store's second epoch is NOT its first again
    raw_files = _epoch(_loader(rhd_dir, dev), 1)
    raw_res = _loader(rhd_dir, dev, resident=True)
    _epoch(raw_res, 0)
    raw_second = _epoch(raw_res, 1)
    assert all("resident" in b and b["resident"].xf is not None for b in raw_second) and "xf" in raw_files[1]
    model = MMHandModel(_opt(dataroot=rhd_dir))
    kept = []
    for batch in (raw_files[1], raw_second[1]):
        model.set_input(batch)
        kept.append({k: getattr(model, k).clone() for k in ("x_H1", "x_H2", "x_P", "x_D", "input_C1", "input_C2")})
    for k in kept[0]:
        assert torch.equal(kept[0][k], kept[1][k]), k
    assert torch.equal(model.input_H1, files[1]["H1"]) and torch.equal(model.input_P2, files[1]["P2"])
    assert torch.equal(model.input_C1, files[1]["C1"])


def _oracle_batch(b, size):
    """the batch dict of decoded tensors (NCHW fp32 on the host) the float64 oracle makes of a raw augmented batch"""
    out = {}
    xf = b["xf"].cpu().numpy()
    for j, s in enumerate(("1", "2")):
        img, dep, uv = (b[k + s].cpu().numpy() for k in ("img", "dep", "uv"))
        n = img.shape[0]
        hd = [AO.decode_affine(img[i], dep[i], xf[i, j].reshape(2, 3), size, size) for i in range(n)]
        out["H" + s] = torch.from_numpy(np.stack([h for h, _ in hd]).astype(np.float32))
        out["D" + s] = torch.from_numpy(np.stack([np.stack([d, d, d]) for _, d in hd]).astype(np.float32))
        out["P" + s] = torch.from_numpy(np.stack([O.pose_heatmaps(uv[i], size, size) for i in range(n)]))
    return out


def test_step_on_an_augmented_batch_equals_step_on_the_oracles_tensors(rhd_dir, dev):
    """one optimize_parameters() on a raw augmented 32 x 32 batch under --resize_inputs 64 == the same step fed the tensors
    the float64 oracle makes of that batch's files, matrices and joints (rtol 1e-6 on the six losses, the bar
    test_resize_inputs_gpu.py holds the resize to); the joints the loader hands out are the independent builders'"""
    from mmhand_amd.mmhand_model import MMHandModel
    ld = _loader(rhd_dir, dev)
    ld.set_epoch(2)
    b = list(ld)[1]
    assert tuple(b["img1"].shape) == (2, 32, 32, 3) and tuple(b["xf"].shape) == (2, 2, 6)
    # the loader's own numbers against the oracle's builders: draws -> forward -> matrix and joints
    d = ld._draws()
    for i, item in enumerate(ld.indices()[2:4]):
        lab = ld.pose_of(ld.image_target[item])
        fwd = AO.forward(*d[ld.aug_item[item], 1], (32, 32))
        assert np.abs(b["xf"][i, 1].cpu().numpy().reshape(2, 3) - AO.inverse(fwd, (32, 32), (64, 64))).max() < 1e-12
        assert np.abs(b["C2"][i].cpu().numpy() - AO.joints(lab, fwd, (32, 32), (64, 64))).max() < 1e-10
        assert np.array_equal(b["C2"][i, :, :2].cpu().numpy(), b["uv2"][i].cpu().numpy())
    model = MMHandModel(_opt(dataroot=rhd_dir))
    model.set_input(b)
    assert tuple(model.input_H1.shape) == (2, 3, 64, 64) and tuple(model.x_D.shape) == (2, 64, 64, 8)
    assert torch.equal(model.input_C1, b["C1"]) and torch.equal(model.input_C2, b["C2"])    # taken as given
    random.seed(9)
    model.optimize_parameters()
    l_flag = [float(v) for v in model.get_current_errors().values()]
    model2 = MMHandModel(_opt(dataroot=rhd_dir, resize_inputs=0, augment_geom=False))
    model2.set_input(_oracle_batch(b, 64))
    random.seed(9)
    model2.optimize_parameters()
    l_orc = [float(v) for v in model2.get_current_errors().values()]
    print("losses with the flag", l_flag, "on the oracle's tensors", l_orc)
    assert len(l_flag) == 6 and np.allclose(l_flag, l_orc, rtol=1e-6), (l_flag, l_orc)
    assert all(np.isfinite(l_flag))


def _run_graph(opt, batches, n_iter, capture, monkeypatch):
    """tests/test_graph_step_gpu.py's _run on raw augmented batches of the prepared directory"""
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
    """--graph_step --augment_geom on raw augmented batches: captured-and-replayed == the same form run eagerly, all
    losses, weights and the generated image to the bit.  Six iterations: the first four end with the capture itself, the
    two behind it go through set_input's replay branch - the affine decode in front of the replay"""
    kw = dict(dataroot=rhd_dir, graph_step=True, no_dropout=False, no_dropout_D=False, pool_size=3, name="augment_graph")
    batches = _epoch(_loader(rhd_dir, dev), 1)
    assert len(batches) == 4 and all("xf" in b for b in batches)
    eager, l0, s0 = _run_graph(_opt(**kw), batches, 6, False, monkeypatch)
    assert eager._graph is None and eager.graph_replays == 0
    graph, l1, s1 = _run_graph(_opt(**kw), batches, 6, True, monkeypatch)
    assert graph.graph_error is None, graph.graph_error
    assert graph._graph is not None and graph.graph_replays == 6 - graph._graph_warm >= 3
    assert np.array_equal(np.array(l0), np.array(l1)), (l0, l1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    assert tuple(s1["fake"].shape) == (2, 3, 64, 64) and all(np.isfinite(l1[-1]))


def test_without_the_flag_the_batches_are_what_they_were(rhd_dir, dev):
    """flag off: no matrices travel, set_epoch changes nothing, and the decoded form is ops.decode_inputs on the raw batch"""
    from mmhand_amd import ops
    raw = _loader(rhd_dir, dev, augment_geom=False)
    dec = _loader(rhd_dir, dev, augment_geom=False, decoded=True)
    assert raw.augment is None
    r0, d0, d1 = _epoch(raw, 0), _epoch(dec, 0), _epoch(dec, 1)
    for r, a, b in zip(r0, d0, d1):
        assert "xf" not in r
        xh1, xh2, xp, xd = ops.decode_inputs(r["img1"], r["img2"], r["dep1"], r["dep2"], r["uv1"], r["uv2"], out_size=64)
        v = ops.nhwc_to_nchw_view
        want = {"H1": v(xh1, 3), "H2": v(xh2, 3), "P1": v(xp)[:, :21], "P2": v(xp)[:, 21:42], "D1": v(xd)[:, :3], "D2": v(xd)[:, 3:6],
                "C1": ops.resize_joints(r["C1"], (32, 32), (64, 64)), "C2": ops.resize_joints(r["C2"], (32, 32), (64, 64))}
        for k in DECODED:
            assert torch.equal(a[k], want[k]) and torch.equal(b[k], want[k]), k
