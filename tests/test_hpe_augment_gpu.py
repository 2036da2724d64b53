"""train_hpe --augment_geom / --augment_color on the device: mmh_hpe_augment_normalize (csrc/hpe_augment.hip) against the float64
restatement of its definition (tests/_hpe_augment_oracle.py) - bit for bit where the definition is exact (identity, integer
shifts, flips, quarter turns, channel permutations, powers of two), within the oracle's derived tolerance elsewhere - and the
driver end to end.  The reduction's grid is capped at 64 chunks of 256 pixels per image: the 136 x 128 cases give a lane a
second turn of its loop.  All weights are generated: no figure here says anything about a trained estimator."""
import os

import numpy as np
import pytest
import torch

from tests import _affine_oracle as AO
from tests import _hpe_augment_oracle as HO
from tests import _hpe_oracle as O

pytestmark = pytest.mark.gpu
NARROW_2D = {k: v for k, v in O.NARROW.items() if k != "fc"}
SWAP_RB = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(dev, img, A=None, cm=None, gamma=None, out=None):
    """img uint8 [B,H,W,3]; A [B,2,3], cm [B,3,3], gamma [B] numpy or None -> numpy fp32 [B,Ho,Wo,3]; lane 3 is checked here"""
    from mmhand_amd import ops

    def t(a, n):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(len(img), n))).to(dev)

    y = ops.hpe_augment_normalize(torch.from_numpy(np.ascontiguousarray(img)).to(dev), t(A, 6), t(cm, 9),
                                  None if gamma is None else t(gamma, 1).reshape(-1), out_size=out)
    y = y.cpu().numpy()
    Ho, Wo = out or img.shape[1:3]
    assert y.shape == (len(img), Ho, Wo, 4) and y.dtype == np.float32
    assert not y[..., 3].any()                                              # lane 3: zero everywhere
    return y[..., :3]


def plain(img):
    """numpy's min-max normalisation of uint8 [B,H,W,3] BGR bytes -> fp32 [B,H,W,3] RGB, one rounding"""
    rgb = img[..., ::-1].astype(np.float64)
    mn, mx = rgb.min(axis=(1, 2, 3), keepdims=True), rgb.max(axis=(1, 2, 3), keepdims=True)
    return ((rgb - mn) / (mx - mn)).astype(np.float32)


def shuffled(img, A, out=None):
    """the bytes an exact matrix (weights 0) picks, edge replicate: uint8 [B,Ho,Wo,3]"""
    Hs, Ws = img.shape[1:3]
    Ho, Wo = out or (Hs, Ws)
    res = []
    for b in range(len(img)):
        sx, sy = AO.coords(A[b], Ho, Wo)
        assert np.array_equal(sx, np.round(sx)) and np.array_equal(sy, np.round(sy))
        res.append(img[b][np.clip(sy, 0, Hs - 1).astype(int), np.clip(sx, 0, Ws - 1).astype(int)])
    return np.stack(res)


# ------------------------------------------------------------------------------------------------- bit-identical cases
@pytest.mark.parametrize("B,H,W_", [(3, 24, 40), (1, 136, 128), (2, 1, 1), (1, 5, 3)])
def test_identity_is_hpe_normalize_bit_for_bit(dev, B, H, W_):
    from mmhand_amd import ops
    img = HO.images(B, H, W_, seed=5)
    want = ops.hpe_normalize(torch.from_numpy(img).to(dev), "bgr_hwc").cpu().numpy()[..., :3]
    eye_a, eye_c = np.tile(HO.IDENTITY, (B, 1, 1)), np.tile(np.eye(3), (B, 1, 1))
    for kw in (dict(), dict(A=eye_a, cm=eye_c, gamma=np.ones(B)), dict(A=eye_a), dict(cm=eye_c), dict(gamma=np.ones(B))):
        got = run(dev, img, **kw)
        assert np.array_equal(_bits(got), _bits(want)), sorted(kw)
    if H * W_ > 1:
        assert np.array_equal(_bits(want), _bits(plain(img)))


def test_integer_shift_flip_and_quarter_turn_are_exact(dev):
    """weights 0: the output is the normalisation of the index-shuffled bytes, edge replicate included; three different
    matrices in one batch (per-image indexing)"""
    from mmhand_amd import ops
    from mmhand_amd.data import affine_forward, affine_inverse
    img = HO.images(3, *HO.SRC, seed=6)
    Ws = HO.SRC[1]
    A = np.array([[[1.0, 0.0, 2.0], [0.0, 1.0, -3.0]],                      # shift (2, -3)
                  [[-1.0, 0.0, Ws - 1.0], [0.0, 1.0, 0.0]],                 # horizontal flip
                  [[1.0, 0.0, -5.0], [0.0, 1.0, 4.0]]])
    src = shuffled(img, A)
    assert np.array_equal(src[1], img[1][:, ::-1]) and np.array_equal(src[0][3:, :-2], img[0][:-3, 2:])
    assert np.array_equal(src[0][0, :-2], img[0][0, 2:]) and np.array_equal(src[0][5, -1], img[0][2, -1])     # replicated edges
    got = run(dev, img, A)
    assert np.array_equal(_bits(got), _bits(plain(src)))
    want = ops.hpe_normalize(torch.from_numpy(src).to(dev), "bgr_hwc").cpu().numpy()[..., :3]
    assert np.array_equal(_bits(got), _bits(want))
    # quarter turns on a square image, both ways, from the host's own builders
    sq = HO.images(2, 24, 24, seed=7)
    A = np.stack([affine_inverse(affine_forward(t, 1.0, 0.0, 0.0, False, (24, 24)), (24, 24)) for t in (90.0, -90.0)])
    src = shuffled(sq, A)
    assert sorted(np.array_equal(src[0], np.rot90(sq[0], k)) for k in (1, 3)) == [False, True]
    assert np.array_equal(_bits(run(dev, sq, A)), _bits(plain(src)))


def test_exact_colour_matrices(dev):
    from mmhand_amd import ops
    img = HO.images(3, *HO.SRC, seed=8)
    # the R <-> B permutation: the normalisation of the channel-swapped image
    got = run(dev, img, cm=np.tile(SWAP_RB, (3, 1, 1)))
    swapped = np.ascontiguousarray(img[..., ::-1])
    assert np.array_equal(_bits(got), _bits(plain(swapped)))
    want = ops.hpe_normalize(torch.from_numpy(swapped).to(dev), "bgr_hwc").cpu().numpy()[..., :3]
    assert np.array_equal(_bits(got), _bits(want))
    # 2 I on bytes above 127: the clamp at 255 is reached; per-image indexing: image 1 keeps the identity, image 2 gets 0.5 I
    img = HO.images(3, *HO.SRC, seed=9, lo=40, hi=256)
    assert (img > 127).any() and (img < 127).any()
    scale = np.array([2.0, 1.0, 0.5])
    v = np.minimum(img[..., ::-1].astype(np.float64) * scale[:, None, None, None], 255.0)
    assert (v[0] == 255.0).sum() > 100
    mn, mx = v.min(axis=(1, 2, 3), keepdims=True), v.max(axis=(1, 2, 3), keepdims=True)
    got = run(dev, img, cm=scale[:, None, None] * np.eye(3))
    assert np.array_equal(_bits(got), _bits(((v - mn) / (mx - mn)).astype(np.float32)))


def test_constant_image_gives_zeros(dev):
    """mx == mn: zeros, not 0 / 0.  [Under a general warp the four-tap sum of equal bytes c may round one ulp beside c, and a
    matrix with gains gives the three channels of a grey image three values: those are no constant images any more.]"""
    img = np.full((2, 7, 9, 3), 200, dtype=np.uint8)
    img[1] = 0
    mix = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5]])    # exact on equal channels: every row sums to 1
    for kw in (dict(), dict(gamma=np.array([0.8, 1.25])), dict(cm=np.tile(mix, (2, 1, 1)), gamma=np.array([1.25, 1.0]))):
        assert not run(dev, img, **kw).any()
    # an all-zero image stays constant under any warp and matrix
    A = np.stack([AO.inverse(AO.forward(*d, (7, 9)), (7, 9), (7, 9)) for d in HO.DRAWS[:2]])
    zero = np.zeros_like(img)
    assert not run(dev, zero, A=A, cm=np.stack([HO.matrix(*c) for c in HO.COLORS[:2]]), gamma=np.array([0.8, 1.25])).any()


def test_min_and_max_are_taken_over_the_output_not_the_source(dev):
    """the source's only 255 and only 0 sit in a corner that a zoom by 2 about the centre never samples"""
    H, W_ = HO.SRC
    img = HO.images(1, H, W_, seed=10, lo=60, hi=200)
    img[0, 0, 0], img[0, 0, 1] = 255, 0
    A = AO.inverse(AO.forward(0.0, 2.0, 0.0, 0.0, False, HO.SRC), HO.SRC, HO.SRC)
    sx, sy = AO.coords(A, H, W_)
    assert sx.min() > 2 and sy.min() > 2 and sx.max() < W_ - 3 and sy.max() < H - 3
    want, tol, rng = HO.tolerance(img[0], A=A)
    assert HO.MIN_RANGE <= rng < 140.0
    got = run(dev, img, A[None])[0]
    assert (np.abs(got.astype(np.float64) - want) <= tol).all()
    assert got.min() == 0.0 and got.max() == 1.0                            # the sampled range is the whole of [0, 1]
    # under the source's range (255) nothing would reach either end
    src_range = (HO.values(img[0], A=A) - 0.0) / 255.0
    assert src_range.min() > 0.2 and src_range.max() < 0.8


# ------------------------------------------------------------------------------------------------- toleranced cases
CASES = HO.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_general_matrices_colours_and_gamma_stay_within_the_oracles_tolerance(dev, case):
    name, img, A, cm, gamma, out = case
    oracle = []
    for b in range(len(img)):
        want, tol, rng = HO.tolerance(img[b], A=None if A is None else A[b], cm=None if cm is None else cm[b],
                                      gamma=None if gamma is None else gamma[b], out=out)
        assert rng >= HO.MIN_RANGE, (name, b, rng)                          # the condition comes first
        oracle.append((want, tol))
    got = run(dev, img, A, cm, gamma, None if tuple(out) == tuple(img.shape[1:3]) else out)
    worst, off = 0.0, 0
    for b, (want, tol) in enumerate(oracle):
        err = np.abs(got[b].astype(np.float64) - want.astype(np.float64))
        worst = max(worst, float((err / tol).max()))
        off += int((_bits(got[b]) != _bits(want)).sum())
    print("%s: largest error / tolerance %.3f; elements not bit-equal to the rounded oracle: %d of %d" % (name, worst, off, got.size))
    for b, (want, tol) in enumerate(oracle):
        err = np.abs(got[b].astype(np.float64) - want.astype(np.float64))
        assert (err <= tol).all(), (name, b, float((err - tol).max()), np.argwhere(err > tol)[:4])
    # two launches on the same inputs: the same bits
    assert np.array_equal(_bits(run(dev, img, A, cm, gamma, None if tuple(out) == tuple(img.shape[1:3]) else out)), _bits(got))


def test_label_and_pixels_move_together_through_the_kernel(dev):
    from mmhand_amd.data import affine_forward, affine_inverse, affine_joints
    H, W_ = HO.SRC
    for (u, v), dst in (((22, 11), (H, W_)), ((9, 15), (H, W_)), ((22, 11), (16, 24))):
        fwd = affine_forward(20.0, 1.1, 0.05, -0.04, True, (H, W_))
        A = affine_inverse(fwd, (H, W_), dst)
        got = run(dev, HO.blob_image(H, W_, u, v)[None], A[None], out=None if dst == (H, W_) else dst)[0]
        ju, jv = affine_joints(np.array([[float(u), float(v)]]), fwd, (H, W_), dst)[0]
        ys, xs = np.nonzero(got[..., 0] == got[..., 0].max())
        assert got.max() > 0.5 and abs(xs.mean() - ju) <= 1.0 and abs(ys.mean() - jv) <= 1.0, (u, v, dst, ju, jv, xs, ys)


def test_ops_argument_checks(dev):
    from mmhand_amd import ops
    img = torch.from_numpy(HO.images(2, 8, 8, seed=1)).to(dev)
    with pytest.raises(ValueError, match="uint8"):
        ops.hpe_augment_normalize(img.float())
    with pytest.raises(ValueError, match="needs xf"):
        ops.hpe_augment_normalize(img, out_size=(4, 4))
    for kw in (dict(xf=torch.zeros((2, 6), device=dev)), dict(xf=torch.zeros((3, 6), dtype=torch.float64, device=dev)),
               dict(cm=torch.zeros((2, 3), dtype=torch.float64, device=dev)), dict(gamma=torch.ones(2, dtype=torch.float64))):
        with pytest.raises(AssertionError):
            ops.hpe_augment_normalize(img, **kw)


# ------------------------------------------------------------------------------------------------- the command line
@pytest.fixture(scope="module")
def roots():
    """prepared directories of 32 x 32 files under a path that does not contain "test" (the loader keys on it)"""
    import shutil
    import tempfile
    from tests._dataset_fixture import write_rhd
    d = tempfile.mkdtemp(prefix="mmh_hpa_")
    assert "test" not in d
    root, val = os.path.join(d, "rhd"), os.path.join(d, "val")
    write_rhd(root, n=6, size=32)
    write_rhd(val, n=3, size=32, seed=10)
    yield d, root, val
    shutil.rmtree(d, ignore_errors=True)


def _train(roots, monkeypatch, widths, name, *extra, epochs=2):
    from mmhand_amd import train_hpe
    d, root, _ = roots
    monkeypatch.chdir(d)
    monkeypatch.setattr(train_hpe, "INIT_WIDTHS", widths)
    return train_hpe.main(["--dataroot", root, "--dataset", "rhd", "--name", name, "--niter", "1", "--niter_decay", str(epochs - 1),
                           "--batchSize", "4", "--init_seed", "3", "--threads", "2"] + list(extra))


def _count_calls(monkeypatch):
    from mmhand_amd import ops
    seen, real = [], ops.hpe_augment_normalize

    def spy(images, xf=None, cm=None, gamma=None, out_size=None):
        seen.append((tuple(images.shape), images.dtype, xf is not None, cm is not None, gamma is not None))
        return real(images, xf, cm, gamma, out_size)

    monkeypatch.setattr(ops, "hpe_augment_normalize", spy)
    return seen


def test_train_hpe_with_both_flags(dev, roots, monkeypatch):
    import json
    from mmhand_amd import hpe_train
    both = ["--augment_geom", "--augment_color"]
    seen = _count_calls(monkeypatch)
    first = _train(roots, monkeypatch, NARROW_2D, "a", *both)
    # 6 images in batches of 4, two epochs: four training batches through the new pass, bytes as the loader reads them
    assert [s[0] for s in seen] == [(4, 32, 32, 3), (2, 32, 32, 3)] * 2 and all(s[1:] == (torch.uint8, True, True, True) for s in seen)
    assert len(first) == 2 and all(np.isfinite(r["loss"]).all() and r["images"] == 6 for r in first)
    assert _train(roots, monkeypatch, NARROW_2D, "b", *both) == first                       # the same seeds: the same log, bit for bit
    off = _train(roots, monkeypatch, NARROW_2D, "c")
    assert len(seen) == 8 and off[0]["loss"] != first[0]["loss"] and off[1]["loss"] != first[1]["loss"]
    other = _train(roots, monkeypatch, NARROW_2D, "d", *both, "--aug_seed", "1")
    assert other[0]["loss"] != first[0]["loss"] and np.isfinite(other[1]["loss"]).all()
    opts = json.load(open(os.path.join(roots[0], "checkpoints", "d", "train_hpe_log.json")))["options"]
    assert opts["augment_geom"] is True and opts["augment_color"] is True and opts["aug_seed"] == 1 and opts["aug_hue"] == 10.0
    # either switch alone changes the run too, and each differently
    geom = _train(roots, monkeypatch, NARROW_2D, "e", "--augment_geom", epochs=1)
    color = _train(roots, monkeypatch, NARROW_2D, "f", "--augment_color", epochs=1)
    assert len({tuple(r[0]["loss"]) for r in (first, off, geom, color)}) == 4
    assert seen[-1][2:] == (False, True, True) and seen[-3][2:] == (True, False, False)
    # validation is never augmented: with the weights held at their initial values the first epoch's figures do not see the flags
    monkeypatch.setattr(hpe_train._PoseTrainer, "_adam", lambda self, lr: None)
    n = len(seen)
    on = _train(roots, monkeypatch, NARROW_2D, "g", *both, "--val_dataroot", roots[2], epochs=1)
    assert len(seen) == n + 2                                                               # the two training batches, no more
    plain_run = _train(roots, monkeypatch, NARROW_2D, "h", "--val_dataroot", roots[2], epochs=1)
    keys = ("pck2d_auc", "epe2d_mean", "epe2d_median")
    assert [on[0][k] for k in keys] == [plain_run[0][k] for k in keys] and on[0]["loss"] != plain_run[0]["loss"]


def test_train_hpe_hpm3d_moves_the_joints(dev, roots, monkeypatch):
    from mmhand_amd import data, hpe_train
    common = ["--net", "hpm3d", "--lr", "2e-4", "--beta1", "0.5"]
    reads, read = [], data._read_bgr
    monkeypatch.setattr(data, "_read_bgr", lambda p: reads.append(p) or read(p))
    first = _train(roots, monkeypatch, O.NARROW, "t", *common, "--augment_geom")
    assert reads == []                                                      # --heat_source target: still no image file
    assert len(first) == 2 and np.isfinite([r["loss"] for r in first]).all()
    assert _train(roots, monkeypatch, O.NARROW, "u", *common, "--augment_geom") == first
    off = _train(roots, monkeypatch, O.NARROW, "v", *common)
    assert off[0]["loss"] != first[0]["loss"]
    assert _train(roots, monkeypatch, O.NARROW, "w", *common, "--augment_geom", "--aug_seed", "1")[0]["loss"] != first[0]["loss"]
    # --heat_source predicted: the augmented images feed the 2D machine (both switches), the depth labels stay
    h2 = os.path.join(roots[0], "h2.pth")
    torch.save(hpe_train.init_state_dict(5, NARROW_2D), h2)
    seen = _count_calls(monkeypatch)
    pred = ["--heat_source", "predicted", "--hpm2d", h2]
    on = _train(roots, monkeypatch, O.NARROW, "x", *common, *pred, "--augment_geom", "--augment_color", epochs=1)
    assert [s[0] for s in seen] == [(4, 32, 32, 3), (2, 32, 32, 3)] and np.isfinite(on[0]["loss"])
    assert _train(roots, monkeypatch, O.NARROW, "y", *common, *pred, epochs=1)[0]["loss"] != on[0]["loss"]
    # validation is not augmented: initial weights, the same validation loss with and without the flag
    monkeypatch.setattr(hpe_train._PoseTrainer, "_adam", lambda self, lr: None)
    a = _train(roots, monkeypatch, O.NARROW, "z", *common, "--augment_geom", "--val_dataroot", roots[2], epochs=1)
    b = _train(roots, monkeypatch, O.NARROW, "zz", *common, "--val_dataroot", roots[2], epochs=1)
    assert a[0]["val_L_z"] == b[0]["val_L_z"] and a[0]["loss"] != b[0]["loss"]
