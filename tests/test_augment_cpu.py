"""--augment_geom without a GPU: the float64 oracle of the sampling rule (tests/_affine_oracle.py) against
F.grid_sample, the host's matrix maths (data.affine_forward / affine_inverse / affine_joints) against the oracle's
independent builders, the draws, the options' validation, and the new entry points' argument checks."""
import ctypes
import fnmatch
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import _affine_oracle as AO
from tests import _resize_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mmh_decode_inputs_affine": 18, "mmh_decode_inputs_indexed_affine": 17}
HS, WS = 12, 10


def _random_matrix(rs, src, dst):
    fwd = AO.forward(rs.uniform(-180, 180), rs.uniform(0.5, 1.6), rs.uniform(-0.4, 0.4), rs.uniform(-0.4, 0.4),
                     rs.rand() < 0.5, src)
    return AO.inverse(fwd, src, dst)


# ----------------------------------------------------------------------------- the oracle against grid_sample
def test_oracle_equals_grid_sample_float64():
    """warp == F.grid_sample(bilinear, border, align_corners=True) on pixel coordinates, in float64, to 1e-9 on raw values
    <= 767; 200 random matrices (rotation, scale 0.5 - 1.6, flips, shifts, resize ratios folded in), many samples outside"""
    rs = np.random.RandomState(11)
    worst, shares = 0.0, []
    for trial in range(200):
        Ho, Wo = [(12, 10), (24, 20), (8, 4), (17, 23)][trial % 4]
        A = _random_matrix(rs, (HS, WS), (Ho, Wo))
        a = rs.randint(0, 768, size=(3, HS, WS)).astype(np.float64)
        got = AO.warp(a, A, Ho, Wo)
        sx, sy = AO.coords(A, Ho, Wo)
        grid = torch.from_numpy(np.stack([2.0 * sx / (WS - 1) - 1.0, 2.0 * sy / (HS - 1) - 1.0], -1))[None]
        want = torch.nn.functional.grid_sample(torch.from_numpy(a)[None], grid, mode="bilinear", padding_mode="border",
                                               align_corners=True)[0].numpy()
        worst = max(worst, float(np.abs(got - want).max()))
        shares.append(AO.outside_share(A, (HS, WS), (Ho, Wo)))
    print(f"oracle vs grid_sample: max difference {worst:.3e}; outside share {min(shares):.2f} .. {max(shares):.2f}")
    assert worst <= 1e-9
    assert max(shares) > 0.5 and np.mean(shares) > 0.1             # the clamp is exercised


def test_oracle_identity_and_nan():
    rs = np.random.RandomState(3)
    a = rs.randint(0, 768, size=(HS, WS)).astype(np.float64)
    assert np.array_equal(AO.warp(a, [[1, 0, 0], [0, 1, 0]], HS, WS), a)
    # a NaN coordinate lands on 0: the corner pixel, never an index outside
    assert np.array_equal(AO.warp(a, [[np.nan, 0, 0], [0, np.nan, 0]], 3, 3), np.full((3, 3), a[0, 0]))
    # identity with the resize folded in is the resize oracle (its taps only clamp below; above, the weight is 0 anyway)
    for dst in ((24, 20), (8, 4)):
        A = AO.inverse(AO.forward(0.0, 1.0, 0.0, 0.0, False, (HS, WS)), (HS, WS), dst)
        assert np.abs(AO.warp(a, A, *dst) - RO.bilinear(a, *dst)).max() < 1e-9


# ----------------------------------------------------------------------------- data.py's matrices
def _cases(rs, n):
    return [(rs.uniform(-180, 180), rs.uniform(0.5, 1.6), rs.uniform(-0.3, 0.3), rs.uniform(-0.3, 0.3), bool(rs.rand() < 0.5))
            for _ in range(n)] + [(0.0, 1.0, 0.0, 0.0, False), (90.0, 1.0, 0.0, 0.0, False), (-90.0, 0.7, 0.1, 0.0, True)]


def test_matrices_agree_with_the_independent_builders():
    from mmhand_amd.data import affine_forward, affine_inverse, affine_joints
    rs = np.random.RandomState(5)
    uv = rs.uniform(-4, 16, size=(21, 3))
    for case in _cases(rs, 40):
        for dst in ((HS, WS), (24, 20), (8, 4)):
            fwd = affine_forward(*case, (HS, WS))
            assert fwd.shape == (2, 3) and np.abs(fwd - AO.forward(*case, (HS, WS))).max() < 1e-12
            assert np.abs(affine_inverse(fwd, (HS, WS), dst) - AO.inverse(fwd, (HS, WS), dst)).max() < 1e-12
            got = affine_joints(uv, fwd, (HS, WS), dst)
            assert np.abs(got - AO.joints(uv, fwd, (HS, WS), dst)).max() < 1e-11
            assert np.array_equal(got[:, 2], uv[:, 2])                                     # depth unchanged


def test_inverse_after_forward_is_the_identity_on_joints():
    from mmhand_amd.data import affine_forward, affine_inverse, affine_joints
    rs = np.random.RandomState(6)
    uv = rs.uniform(-4, 16, size=(21, 2))
    for case in _cases(rs, 40):
        for dst in ((HS, WS), (24, 20), (8, 4)):
            fwd = affine_forward(*case, (HS, WS))
            A = affine_inverse(fwd, (HS, WS), dst)
            out = affine_joints(uv, fwd, (HS, WS), dst)
            back = np.stack([A[0, 0] * out[:, 0] + A[0, 1] * out[:, 1] + A[0, 2], A[1, 0] * out[:, 0] + A[1, 1] * out[:, 1] + A[1, 2]], -1)
            assert np.abs(back - uv).max() < 1e-12, case


def test_broadcasting_equals_one_at_a_time_bit_for_bit():
    """a whole epoch's table and one sample's matrices are the same numbers: the resident path and the file path agree"""
    from mmhand_amd.data import affine_forward, affine_inverse, affine_joints
    rs = np.random.RandomState(8)
    d = np.stack([rs.uniform(-30, 30, (7, 2)), rs.uniform(0.8, 1.2, (7, 2)), rs.uniform(-0.1, 0.1, (7, 2)),
                  rs.uniform(-0.1, 0.1, (7, 2)), rs.rand(7, 2) < 0.5], -1)
    uv = rs.uniform(0, 32, size=(7, 2, 21, 3))
    fwd = affine_forward(d[..., 0], d[..., 1], d[..., 2], d[..., 3], d[..., 4], (32, 32))
    inv, j = affine_inverse(fwd, (32, 32), (64, 64)), affine_joints(uv, fwd, (32, 32), (64, 64))
    assert fwd.shape == (7, 2, 2, 3) and inv.shape == (7, 2, 2, 3) and j.shape == uv.shape
    for i in range(7):
        for s in range(2):
            f1 = affine_forward(*d[i, s], (32, 32))
            assert np.array_equal(f1, fwd[i, s])
            assert np.array_equal(affine_inverse(f1, (32, 32), (64, 64)), inv[i, s])
            assert np.array_equal(affine_joints(uv[i, s], f1, (32, 32), (64, 64)), j[i, s])


def test_quarter_turn_puts_a_bright_pixel_on_its_transformed_joint():
    from mmhand_amd.data import affine_forward, affine_inverse, affine_joints
    a = np.zeros((9, 9))
    a[2, 6] = 255.0                                                 # (u, v) = (6, 2)
    fwd = affine_forward(90.0, 1.0, 0.0, 0.0, False, (9, 9))
    assert np.array_equal(fwd, [[0.0, -1.0, 8.0], [1.0, 0.0, 0.0]])  # exact: no 6e-17 where cos(90 degrees) belongs
    u, v = affine_joints(np.array([[6.0, 2.0]]), fwd, (9, 9))[0]
    assert (u, v) == (6.0, 6.0)
    out = AO.warp(a, affine_inverse(fwd, (9, 9)), 9, 9)
    assert out[int(v), int(u)] == 255.0 and np.count_nonzero(out) == 1


def test_flip_mirrors_u_about_the_centre():
    from mmhand_amd.data import affine_forward, affine_joints
    fwd = affine_forward(0.0, 1.0, 0.0, 0.0, True, (HS, WS))
    uv = np.array([[0.0, 3.0, 7.0], [WS - 1.0, 5.0, 7.0], [2.5, 0.0, 7.0]])
    assert np.array_equal(affine_joints(uv, fwd, (HS, WS)), [[WS - 1.0, 3.0, 7.0], [0.0, 5.0, 7.0], [WS - 1.0 - 2.5, 0.0, 7.0]])


def test_identity_draw_with_the_resize_folded_in_is_resize_joints():
    from mmhand_amd import ops
    from mmhand_amd.data import affine_forward, affine_inverse, affine_joints
    rs = np.random.RandomState(9)
    uv = rs.uniform(-4, 36, size=(5, 21, 3))
    fwd = affine_forward(0.0, 1.0, 0.0, 0.0, False, (32, 32))
    for dst in ((64, 64), (20, 28), (32, 32)):
        assert np.array_equal(affine_joints(uv, fwd, (32, 32), dst), ops.resize_joints(torch.from_numpy(uv), (32, 32), dst).numpy())
    # ... and its sampling matrix is the resize pass's map sx = (x + 0.5) Ws / Wo - 0.5
    A = affine_inverse(fwd, (32, 32), (64, 64))
    assert np.array_equal(A, [[0.5, 0.0, -0.25], [0.0, 0.5, -0.25]])
    assert np.array_equal(np.abs(affine_inverse(fwd, (32, 32))), [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def test_affine_inverse_refuses_what_it_cannot_invert():
    from mmhand_amd.data import affine_inverse
    for bad in (np.nan, np.inf, -np.inf):
        m = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, bad]])
        with pytest.raises(ValueError, match="non-finite"):
            affine_inverse(m, (HS, WS))
    with pytest.raises(ValueError, match="singular"):
        affine_inverse([[1.0, 2.0, 0.0], [2.0, 4.0, 0.0]], (HS, WS))
    with pytest.raises(ValueError, match="singular"):
        affine_inverse(np.zeros((3, 2, 3)), (HS, WS))
    with pytest.raises(ValueError, match="2, 3"):
        affine_inverse(np.eye(3), (HS, WS))


# ----------------------------------------------------------------------------- draws and options
def _aug_opt(**kw):
    d = dict(augment_geom=True, aug_rotate=15.0, aug_scale=0.1, aug_shift=0.05, aug_flip=0.0, aug_pair="shared", aug_seed=0,
             dataroot="/somewhere")
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_augment_draws():
    from mmhand_amd.data import augment_draws
    opt = _aug_opt(aug_pair="independent", aug_flip=0.5, aug_seed=4)
    d0 = augment_draws(50, 0, opt)
    assert d0.shape == (50, 2, 5) and d0.dtype == np.float64
    assert np.array_equal(d0, augment_draws(50, 0, opt))                      # (seed, epoch, item) decides, nothing else
    assert not np.array_equal(d0, augment_draws(50, 1, opt))                  # another epoch, other draws
    assert not np.array_equal(d0, augment_draws(50, 0, _aug_opt(aug_pair="independent", aug_flip=0.5, aug_seed=5)))
    assert not np.array_equal(d0[:, 0], d0[:, 1])                             # independent sides
    assert (np.abs(d0[..., 0]) <= 15.0).all() and (np.abs(d0[..., 1] - 1.0) <= 0.1).all()
    assert (np.abs(d0[..., 2:4]) <= 0.05).all() and set(np.unique(d0[..., 4])) == {0.0, 1.0}
    assert np.abs(d0[..., 0]).max() > 10.0 and np.ptp(d0[..., 1]) > 0.1       # and the ranges are used
    sh = augment_draws(50, 0, _aug_opt(aug_seed=4))
    assert np.array_equal(sh[:, 0], sh[:, 1]) and not sh[..., 4].any()        # shared: one draw; flip probability 0: none
    assert augment_draws(50, 0, _aug_opt(aug_flip=1.0))[..., 4].all()
    zero = augment_draws(9, 3, _aug_opt(aug_rotate=0.0, aug_scale=0.0, aug_shift=0.0))
    assert np.array_equal(zero, np.tile([0.0, 1.0, 0.0, 0.0, 0.0], (9, 2, 1)))


@pytest.fixture
def rhd_root():
    """a prepared directory of 32 x 32 files (its path must not contain "test": generic_dataset.py:116 keys on that)"""
    import shutil
    import tempfile
    from tests._dataset_fixture import write_rhd
    d = tempfile.mkdtemp(prefix="mmh_ag_")
    root = os.path.join(d, "rhd")
    write_rhd(root, n=8, size=32)
    yield root
    shutil.rmtree(d, ignore_errors=True)


def test_draws_reach_the_loader_by_item_whatever_the_batch_size_or_rank(rhd_root):
    """loaders over the same directory with other batch sizes and ranks hand an item the same matrices in an epoch"""
    from mmhand_amd.data import HandFolderLoader
    from mmhand_amd.options import default_train_opt
    root = rhd_root
    seen = []
    for bs, world, rank in ((2, 1, 0), (3, 1, 0), (2, 2, 1)):
        opt = default_train_opt(batchSize=bs, dataroot=root, dataset="rhd", augmentation_ratio=1.0, augment_geom=True,
                                aug_pair="independent", resize_inputs=64, distributed=world > 1, world_size=world)
        import random
        random.seed(5)
        ld = HandFolderLoader(opt, device=torch.device("cpu"))
        ld.rank = rank
        ld.set_epoch(3)
        assert ld.epoch == 0 and ld.aug_epoch == 3                  # indices() does not see the epoch
        rows = {}
        for item in ld.indices():
            s = ld.load_sample(item)
            assert s["xf"].shape == (2, 6) and s["uv1"].shape == (21, 2) and s["C2"].shape == (21, 3)
            rows[item] = np.concatenate([s["xf"].ravel(), s["uv1"].ravel(), s["C2"].ravel()])
        seen.append(rows)
    assert len(seen[0]) == 8 and len(seen[2]) == 4
    for other in seen[1:]:
        for item, row in other.items():
            assert np.array_equal(row, seen[0][item])
    item = next(iter(seen[2]))
    ld.set_epoch(4)
    assert not np.array_equal(ld.load_sample(item)["xf"].ravel(), seen[2][item][:12])      # another epoch, another matrix


def test_check_augment():
    from mmhand_amd.options import TestOptions, TrainOptions, check_augment, default_train_opt
    assert check_augment(types.SimpleNamespace()) is None
    assert check_augment(_aug_opt(augment_geom=False, aug_scale=7.0)) is None   # off: nothing is looked at
    assert check_augment(_aug_opt()) == (15.0, 0.1, 0.05, 0.0, "shared", 0)
    assert check_augment(types.SimpleNamespace(augment_geom=True, dataroot="/d")) == (15.0, 0.1, 0.05, 0.0, "shared", 0)
    for kw in (dict(aug_rotate=-1.0), dict(aug_rotate=181.0), dict(aug_rotate=float("nan")), dict(aug_scale=1.0),
               dict(aug_scale=-0.1), dict(aug_shift=-0.01), dict(aug_shift=1.5), dict(aug_flip=1.1), dict(aug_flip=-0.5),
               dict(aug_flip=float("inf")), dict(aug_pair="both"), dict(aug_seed=-1), dict(aug_seed=1.5), dict(aug_rotate="15"),
               dict(dataroot=None)):
        with pytest.raises(ValueError, match="aug"):
            check_augment(_aug_opt(**kw))
    opt = TrainOptions().parse([], init_dist=False, save=False)
    assert opt.augment_geom is False and (opt.aug_rotate, opt.aug_scale, opt.aug_shift, opt.aug_flip) == (15.0, 0.1, 0.05, 0.0)
    assert opt.aug_pair == "shared" and opt.aug_seed == 0
    opt = TrainOptions().parse(["--augment_geom", "--dataroot", "/d", "--aug_pair", "independent", "--aug_flip", "0.5"],
                               init_dist=False, save=False)
    assert opt.augment_geom is True and opt.aug_pair == "independent" and opt.aug_flip == 0.5
    with pytest.raises(ValueError, match="dataroot"):
        TrainOptions().parse(["--augment_geom"], init_dist=False, save=False)
    with pytest.raises(ValueError, match="aug_scale"):
        TrainOptions().parse(["--augment_geom", "--dataroot", "/d", "--aug_scale", "1.0"], init_dist=False, save=False)
    with pytest.raises(SystemExit):                                 # aug and evaluate do not take it
        TestOptions().parse(["--augment_geom"], init_dist=False, save=False)
    assert default_train_opt().augment_geom is False


# ----------------------------------------------------------------------------- the C-ABI
def test_entry_points_are_declared_and_exported():
    from mmhand_amd import lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmhand_hip.h")).read(), flags=re.S)
    vs = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "mmhand_amd", "csrc", "exports.map")).read(), flags=re.S)
    pats = [p.strip() for p in re.search(r"global\s*:(.*?)local\s*:", vs, flags=re.S).group(1).split(";") if p.strip()]
    for name, n_args in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"include/mmhand_hip.h does not declare {name}"
        assert len(m.group(1).split(",")) == n_args
        assert any(fnmatch.fnmatchcase(name, p) for p in pats), pats
        assert len(lib.SIGNATURES[name][1]) == n_args


@pytest.fixture(scope="module")
def built():
    from mmhand_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mmhand_amd", "csrc")])
    return lib.load()


def test_entry_points_refuse_bad_arguments_without_gpu(built):
    """MMH_REQUIRE runs before any launch: NULL buffers, non-positive shapes, S = 0 and misaligned buffers come back as
    errors, each with its own message, on a machine without a device"""
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    p = ctypes.c_void_p((p.value + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 4)
    lb = built

    def aff(srcs=(p, p, p, p), uvs=(p, p), xf=p, B=1, Hs=2, Ws=2, Ho=4, Wo=4, sigma=6.0, outs=(p, p, p, p)):
        return lb.mmh_decode_inputs_affine(*srcs, *uvs, xf, B, Hs, Ws, Ho, Wo, sigma, *outs, None)

    for kw in (dict(srcs=(None, p, p, p)), dict(srcs=(p, p, p, None)), dict(uvs=(p, None)), dict(xf=None),
               dict(outs=(None, p, p, p)), dict(outs=(p, p, p, None))):
        assert aff(**kw) != 0
        assert b"mmh_decode_inputs_affine: NULL buffer" in lb.mmh_last_error()
    for kw in (dict(B=0), dict(Hs=0), dict(Ws=-1), dict(Ho=0), dict(Wo=-4), dict(sigma=0.0)):
        assert aff(**kw) != 0
        assert b"mmh_decode_inputs_affine: bad shape" in lb.mmh_last_error()
    for outs in ((odd, p, p, p), (p, p, odd, p), (p, p, p, odd)):
        assert aff(outs=outs) != 0
        assert b"mmh_decode_inputs_affine: outputs must be 16-byte aligned" in lb.mmh_last_error()
    assert aff(xf=odd) != 0
    assert b"mmh_decode_inputs_affine: xf must be 8-byte aligned" in lb.mmh_last_error()

    def idx(store=p, S=1, Hs=2, Ws=2, idx=p, uv=p, xf=p, B=1, Ho=4, Wo=4, sigma=6.0, outs=(p, p, p, p)):
        return lb.mmh_decode_inputs_indexed_affine(store, S, Hs, Ws, idx, uv, xf, B, Ho, Wo, sigma, *outs, None, None)

    for kw in (dict(store=None), dict(idx=None), dict(uv=None), dict(xf=None), dict(outs=(None, p, p, p)), dict(outs=(p, p, p, None))):
        assert idx(**kw) != 0
        assert b"mmh_decode_inputs_indexed_affine: NULL buffer" in lb.mmh_last_error()
    for kw in (dict(B=0), dict(Hs=0), dict(Ws=-1), dict(Ho=0), dict(Wo=-4), dict(sigma=0.0)):
        assert idx(**kw) != 0
        assert b"mmh_decode_inputs_indexed_affine: bad shape" in lb.mmh_last_error()
    for S in (0, -1):
        assert idx(S=S) != 0
        assert b"mmh_decode_inputs_indexed_affine: S must be at least 1" in lb.mmh_last_error()
    assert idx(outs=(p, p, odd, p)) != 0
    assert b"mmh_decode_inputs_indexed_affine: outputs must be 16-byte aligned" in lb.mmh_last_error()
    for kw in (dict(xf=odd), dict(uv=odd)):
        assert idx(**kw) != 0
        assert b"mmh_decode_inputs_indexed_affine: uv and xf must be 8-byte aligned" in lb.mmh_last_error()
