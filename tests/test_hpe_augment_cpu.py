"""train_hpe --augment_geom / --augment_color without a GPU: the host's colour maths (data.color_matrix) against the oracle's
independent construction (tests/_hpe_augment_oracle.py), the draws and their independence, the options' validation, the parser,
the new entry points' declarations and argument checks, and label / pixel consistency on the oracle."""
import ctypes
import fnmatch
import os
import re
import types

import numpy as np
import pytest

from tests import _hpe_augment_oracle as HO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mmh_hpe_augment_normalize": 13, "mmh_hpe_augment_normalize_ws_bytes": 3}
BASE = ["--dataroot", "/somewhere/rhd", "--dataset", "rhd", "--name", "n"]


# ----------------------------------------------------------------------------- data.color_matrix
def test_color_matrix_is_the_exact_identity_at_the_neutral_draw():
    from mmhand_amd.data import color_matrix
    m = color_matrix(1.0, 0.0, [1.0, 1.0, 1.0])
    assert m.shape == (3, 3) and m.dtype == np.float64
    assert np.array_equal(m.view(np.uint64), np.eye(3).view(np.uint64))             # bit for bit: no -0.0 either
    many = color_matrix(np.ones(4), np.zeros(4), np.ones((4, 3)))
    assert many.shape == (4, 3, 3) and all(np.array_equal(x.view(np.uint64), np.eye(3).view(np.uint64)) for x in many)
    assert np.array_equal(color_matrix(1.0, 360.0, [1.0, 1.0, 1.0]), np.eye(3))
    with pytest.raises(ValueError, match="gains"):
        color_matrix(1.0, 0.0, [1.0, 1.0])


def test_color_matrix_maps_grey_to_the_gains_times_grey():
    """saturation and hue leave the grey axis where it is"""
    from mmhand_amd.data import color_matrix
    rs = np.random.RandomState(2)
    for _ in range(50):
        s, h, g = rs.uniform(0.0, 2.0), rs.uniform(-180.0, 180.0), rs.uniform(0.5, 1.5, 3)
        for grey in (1.0, 0.37):
            assert np.abs(color_matrix(s, h, g) @ np.full(3, grey) - g * grey).max() <= 1e-13


def test_color_matrix_agrees_with_the_independent_construction():
    from mmhand_amd.data import color_matrix
    worst = 0.0
    for s in (0.0, 0.5, 0.7, 1.0, 1.3, 2.0):
        for h in (-180.0, -90.0, -10.0, -3.3, 0.0, 7.25, 10.0, 45.0, 90.0, 120.0):
            for g in ((1.0, 1.0, 1.0), (0.9, 1.1, 1.0), (1.07, 0.93, 1.02)):
                worst = max(worst, float(np.abs(color_matrix(s, h, g) - HO.matrix(s, h, g)).max()))
    print(f"color_matrix against the per-pixel construction: largest distance {worst:.2e}")
    assert worst <= 1e-12
    # broadcasting equals one at a time, bit for bit: a batch gets the matrices a single image would
    rs = np.random.RandomState(4)
    s, h, g = rs.uniform(0.7, 1.3, 6), rs.uniform(-10, 10, 6), rs.uniform(0.9, 1.1, (6, 3))
    many = color_matrix(s, h, g)
    assert all(np.array_equal(many[i], color_matrix(s[i], h[i], g[i])) for i in range(6))


def test_opposite_quarter_turns_of_the_hue_cancel():
    from mmhand_amd.data import color_matrix
    one = [1.0, 1.0, 1.0]
    assert np.abs(color_matrix(1.0, 90.0, one) @ color_matrix(1.0, -90.0, one) - np.eye(3)).max() <= 1e-15
    # and a turn by 120 degrees about the grey axis is the cyclic permutation R -> G -> B -> R
    assert np.abs(color_matrix(1.0, 120.0, one) - np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]])).max() <= 1e-15


# ----------------------------------------------------------------------------- draws and options
def _args(*extra):
    from mmhand_amd import train_hpe
    p = train_hpe.build_parser()
    a = p.parse_args(BASE + list(extra))
    train_hpe.check_args(p, a)
    return a


def test_color_draws():
    from mmhand_amd.data import color_draws
    a = _args("--augment_color", "--aug_seed", "4")
    d0 = color_draws(200, 0, a)
    assert d0.shape == (200, 6) and d0.dtype == np.float64
    assert np.array_equal(d0, color_draws(200, 0, a))                         # (seed, epoch, item) decides, nothing else
    assert np.array_equal(d0[:50], color_draws(50, 0, a))                     # ... not the length of the list either
    assert not np.array_equal(d0, color_draws(200, 1, a))
    assert not np.array_equal(d0, color_draws(200, 0, _args("--augment_color", "--aug_seed", "5")))
    assert (np.abs(d0[:, 0] - 1.0) <= 0.3).all() and (np.abs(d0[:, 1]) <= 10.0).all() and (np.abs(d0[:, 2:5] - 1.0) <= 0.1).all()
    assert (np.abs(np.log(d0[:, 5])) <= 0.2 + 1e-15).all()
    assert np.ptp(d0[:, 0]) > 0.5 and np.ptp(d0[:, 1]) > 17.0 and np.ptp(d0[:, 2:5]) > 0.17 and np.ptp(np.log(d0[:, 5])) > 0.35
    assert not np.array_equal(d0[:, 2], d0[:, 3])                             # the gains are per channel
    wide = color_draws(200, 0, _args("--augment_color", "--aug_saturation", "3.0"))
    assert wide[:, 0].min() == 0.0 and wide[:, 0].max() > 3.0                 # clipped at 0
    zero = color_draws(9, 3, _args("--augment_color", "--aug_saturation", "0", "--aug_hue", "0", "--aug_gain", "0", "--aug_gamma", "0"))
    assert np.array_equal(zero, np.tile([1.0, 0.0, 1.0, 1.0, 1.0, 1.0], (9, 1)))


def test_either_switch_leaves_the_others_draws_as_they_are():
    from mmhand_amd import train_hpe
    from mmhand_amd.data import augment_draws, color_draws
    geom, color, both = _args("--augment_geom"), _args("--augment_color"), _args("--augment_geom", "--augment_color")
    for epoch in (1, 2):
        assert np.array_equal(augment_draws(30, epoch, geom), augment_draws(30, epoch, both))
        assert np.array_equal(color_draws(30, epoch, color), color_draws(30, epoch, both))
    # the two streams are different streams
    assert not np.array_equal(augment_draws(30, 1, both)[:, 0, :5].ravel()[:6], color_draws(30, 1, both).ravel()[:6])
    # ... and that is what the driver's Augment hands out, by item number: side 0 of the geometry draws
    assert train_hpe.Augment.of(_args(), 30) is None
    ag, ab = train_hpe.Augment.of(geom, 30), train_hpe.Augment.of(both, 30)
    ag.set_epoch(2)
    ab.set_epoch(2)
    assert ag.color is None and np.array_equal(ag.geom, ab.geom) and np.array_equal(ab.geom, augment_draws(30, 2, both)[:, 0])
    assert np.array_equal(ab.color, color_draws(30, 2, color))
    ids = [7, 0, 29]
    fwd = ab.forward_maps(ids, (32, 32))
    ab.set_epoch(3)
    assert fwd.shape == (3, 2, 3) and not np.array_equal(fwd, ab.forward_maps(ids, (32, 32)))       # another epoch
    ab.set_epoch(2)
    assert np.array_equal(fwd[::-1], ab.forward_maps(ids[::-1], (32, 32)))                         # by item, whatever the batch
    uv = np.random.RandomState(1).uniform(0, 32, (3, 21, 2))
    moved = ab.joints(uv, ids, (32, 32))
    assert moved.shape == uv.shape and not np.array_equal(moved, uv)
    ac = train_hpe.Augment.of(color, 30)
    ac.set_epoch(2)
    assert ac.joints(uv, ids, (32, 32)) is uv                                                       # colour moves no joint


def test_check_augment_color():
    from mmhand_amd.options import check_augment_color
    assert check_augment_color(types.SimpleNamespace()) is None
    assert check_augment_color(types.SimpleNamespace(augment_color=False, aug_gain=7.0)) is None    # off: nothing is looked at
    assert check_augment_color(types.SimpleNamespace(augment_color=True)) == (0.3, 10.0, 0.1, 0.2, 0)
    ok = dict(augment_color=True, aug_saturation=0.5, aug_hue=20.0, aug_gain=0.2, aug_gamma=0.3, aug_seed=3)
    assert check_augment_color(types.SimpleNamespace(**ok)) == (0.5, 20.0, 0.2, 0.3, 3)
    for kw in (dict(aug_saturation=-0.1), dict(aug_saturation=float("nan")), dict(aug_hue=-1.0), dict(aug_hue=181.0),
               dict(aug_gain=1.0), dict(aug_gain=-0.1), dict(aug_gamma=-0.2), dict(aug_gamma=float("inf")), dict(aug_gamma=5.0),
               dict(aug_hue="10"), dict(aug_gain=True), dict(aug_seed=-1), dict(aug_seed=1.5)):
        with pytest.raises(ValueError, match="aug_"):
            check_augment_color(types.SimpleNamespace(**dict(ok, **kw)))


def test_parser():
    a = _args()
    assert a.augment_geom is False and a.augment_color is False
    assert (a.aug_rotate, a.aug_scale, a.aug_shift, a.aug_flip, a.aug_seed) == (15.0, 0.1, 0.05, 0.0, 0)
    assert (a.aug_saturation, a.aug_hue, a.aug_gain, a.aug_gamma) == (0.3, 10.0, 0.1, 0.2)
    assert not hasattr(a, "aug_pair")
    a = _args("--augment_geom", "--aug_rotate", "30", "--aug_flip", "0.5", "--augment_color", "--aug_hue", "5", "--aug_seed", "2")
    assert a.augment_geom and a.augment_color and (a.aug_rotate, a.aug_flip, a.aug_hue, a.aug_seed) == (30.0, 0.5, 5.0, 2)
    _args("--net", "hpm3d", "--augment_geom")                                  # the joints move; no image exists
    _args("--net", "hpm3d", "--heat_source", "predicted", "--hpm2d", "h.pth", "--augment_geom", "--augment_color")
    bad = [["--net", "hpm3d", "--augment_color"],                              # --heat_source target reads no image
           ["--net", "hpm3d", "--heat_source", "target", "--augment_geom", "--augment_color"],
           ["--aug_rotate", "10"], ["--aug_scale", "0.2"], ["--aug_shift", "0.1"], ["--aug_flip", "0.5"], ["--aug_seed", "1"],
           ["--aug_saturation", "0.1"], ["--aug_hue", "5"], ["--aug_gain", "0.1"], ["--aug_gamma", "0.1"],
           ["--augment_color", "--aug_rotate", "10"], ["--augment_geom", "--aug_hue", "5"],      # the other switch's range
           ["--augment_geom", "--aug_scale", "1.0"], ["--augment_geom", "--aug_rotate", "181"],   # `train`'s validation
           ["--augment_color", "--aug_gain", "1.0"], ["--augment_geom", "--aug_seed", "-1"], ["--aug_pair", "shared"]]
    for extra in bad:
        with pytest.raises(SystemExit):
            _args(*extra)


# ----------------------------------------------------------------------------- the C-ABI
def test_entry_points_are_declared_and_exported():
    from mmhand_amd import lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmhand_hip.h")).read(), flags=re.S)
    vs = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "mmhand_amd", "csrc", "exports.map")).read(), flags=re.S)
    pats = [p.strip() for p in re.search(r"global\s*:(.*?)local\s*:", vs, flags=re.S).group(1).split(";") if p.strip()]
    for name, n_args in NAMES.items():
        m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"include/mmhand_hip.h does not declare {name}"
        assert len(m.group(1).split(",")) == n_args
        assert any(fnmatch.fnmatchcase(name, p) for p in pats), pats
        assert len(lib.SIGNATURES[name][1]) == n_args
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert f"({len(lib.SIGNATURES)} entry points" in fh.read()


@pytest.fixture(scope="module")
def built():
    from mmhand_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mmhand_amd", "csrc")])
    return lib.load()


def test_entry_point_refuses_bad_arguments_without_gpu(built):
    """MMH_REQUIRE runs before any launch: every refusal comes back as an error with its own message on a machine without a
    device"""
    lb = built
    assert lb.mmh_hpe_augment_normalize_ws_bytes(3, 24, 40) == 3 * 4 * 16           # 960 pixels: 4 chunks of (min, max)
    assert lb.mmh_hpe_augment_normalize_ws_bytes(1, 136, 128) == 64 * 16            # the cap
    for bad in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, -2), (65536, 8, 8), (1, 65536, 65536)):
        assert lb.mmh_hpe_augment_normalize_ws_bytes(*bad) == 0
    buf = (ctypes.c_char * 256)()
    p = ctypes.c_void_p((ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15)
    odd8, odd4 = ctypes.c_void_p(p.value + 8), ctypes.c_void_p(p.value + 4)

    def call(img=p, B=1, Hs=2, Ws=2, Ho=2, Wo=2, xf=p, cm=p, gamma=p, ws=p, ws_bytes=16, out=p):
        return lb.mmh_hpe_augment_normalize(img, B, Hs, Ws, Ho, Wo, xf, cm, gamma, ws, ws_bytes, out, None)

    for kw in (dict(img=None), dict(ws=None), dict(out=None)):
        assert call(**kw) != 0
        assert b"mmh_hpe_augment_normalize: NULL buffer" in lb.mmh_last_error()
    for kw in (dict(B=0), dict(Hs=0), dict(Ws=-1), dict(Ho=0), dict(Wo=-4), dict(B=65536)):
        assert call(**kw) != 0
        assert b"mmh_hpe_augment_normalize: bad shape" in lb.mmh_last_error()
    for kw in (dict(xf=None, Ho=4, Wo=4, ws_bytes=64), dict(xf=None, Ho=2, Wo=3), dict(xf=None, Hs=3)):
        assert call(**kw) != 0
        assert b"mmh_hpe_augment_normalize: xf = NULL needs an output of the source's size" in lb.mmh_last_error()
    for kw in (dict(ws_bytes=15), dict(ws_bytes=0), dict(B=2, ws_bytes=16)):
        assert call(**kw) != 0
        assert b"mmh_hpe_augment_normalize: workspace" in lb.mmh_last_error()
    for out in (odd8, odd4):
        assert call(out=out) != 0
        assert b"mmh_hpe_augment_normalize: out must be 16-byte aligned" in lb.mmh_last_error()
    for kw in (dict(xf=odd4), dict(cm=odd4), dict(gamma=odd4), dict(ws=odd4)):
        assert call(**kw) != 0
        assert b"mmh_hpe_augment_normalize: xf, cm, gamma and ws must be 8-byte aligned" in lb.mmh_last_error()


# ----------------------------------------------------------------------------- the oracle itself
def test_oracle_identity_is_the_plain_normalisation():
    img = HO.images(1, *HO.SRC, seed=3)[0]
    rgb = img[:, :, ::-1].astype(np.float64)
    want = (rgb - rgb.min()) / (rgb.max() - rgb.min())
    for kw in (dict(), dict(A=HO.IDENTITY, cm=np.eye(3), gamma=1.0)):
        got, rng = HO.augment_normalize(img, **kw)
        assert np.array_equal(got, want) and rng == float(rgb.max() - rgb.min())
    assert not HO.augment_normalize(np.full((4, 5, 3), 9, dtype=np.uint8))[0].any()                 # a constant image: zeros


def test_every_toleranced_case_has_the_range_its_tolerance_needs():
    """CONDITION of tests/_hpe_augment_oracle.py: mx - mn >= 32 in every image of every toleranced case; and the float64 term
    of the tolerance stays where the docstring says"""
    names = []
    for name, img, A, cm, gamma, out in HO.cases():
        names.append(name)
        for b in range(img.shape[0]):
            kw = dict(A=None if A is None else A[b], cm=None if cm is None else cm[b], gamma=None if gamma is None else gamma[b],
                      out=out)
            want, tol, rng = HO.tolerance(img[b], **kw)
            assert rng >= HO.MIN_RANGE, (name, b, rng)
            extra = (tol - np.spacing(np.abs(want)).astype(np.float64)).max()
            assert 0.0 < extra <= (1e-13 if gamma is None else 2e-10), (name, b, extra)
            assert want.shape == tuple(out) + (3,) and want.min() == 0.0 and want.max() == 1.0
    assert names == ["geom_24x40", "all_24x40", "geom_16x24", "all_16x24", "color", "gamma", "second_turn"]


def test_label_and_pixels_move_together_on_the_oracle():
    """a 3x3 blob at a joint, warped through affine_inverse(fwd): the brightest output pixels lie within one pixel of
    affine_joints(joint, fwd)"""
    from mmhand_amd.data import affine_forward, affine_inverse, affine_joints
    H, W = HO.SRC
    for (u, v), dst in (((22, 11), (H, W)), ((9, 15), (H, W)), ((22, 11), (16, 24))):
        fwd = affine_forward(20.0, 1.1, 0.05, -0.04, True, (H, W))
        got, _ = HO.augment_normalize(HO.blob_image(H, W, u, v), A=affine_inverse(fwd, (H, W), dst), out=dst)
        ju, jv = affine_joints(np.array([[float(u), float(v)]]), fwd, (H, W), dst)[0]
        ys, xs = np.nonzero(got[..., 0] == got[..., 0].max())
        assert got.max() > 0.5 and abs(xs.mean() - ju) <= 1.0 and abs(ys.mean() - jv) <= 1.0, (u, v, dst, ju, jv, xs, ys)
