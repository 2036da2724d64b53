"""--resize_inputs without a GPU: the float64 restatement of the sampling rule the GPU tests hold the kernel to
(tests/_resize_oracle.py) IS torch's bilinear interpolation with half-pixel centres, the option is checked where options
are checked, and the new entry point is declared where test_host_cpu.py's ABI test will look for it."""
import fnmatch
import os
import re

import numpy as np
import pytest
import torch

from tests import _resize_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(24, 20), (20, 28), (8, 4)]          # from 12 x 10: up 2x both ways, independent ratios, down (2.5x in W)


@pytest.mark.parametrize("out", SIZES, ids=lambda s: "%dx%d" % s)
def test_oracle_is_torch_bilinear_half_pixel(out):
    rs = np.random.RandomState(11)
    a = rs.randint(0, 256, size=(2, 3, 12, 10)).astype(np.float64)
    want = torch.nn.functional.interpolate(torch.from_numpy(a), size=out, mode="bilinear", align_corners=False).numpy()
    got = RO.bilinear(a, *out)
    assert got.shape == want.shape == (2, 3) + out
    assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()


def test_oracle_identity_and_edge_clamp():
    rs = np.random.RandomState(12)
    a = rs.uniform(0, 255, size=(12, 10))
    assert np.array_equal(RO.bilinear(a, 12, 10), a)
    up = RO.bilinear(a, 24, 20)
    assert up[0, 0] == a[0, 0] and np.isclose(up[-1, -1], a[-1, -1], rtol=1e-15) and np.isclose(up[0, -1], a[0, -1], rtol=1e-15)
    i0, i1, w = RO.taps(10, 4)
    assert i0.tolist() == [0, 3, 5, 8] and i1.tolist() == [1, 4, 6, 9] and np.allclose(w, [0.75, 0.25, 0.75, 0.25])


def test_oracle_rounds_nothing_between_the_bytes_and_the_result():
    """neighbours that straddle a G boundary, (G, R) = (0, 255) next to (1, 0): raw depths 255 and 256, a quarter of the
    way 255.25.  Interpolated G and R rounded back to bytes first would give 256 * 0 + 191 there."""
    dep = np.zeros((2, 4, 3), dtype=np.uint8)            # B, G, R
    dep[:, 1] = (0, 0, 255)
    dep[:, 2] = (0, 1, 0)
    _, d = RO.decode_resized(dep, dep, 2, 8)             # x only: sx = 1.25 at output 3, 1.75 at output 4
    raw = (d * 0.5 + 0.5) * 700.0
    assert np.allclose(raw[:, 3], 255.25, atol=1e-9) and np.allclose(raw[:, 4], 255.75, atol=1e-9)
    w32, tol = RO.f32_tolerance(np.array([0.0, 1.0, -0.27, 186.0]))
    assert tol[0] == 1e-13 and abs(tol[1] - (2.0 ** -23 + 1e-13)) < 1e-20 and w32.dtype == np.float32


def test_joint_scaling_follows_the_pixel_centres():
    """a joint on the centre of source pixel (x, y) lands where that pixel's centre lands: at 2x, pixel 3 covers output
    pixels 6 and 7, its centre sits at 6.5; the third component (C1 / C2's depth) is not touched"""
    uv = np.array([[3.0, 5.0, 77.0], [-0.5, -0.5, 1.0]])
    out = RO.scale_joints(uv, (12, 10), (24, 20))
    assert out.tolist() == [[6.5, 10.5, 77.0], [-0.5, -0.5, 1.0]]
    assert np.array_equal(RO.scale_joints(uv, (12, 10), (12, 10)), uv)


def test_resize_inputs_option_is_checked_without_gpu():
    from mmhand_amd.options import TestOptions, TrainOptions, check_resize_inputs, default_train_opt
    for n in (0, 32):
        opt = TrainOptions().parse(["--resize_inputs", str(n)], init_dist=False, save=False)
        assert opt.resize_inputs == n and opt.fineSize == 256
    assert TrainOptions().parse([], init_dist=False, save=False).resize_inputs == 0          # off by default
    assert TestOptions().parse(["--resize_inputs", "64"], init_dist=False, save=False).resize_inputs == 64
    for bad in ("30", "-4", "2"):
        with pytest.raises(ValueError, match="resize_inputs"):
            TrainOptions().parse(["--resize_inputs", bad], init_dist=False, save=False)
    for bad in (30, -4, 6.0, True):
        with pytest.raises(ValueError, match="resize_inputs"):
            check_resize_inputs(default_train_opt(resize_inputs=bad))
    assert check_resize_inputs(default_train_opt()) == 0 and check_resize_inputs(default_train_opt(resize_inputs=128)) == 128


def test_resize_size_and_joints_helpers():
    from mmhand_amd import ops
    assert ops.resize_size(None, (12, 10)) is None and ops.resize_size(0, (12, 10)) is None
    assert ops.resize_size((12, 10), (12, 10)) is None and ops.resize_size(12, (12, 12)) is None
    assert ops.resize_size(16, (12, 10)) == (16, 16) and ops.resize_size((8, 4), (12, 10)) == (8, 4)
    with pytest.raises(ValueError):
        ops.resize_size((8, -4), (12, 10))
    rs = np.random.RandomState(13)
    c = rs.uniform(-4, 16, size=(2, 21, 3))
    got = ops.resize_joints(torch.from_numpy(c), (12, 10), (20, 28))
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), RO.scale_joints(c, (12, 10), (20, 28)))


def test_entry_point_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mmhand_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+mmh_decode_inputs_resized\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/mmhand_hip.h does not declare mmh_decode_inputs_resized"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 17 and [p.split()[-1] for p in params[6:12]] == ["B", "Hs", "Ws", "Ho", "Wo", "sigma"]
    # exports.map is the version script the library is linked through: its global patterns must let the symbol out
    vs = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "mmhand_amd", "csrc", "exports.map")).read(), flags=re.S)
    glob = re.search(r"global\s*:(.*?)local\s*:", vs, flags=re.S).group(1)
    pats = [p.strip() for p in glob.split(";") if p.strip()]
    assert any(fnmatch.fnmatchcase("mmh_decode_inputs_resized", p) for p in pats), pats
    from mmhand_amd import lib
    assert len(lib.SIGNATURES["mmh_decode_inputs_resized"][1]) == 17


def test_entry_point_refuses_bad_arguments_without_gpu():
    """MMH_REQUIRE runs before any launch: NULL buffers and non-positive sizes come back as errors on the CPU"""
    import ctypes
    from mmhand_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mmhand_amd", "csrc")])
    l = lib.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert l.mmh_decode_inputs_resized(None, p, p, p, p, p, 1, 2, 2, 4, 4, 6.0, p, p, p, p, None) != 0
    assert b"mmh_decode_inputs_resized: NULL buffer" in l.mmh_last_error()
    for shape in ((0, 2, 2, 4, 4), (1, 2, 0, 4, 4), (1, 2, 2, 4, -4)):
        assert l.mmh_decode_inputs_resized(p, p, p, p, p, p, *shape, 6.0, p, p, p, p, None) != 0
        assert b"mmh_decode_inputs_resized: bad shape" in l.mmh_last_error()
    assert l.mmh_decode_inputs_resized(p, p, p, p, p, p, 1, 2, 2, 4, 4, 0.0, p, p, p, p, None) != 0
