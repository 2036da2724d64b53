"""mmh_ms_ssim (csrc/metrics.hip: ms_ssim_level_kernel, ms_ssim_final_kernel; mmhand_amd.metrics.ms_ssim) on the device against
the float64 oracle of tests/_msssim_oracle.py.

* per level, per pixel: probe pairs make N_l (1 - scales[b][c][l]) a sum over the few valid pixels of level l whose window holds
  a pooled probe; it is held to `affected_l x 1e-6`, the kernel's documented bar.  The probes sit at the first and last valid
  row and column, the image corners, row and column 0 of an odd-sized level (pooled with zeros), the level-1 and level-2 tile
  seams (the pooling workgroup reads the row before its tile from its halo) and in the ragged last tile of every level;
* the whole value on perturbed pairs: |ms - oracle| <= ms * sum_l w_l * 1e-6 / v_l (1.0e-6 at five levels), at the smallest
  five-level shape, at 17 tile rows and with more partials per plane than the finishing kernel has threads;
* exact statements: ms_ssim(x, x) == 1, symmetry, ms_ssim(a, 1 - a) == 0, run-to-run and batch-slice bit-identity, one level;
* all nine storage pairs, a u8 pair, an NHWC view; refused shapes.

Measured on an MI355X (each test prints its figures): per level and pixel 0.167 of the bar at worst; whole value 7.5e-9 at five
levels against a bound of 1.0e-6; off the grid 1.0e-8 (1.5e-8 from the all-float64 definition)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _metrics_oracle as M
from tests import _msssim_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    O.clear_caches()
    M.clear_caches()


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _run(dev, a, b, window, weights, range="pm1"):
    from mmhand_amd.metrics import ms_ssim
    r = ms_ssim(a.to(dev), b.to(dev), range=range, window=window, weights=weights)
    ms, scales = r["ms_ssim"].cpu().numpy(), r["scales"].cpu().numpy()
    assert ms.dtype == scales.dtype == np.float64 and scales.shape[:2] == tuple(a.shape[:2]) and scales.shape[2] == len(weights)
    return ms, scales


@pytest.mark.parametrize("name", list(O.PROBE_SHAPES))
def test_levels_per_pixel(dev, name):
    """One probe per image.  |S_got - S_want| / (affected_l x 1e-6), the largest per case, is printed.  Measured on an MI355X:
    67 x 45, w = 5: 0.167 (a corner probe at level 1); 131 x 70, w = 3: 0.166 (the bottom-right corner at level 2)."""
    case = O.probe_case(name)
    ms, scales = _run(dev, case["a"], case["b"], case["window"], case["weights"])
    S_got = O.level_S(scales, case["shape"], case["window"])[:, 0]
    ratio = np.abs(S_got - case["S"]) / (case["affected"] * O.LEVEL_BAR)
    i, l = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"\n[{name}] worst |S_got - S_want| / bar = {ratio[i, l]:.3f} at image {i} ({case['why'][i]}), level {l}")
    bad = np.argwhere(~(ratio <= 1.0))
    assert bad.size == 0, [(int(i), int(l), case["why"][i], S_got[i, l], case["S"][i, l], int(case["affected"][i, l])) for i, l in bad[:8]]
    assert np.all(np.abs(ms - case["ms"]) <= 1e-6), (ms, case["ms"])


@pytest.mark.parametrize("name", list(O.WHOLE_CASES))
def test_whole_value(dev, name):
    """Perturbed pairs: the whole value inside the propagated bound, every level value inside 1e-6.  Measured on an MI355X,
    |ms - oracle| (bound; largest level error): five_levels 7.5e-9 (1.0e-6; 2.0e-7), two_levels_w11 1.5e-9 (3.5e-7; 5.1e-9),
    three_levels_w5 4.7e-9 (6.5e-7; 4.4e-8), smallest 2.7e-8 (3.3e-7; 9.3e-8), tall 2.0e-9 (6.3e-7; 5.2e-9), many 9.1e-10
    (3.3e-7; 3.3e-9)."""
    case = O.whole_case(name)
    ms, scales = _run(dev, case["a"], case["b"], case["window"], case["weights"])
    err, lvl = np.abs(ms - case["ms"]), np.abs(scales - case["scales"]).max()
    print(f"\n[{name}] |ms - oracle| = {err.max():.3e} (bound {case['bound'].min():.3e}), largest level error {lvl:.3e}")
    assert lvl <= O.LEVEL_BAR, (name, lvl)
    assert np.all(err <= case["bound"]), (name, err, case["bound"])


def test_identical_pair_is_exactly_one(dev):
    """every map value is 1.0 exactly, so a level's sum is its count N; N * (1.0 / N) may be one ulp below 1, the product of the
    powers is 1.0"""
    ulp = np.finfo(np.float64).eps
    case = O.whole_case("three_levels_w5")
    ms, scales = _run(dev, case["a"], case["a"], 5, case["weights"])
    assert np.all(ms == 1.0) and np.all(np.abs(scales - 1.0) <= ulp), (ms, scales - 1.0)
    five = O.whole_case("five_levels")
    ms, scales = _run(dev, five["b"], five["b"], 11, five["weights"])
    assert np.all(ms == 1.0) and np.all(np.abs(scales - 1.0) <= ulp), (ms, scales - 1.0)


@pytest.mark.parametrize("name", ["five_levels", "two_levels_w11"])
def test_symmetric_bit_for_bit(dev, name):
    case = O.whole_case(name)
    ab = _run(dev, case["a"], case["b"], case["window"], case["weights"])
    ba = _run(dev, case["b"], case["a"], case["window"], case["weights"])
    assert np.array_equal(_bits(ab[0]), _bits(ba[0])) and np.array_equal(_bits(ab[1]), _bits(ba[1]))


def test_inverted_image_is_exactly_zero(dev):
    """b = 1 - a on [0, 1] (-a in the stored range): every cs level is negative in the oracle, the clamp makes the product 0"""
    a = M.from_grid(np.maximum(M.grid((2, 3, 33, 33), 1), 1))          # k >= 1, so that -a stays on the grid
    ms_want, scales_want = O.ms_ssim(M.mapped(a, "pm1"), M.mapped(-a, "pm1"), 5, O.MS_WEIGHTS[:3])
    assert np.all(scales_want[:, :, :-1] < 0) and np.all(ms_want == 0.0)
    ms, scales = _run(dev, a, -a, 5, O.MS_WEIGHTS[:3])
    assert np.all(ms == 0.0) and not np.signbit(ms).any(), ms
    assert np.all(scales[:, :, :-1] < 0) and np.abs(scales - scales_want).max() <= O.LEVEL_BAR


def test_run_to_run_and_batch_slices(dev):
    case = O.whole_case("five_levels")
    full, again = (_run(dev, case["a"], case["b"], 11, case["weights"]) for _ in range(2))
    assert np.array_equal(_bits(full[0]), _bits(again[0])) and np.array_equal(_bits(full[1]), _bits(again[1]))
    for i in range(case["shape"][0]):
        alone = _run(dev, case["a"][i:i + 1].clone(), case["b"][i:i + 1].clone(), 11, case["weights"])
        assert np.array_equal(_bits(alone[0]), _bits(full[0][i:i + 1])) and np.array_equal(_bits(alone[1]), _bits(full[1][i:i + 1]))


def test_one_level_is_the_valid_interior_ssim(dev):
    case = O.whole_case("two_levels_w11")
    a01, b01 = M.mapped(case["a"], "pm1"), M.mapped(case["b"], "pm1")
    want = O.valid(M.ssim_map(a01, b01, 11), 11).mean(axis=(2, 3))
    ms, scales = _run(dev, case["a"], case["b"], 11, (1.0,))
    assert scales.shape == (2, 1, 1) and np.abs(scales[:, :, 0] - want).max() <= O.LEVEL_BAR
    assert np.abs(ms - scales[:, 0, 0]).max() <= 4 * np.finfo(np.float64).eps, (ms, scales)


_TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _nhwc_view(t, cs=8):
    B, Cc, H, W = t.shape
    buf = torch.full((B, H, W, cs), float("nan"), dtype=t.dtype, device=t.device)
    buf[..., :Cc] = t.permute(0, 2, 3, 1)
    v = buf.permute(0, 3, 1, 2)[:, :Cc]
    assert not v.is_contiguous() and torch.equal(v, t)
    return v


@pytest.mark.parametrize("tb", list(_TORCH))
@pytest.mark.parametrize("ta", list(_TORCH))
def test_storage_types_give_the_fp32_bits(dev, ta, tb):
    """grid values are exact in all three types, so every pair must return what fp32 / fp32 returns, bit for bit; side b is an
    NHWC view when the types differ"""
    from mmhand_amd.metrics import ms_ssim
    case = O.whole_case("three_levels_w5")
    ref = _run(dev, case["a"], case["b"], 5, case["weights"])
    a, b = case["a"].to(dev).to(_TORCH[ta]), case["b"].to(dev).to(_TORCH[tb])
    assert torch.equal(a.float().cpu(), case["a"]) and torch.equal(b.float().cpu(), case["b"])
    r = ms_ssim(a, _nhwc_view(b) if ta != tb else b, range="pm1", window=5, weights=case["weights"])
    assert np.array_equal(_bits(r["ms_ssim"].cpu().numpy()), _bits(ref[0]))
    assert np.array_equal(_bits(r["scales"].cpu().numpy()), _bits(ref[1]))


def test_u8_pair_off_the_dyadic_grid(dev):
    """8-bit B,G,R pixels, u / 255 in fp32: the levels are pooled in fp32 in the kernel's order in the oracle too"""
    case = O.whole_case("three_levels_w5")
    ka = np.rint((case["a"].numpy().astype(np.float64) + 1.0) * 128.0).astype(np.uint8)
    kb = np.rint((case["b"].numpy().astype(np.float64) + 1.0) * 128.0).astype(np.uint8)
    a = torch.from_numpy(np.ascontiguousarray(ka.transpose(0, 2, 3, 1)))
    b = torch.from_numpy(np.ascontiguousarray(kb.transpose(0, 2, 3, 1)))
    want_ms, want_scales = O.ms_ssim(M.mapped(a, "u8_bgr_hwc"), M.mapped(b, "u8_bgr_hwc"), 5, case["weights"], pool_dtype=np.float32)
    from mmhand_amd.metrics import ms_ssim
    r = ms_ssim(a.to(dev), b.to(dev), range="u8_bgr_hwc", window=5, weights=case["weights"])
    ms, scales = r["ms_ssim"].cpu().numpy(), r["scales"].cpu().numpy()
    assert np.abs(scales - want_scales).max() <= O.LEVEL_BAR
    assert np.all(np.abs(ms - want_ms) <= O.whole_bound(want_ms, want_scales, case["weights"]))


def test_off_the_grid(dev):
    """Values that are not on the dyadic grid: against the oracle pooling in fp32 in the kernel's stated order, per level and as
    a whole.  The distance to the all-float64 definition (float64 pooling) is printed, not asserted: it is the fp32 rounding of
    the pooled levels, not an error of the kernel.  Measured on an MI355X: 1.0e-8 to the fp32-pooling oracle (level 2.3e-7),
    1.5e-8 to the all-float64 definition (level 2.6e-7); the two oracles differ by 4.9e-9."""
    from tests._hpe_oracle import hashed
    shape = (1, 3, 161, 176)
    n = int(np.prod(shape))
    a = torch.from_numpy((hashed(7100, n, 1) * 0.9).reshape(shape).astype(np.float32))
    b = torch.from_numpy(np.clip(a.numpy().astype(np.float64) + 0.2 * hashed(7101, n, 1).reshape(shape), -1, 1).astype(np.float32))
    a01, b01 = M.mapped(a, "pm1"), M.mapped(b, "pm1")
    want_ms, want_scales = O.ms_ssim(a01, b01, 11, O.MS_WEIGHTS, pool_dtype=np.float32)
    assert want_scales.min() >= O.FLOOR
    ms, scales = _run(dev, a, b, 11, O.MS_WEIGHTS)
    f64_ms, f64_scales = O.ms_ssim(a01, b01, 11, O.MS_WEIGHTS)
    print(f"\n[off the grid] |ms - oracle(fp32 pooling)| = {np.abs(ms - want_ms).max():.3e}, level {np.abs(scales - want_scales).max():.3e}; "
          f"to the all-float64 definition: ms {np.abs(ms - f64_ms).max():.3e}, level {np.abs(scales - f64_scales).max():.3e}; "
          f"oracle fp32 vs float64 pooling: ms {np.abs(want_ms - f64_ms).max():.3e}")
    assert np.abs(scales - want_scales).max() <= O.LEVEL_BAR
    assert np.all(np.abs(ms - want_ms) <= O.whole_bound(want_ms, want_scales, O.MS_WEIGHTS))


def test_refused_shapes_launch_nothing(dev):
    from mmhand_amd import lib as L
    from mmhand_amd.metrics import C1, C2, _src, gaussian_taps, ms_ssim
    a = torch.zeros((1, 3, 160, 176), device=dev)
    with pytest.raises(ValueError, match="must exceed"):
        ms_ssim(a, a)
    with pytest.raises(ValueError, match="weights"):
        ms_ssim(a, a, weights=(0.5, -0.5))
    with pytest.raises(ValueError, match="weights"):
        ms_ssim(a, a, weights=(0.2,) * 6)
    lib = L.load()
    assert lib.mmh_ms_ssim_ws_bytes(1, 3, 160, 176, 11, 5) == 0
    sa, _ = _src(a, "pm1")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    out = torch.full((1,), -7.0, dtype=torch.float64, device=dev)
    scales = torch.full((1, 3, 5), -7.0, dtype=torch.float64, device=dev)
    w = np.array(O.MS_WEIGHTS)
    rc = lib.mmh_ms_ssim(C.byref(sa), C.byref(sa), 1, 3, 160, 176, 11, gaussian_taps(11).ctypes.data_as(C.c_void_p), C1, C2, 5,
                         w.ctypes.data_as(C.c_void_p), ws.data_ptr(), ws.numel(), scales.data_ptr(), out.data_ptr(), None)
    assert rc != 0 and b"(window - 1) * 2^(levels - 1)" in lib.mmh_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((scales == -7.0).all()) and int(ws.count_nonzero()) == 0
