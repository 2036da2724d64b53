"""The per-pixel oracle of the image metrics (tests/_metrics_oracle.py) checked on its own, and the probe cases of
tests/test_metrics_local_gpu.py checked for what they can see.  No GPU needed.

* the oracle's map, averaged, is the reference's own float64 SSIM (tests/golden/ssim.npz);
* a probe pair's map is exactly 1.0 outside the pixels whose window holds a probe - the premise of the device test;
* sensitivity: a probe read one column or one row off, a border padded by replication and a tap left out each move a
  case's sum of (1 - map) by at least ten times the tolerance the device test gives that case;
* caps: the L1 / MSE sums of every grid-valued case are exact in any order."""
import os

import numpy as np
import pytest

from tests import _metrics_oracle as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    M.clear_caches()


def test_oracle_map_mean_is_the_reference_float64():
    from tests.ssim_cases import cases
    gold = np.load(os.path.join(ROOT, "tests", "golden", "ssim.npz"))
    names = list(gold["names"])
    worst = 0.0
    for name, a, b, w in cases():
        a01, b01 = (a.astype(np.float64) + 1) / 2, (b.astype(np.float64) + 1) / 2      # as make_ssim_golden.py maps them
        got = M.ssim_map(a01, b01, w).mean(axis=(1, 2, 3))
        err = np.abs(got - gold["f64"][names.index(name)]).max()
        worst = max(worst, err)
        assert err <= 1e-12, (name, err)
    print("\nworst |oracle map mean - golden float64|: %.2e" % worst)


def test_mapped_is_the_kernels_fp32_fma():
    import torch
    x = torch.tensor([[[[-1.0, -0.9999999, 1e-30, 0.3333333, 1.0]]]], dtype=torch.float32)
    want = torch.addcmul(torch.tensor(0.5), x, torch.tensor(0.5)).double().numpy()      # exact here: x / 2 is exact
    assert np.array_equal(M.mapped(x, "pm1"), want)
    for dt in (torch.bfloat16, torch.float16):
        assert np.array_equal(M.mapped(x.to(dt), "pm1"), M.mapped(x.to(dt).float(), "pm1"))
    u = torch.arange(256, dtype=torch.uint8).reshape(1, 1, 256, 1).expand(1, 1, 256, 3).contiguous()
    u[..., 0] = 0                                                                        # B plane: the LAST plane of the RGB view
    got = M.mapped(u, "u8_bgr_hwc")
    assert got.shape == (1, 3, 1, 256) and (got[0, 2] == 0).all()
    want = (np.arange(256, dtype=np.float32) * np.float32(1.0 / 255.0)).astype(np.float64)   # one fp32 product = fma(x, s, 0)
    assert np.array_equal(got[0, 0, 0], want)
    k = M.grid((3, 5, 7), seed=1)
    assert np.array_equal(M.mapped(M.from_grid(k)[None], "pm1")[0], k / 256.0)         # the grid maps to multiples of 1/256


@pytest.mark.parametrize("name", list(M.PROBE_CASES))
def test_probe_map_is_one_outside_the_affected_pixels(name):
    case = M.probe_case(name)
    a01, b01 = M.mapped(case["a"], "pm1"), M.mapped(case["b"], "pm1")
    m = M.ssim_map(a01, b01, case["window"])
    mask = M.affected_mask(case["shape"], case["probes"], case["window"])
    assert np.array_equal(mask.reshape(mask.shape[0], -1).sum(1), case["affected"])
    assert (m[~mask] == 1.0).all(), (name, int((m[~mask] != 1.0).sum()))
    assert (m[mask] < 1.0).all()                      # ... and every affected pixel takes part
    # S is therefore the sum over the affected pixels alone, to the last bit
    assert np.array_equal(case["S"], np.where(mask, 1.0 - m, 0.0).sum(axis=(1, 2, 3)))
    # one probe moves |a01 - b01| by exactly 1/2
    d = np.abs(a01 - b01)
    assert set(np.unique(d)) == {0.0, 0.5} and int((d == 0.5).sum()) == len(case["probes"])


def test_last_round_pixels_are_in_the_partial_round():
    for w in M.WINDOWS:
        R, half = M.MT + w - 1, w // 2
        y, x = M.last_round_pixel(w)
        i = (y + half) * R + (x + half)
        assert (R * R) % M.MTPB != 0 and (R * R) // M.MTPB * M.MTPB <= i < R * R, (w, i)
        assert 0 <= y < 67 and 0 <= x < 45 and y - half <= M.MT - 1                  # in the image, and seen by tile 0's outputs


@pytest.mark.parametrize("name", list(M.PROBE_CASES))
def test_planted_faults_move_every_case_by_ten_bars(name):
    """Each planted fault that applies moves an image's sum of (1 - map) by >= 10 x the device tolerance of that image
    (affected x 1e-6).  The shift faults apply wherever the image has a second column / row; the padding fault where a
    probe's own window reaches past a border (elsewhere it moves the sum by next to nothing, which is why those images need
    a shift fault that counts); the dropped tap always."""
    case = M.probe_case(name)
    bar = case["affected"] * M.PIXEL_BAR
    effects = M.fault_effects(case)
    assert set(effects) == set(M.FAULTS)
    assert effects["shift_col"][1].all() and effects["shift_row"][1].all() and effects["drop_tap"][1].all()
    smallest = min(float((e[ap] / bar[ap]).min()) for e, ap in effects.values() if ap.any())
    rep, leaves = effects["replicate"]
    print(f"\n[{name}] smallest planted-fault effect / bar = {smallest:.1f}; padding fault where it does not apply: "
          f"{float(rep[~leaves].max()) if (~leaves).any() else 0.0:.1e}")
    for fault, (e, ap) in effects.items():
        bad = np.nonzero(ap & (e < 10 * bar))[0]
        assert bad.size == 0, (name, fault, [(int(i), e[i], bar[i]) for i in bad[:4]])
    assert smallest >= 10.0


def _grid_cases():
    for name, case in M.probe_cases():
        yield name, case["a"], case["b"]
    for (H, W) in M.SMALL_SHAPES:
        for C in M.SMALL_C:
            a, b = M.grid_pair((1, C, H, W), seed=500 + 41 * H + W)
            yield f"small_{C}x{H}x{W}", a, b
    yield "mixed_dtypes_grid", *M.grid_pair((2, 3, 40, 37), seed=77)


def test_l1_and_mse_sums_are_exact_on_the_grid():
    """every |a - b| a multiple of 2^-8, every (a - b)^2 of 2^-16, every sum under 2^36 units: exact in any order"""
    biggest = 0
    for name, a, b in _grid_cases():
        i1, i2 = M.check_caps(M.mapped(a, "pm1"), M.mapped(b, "pm1"))
        biggest = max(biggest, int(i1.max()), int(i2.max()))
    assert 0 < biggest < 2 ** 36
    print("\nlargest sum: %d units (2^%.1f)" % (biggest, np.log2(biggest)))
    # off the grid the check refuses
    import torch
    x = torch.full((1, 1, 2, 2), 0.1)
    with pytest.raises(AssertionError):
        M.check_caps(M.mapped(x, "pm1"), M.mapped(-x, "pm1"))


def test_closed_form_of_the_single_pixel():
    for w in M.SMALL_WINDOWS:
        a, b = np.array([[[[0.25]]]]), np.array([[[[0.75]]]])
        assert abs(M.ssim_map(a, b, w)[0, 0, 0, 0] - M.closed_form_1x1(0.25, 0.75, w)) <= 1e-15
