"""The image-metrics kernel (csrc/metrics.hip) held to its float64 oracle pixel by pixel (tests/_metrics_oracle.py).

tests/test_metrics_gpu.py compares one mean per image with 1e-6: a single wrong pixel of a 3 x 256 x 256 image is averaged
away.  Here

* probe pairs (b = a but for a few pixels) make S = C H W (1 - ssim) a sum over the few pixels whose window holds a probe;
  S is held to `affected x 1e-6`, the documented 1e-6 per PIXEL.  The probes sit where single pixels go wrong: image corners
  (zero padding), tile seams and their halos, the ragged last tile, the column pairs of the horizontal pass, the row groups
  of the vertical pass, the last partial round of the halo load, and planes / partials that only a wrong base or a second
  trip of the final reduction's loop would mix up (each position's source line: tests/_metrics_oracle.py);
* images smaller than the window, down to 1 x 1 (closed form);
* more partials (260) than the final reduction has threads;
* all nine fp32 / bf16 / fp16 pairs, both sides contiguous and one an NHWC view, and u8 against fp32 through the C ABI;
* L1 and MSE bit for bit on grid values (tests/test_metrics_local_cpu.py shows their sums exact in any order), PSNR bit for
  bit from MSE.

Measured on an MI355X, the largest |S_got - S_want| / bar of the probe cases is 0.242 (test_probe_pairs_per_pixel).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _metrics_oracle as M

pytestmark = pytest.mark.gpu
BAR = 1e-6


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    M.clear_caches()


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _host(m):
    return {k: v.cpu().numpy() for k, v in m.items()}


def _check_psnr(m):
    """psnr == -10 log10(mse) bit for bit, +inf where the pair is identical"""
    mse = m["mse"].cpu()
    want = -10.0 * torch.log10(mse)
    assert torch.equal(m["psnr"].cpu(), want)
    zero = mse == 0
    assert bool(torch.isinf(want[zero]).all()) and bool((want[zero] > 0).all())


def _check_sums_exact(m, a01, b01, what):
    """grid values: l1 and mse equal the oracle's sum * (1.0 / N) to the last bit"""
    _, _, l1, mse = M.sums(a01, b01)
    got = _host(m)
    assert np.array_equal(_bits(got["l1"]), _bits(l1)), (what, "l1", got["l1"], l1)
    assert np.array_equal(_bits(got["mse"]), _bits(mse)), (what, "mse", got["mse"], mse)
    _check_psnr(m)


def _check_sums_close(l1_got, mse_got, a01, b01, what):
    """off the grid the float64 sums are rounded, in the kernel's order and in the oracle's: 1e-13 relative, per image"""
    _, _, l1, mse = M.sums(a01, b01)
    assert (l1 > 0).all() and (mse > 0).all()
    assert (np.abs(l1_got - l1) <= 1e-13 * l1).all() and (np.abs(mse_got - mse) <= 1e-13 * mse).all(), (what, l1_got, l1, mse_got, mse)


def _run_probe_case(dev, name, case, place=lambda t: t):
    """-> the largest |S_got - S_want| / bar of the case's images; asserts it <= 1, and L1 / MSE exactly"""
    from mmhand_amd.metrics import image_metrics
    B, Cc, H, W = case["shape"]
    n = Cc * H * W
    m = image_metrics(place(case["a"].to(dev)), place(case["b"].to(dev)), range="pm1", window=case["window"])
    got = _host(m)
    assert got["ssim"].dtype == np.float64 and got["ssim"].shape == (B,)
    S_got = n * (1.0 - got["ssim"])
    bar = case["affected"] * M.PIXEL_BAR
    ratio = np.abs(S_got - case["S"]) / bar
    worst = int(np.argmax(ratio))
    print(f"\n[{name}] worst |S_got - S_want| / bar = {ratio[worst]:.3f} at image {worst} "
          f"(probes {[p for p in case['probes'] if p[0] == worst]}, {case['why'][worst] if len(case['why']) == B else ''})")
    bad = np.nonzero(~(ratio <= 1.0))[0]
    assert bad.size == 0, (name, [(int(i), [p for p in case["probes"] if p[0] == i], S_got[i], case["S"][i], bar[i]) for i in bad[:6]])
    a01, b01 = M.mapped(case["a"], "pm1"), M.mapped(case["b"], "pm1")
    _check_sums_exact(m, a01, b01, name)
    per_image = np.bincount([p[0] for p in case["probes"]], minlength=B)      # each probe: |a01 - b01| = 1/2 at one pixel
    assert np.array_equal(got["l1"], per_image * 0.5 * (1.0 / n)) and np.array_equal(got["mse"], per_image * 0.25 * (1.0 / n))
    if (per_image == 1).all():
        assert (got["l1"] == 0.5 / n).all() and (got["mse"] == 0.25 / n).all(), (got["l1"], got["mse"])
    return float(ratio[worst])


@pytest.mark.parametrize("window", M.WINDOWS)
@pytest.mark.parametrize("shape", list(M.SINGLE_SHAPES))
def test_probe_pairs_per_pixel(dev, shape, window):
    """One probe per image, one image per position (corners, seams, ragged tile, column pair, row group, last load round).
    Measured on an MI355X, |S_got - S_want| / bar, the largest per case: 67 x 45: 0.242 (window 3, corner (0, 44)), 0.083 (5),
    0.027 (11), 0.016 (15); 33 x 33: 0.078, 0.051, 0.026, 0.016; the B = 3, C = 4 and the 260-partial cases below: 0.012 and
    less.  The largest of the file is 0.242, so the bar stays at affected x 1e-6."""
    _run_probe_case(dev, f"{shape}_w{window}", M.single_probe_case(shape, window))


def _nhwc_view(t, cs=8):
    """the same values as an NCHW view of an NHWC buffer with `cs` channels per pixel (the spare ones poisoned)"""
    B, Cc, H, W = t.shape
    buf = torch.full((B, H, W, cs), float("nan"), dtype=t.dtype, device=t.device)
    buf[..., :Cc] = t.permute(0, 2, 3, 1)
    v = buf.permute(0, 3, 1, 2)[:, :Cc]
    assert not v.is_contiguous() and v.stride(1) == 1 and v.stride(3) == cs and torch.equal(v, t)
    return v


@pytest.mark.parametrize("layout", ["contiguous", "nhwc_cs8"])
@pytest.mark.parametrize("window", M.PLANES_WINDOWS)
def test_every_plane_carries_its_own_probe(dev, window, layout):
    """B = 3, C = 4, every (b, c) plane probed at another position: a wrong sb / sc base or a partial written to another
    plane's slot changes some image's S"""
    _run_probe_case(dev, f"planes_w{window}_{layout}", M.planes_case(window), _nhwc_view if layout == "nhwc_cs8" else (lambda t: t))


@pytest.mark.parametrize("B", [1, 2])
def test_more_partials_than_final_threads(dev, B):
    """C = 65 at 33 x 33: 4 tiles x 65 = 260 partials per image, so image_metrics_final_kernel's loop takes a second trip;
    probes in channel 64 (partials 256 .. 259) and channel 0"""
    case = M.many_partials_case(B)
    Cc, H, W = case["shape"][1:]
    tiles = ((H + M.MT - 1) // M.MT) * ((W + M.MT - 1) // M.MT)
    assert Cc * tiles > 256
    from mmhand_amd import lib as L
    assert L.load().mmh_image_metrics_ws_bytes(B, Cc, H, W, case["window"]) == B * Cc * tiles * 3 * 8
    _run_probe_case(dev, f"many_partials_B{B}", case)


@pytest.mark.parametrize("C_", M.SMALL_C)
@pytest.mark.parametrize("window", M.SMALL_WINDOWS)
def test_images_smaller_than_the_window(dev, window, C_):
    """1 x 1 .. 3 x 3, 1 x 40, 40 x 1: every window hangs over every border.  At most 120 pixels: the mean is local."""
    from mmhand_amd.metrics import image_metrics
    worst = 0.0
    for (H, W) in M.SMALL_SHAPES:
        a, b = M.grid_pair((1, C_, H, W), seed=500 + 41 * H + W)
        a01, b01 = M.mapped(a, "pm1"), M.mapped(b, "pm1")
        want = M.ssim_map(a01, b01, window).mean(axis=(1, 2, 3))
        m = image_metrics(a.to(dev), b.to(dev), range="pm1", window=window)
        got = _host(m)
        err = float(np.abs(got["ssim"] - want).max())
        worst = max(worst, err)
        assert err <= BAR, (H, W, C_, window, got["ssim"], want)
        _check_sums_exact(m, a01, b01, (H, W, C_, window))
        if (H, W, C_) == (1, 1, 1):
            closed = M.closed_form_1x1(a01[0, 0, 0, 0], b01[0, 0, 0, 0], window)
            assert abs(got["ssim"][0] - closed) <= BAR and abs(want[0] - closed) <= 1e-15, (got["ssim"], want, closed)
        same = _host(image_metrics(a.to(dev), a.to(dev), range="pm1", window=window))
        assert (same["ssim"] == 1.0).all() and (same["l1"] == 0).all() and np.isposinf(same["psnr"]).all()
    print(f"\n[small w{window} C{C_}] worst |ssim - oracle| = {worst:.2e}")


# ------------------------------------------------------------------------------------------------- dtypes and layouts
MIXED_SHAPE = (2, 3, 40, 37)
_TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module")
def mixed_pair():
    """fp32 values OFF the grid, so that each 16-bit side's own rounding matters: a in [-1, 1), b = a + 0.2 noise, clipped"""
    from tests._hpe_oracle import hashed
    n = int(np.prod(MIXED_SHAPE))
    a = hashed(7100, n).reshape(MIXED_SHAPE)
    b = np.clip(a + 0.2 * hashed(7101, n).reshape(MIXED_SHAPE), -1, 1)
    return torch.from_numpy(a.astype(np.float32)), torch.from_numpy(b.astype(np.float32))


@pytest.mark.parametrize("layout", ["contiguous", "b_nhwc"])
@pytest.mark.parametrize("tb", list(_TORCH))
@pytest.mark.parametrize("ta", list(_TORCH))
def test_mixed_dtypes_and_layouts(dev, mixed_pair, ta, tb, layout):
    """every (dtype of a, dtype of b) branch of load_halos, against the oracle on what each side holds after its own rounding"""
    from mmhand_amd.metrics import image_metrics
    a, b = mixed_pair[0].to(_TORCH[ta]), mixed_pair[1].to(_TORCH[tb])
    a01, b01 = M.mapped(a, "pm1"), M.mapped(b, "pm1")
    want = M.ssim_map(a01, b01, 11).mean(axis=(1, 2, 3))
    da, db = a.to(dev), b.to(dev)
    if layout == "b_nhwc":
        db = _nhwc_view(db, cs=4)
    ab, ba = image_metrics(da, db, range="pm1", window=11), image_metrics(db, da, range="pm1", window=11)
    got = _host(ab)
    err = float(np.abs(got["ssim"] - want).max())
    print(f"\n[{ta} x {tb} {layout}] |ssim - oracle| = {err:.2e}")
    assert err <= BAR, (ta, tb, layout, got["ssim"], want)
    _check_sums_close(got["l1"], got["mse"], a01, b01, (ta, tb, layout))
    _check_psnr(ab)
    for k in ("ssim", "l1", "mse", "psnr"):
        assert torch.equal(ab[k], ba[k]), (ta, tb, layout, k)
    # grid values are exact in all three types: whatever the pair of types, L1 and MSE to the last bit
    ga, gb = M.grid_pair(MIXED_SHAPE, seed=77)
    g01a, g01b = M.mapped(ga, "pm1"), M.mapped(gb, "pm1")
    assert np.array_equal(M.mapped(ga.to(_TORCH[ta]), "pm1"), g01a) and np.array_equal(M.mapped(gb.to(_TORCH[tb]), "pm1"), g01b)
    dgb = gb.to(_TORCH[tb]).to(dev)
    mg = image_metrics(ga.to(_TORCH[ta]).to(dev), _nhwc_view(dgb, cs=4) if layout == "b_nhwc" else dgb, range="pm1", window=11)
    _check_sums_exact(mg, g01a, g01b, (ta, tb, layout, "grid"))
    assert np.abs(_host(mg)["ssim"] - M.ssim_map(g01a, g01b, 11).mean(axis=(1, 2, 3))).max() <= BAR


def _abi(sa, sb, shape, window, dev):
    """mmh_image_metrics on two mmh_image_src descriptors, as mmhand_amd.metrics.image_metrics calls it"""
    from mmhand_amd import lib as L
    from mmhand_amd.metrics import C1, C2, gaussian_taps
    from mmhand_amd.ops import _ptr, _stream
    B, Cc, H, W = shape
    nbytes = L.load().mmh_image_metrics_ws_bytes(B, Cc, H, W, window)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((B, 3), dtype=torch.float64, device=dev)
    taps = gaussian_taps(window)
    L.call("mmh_image_metrics", C.byref(sa), C.byref(sb), B, Cc, H, W, window, taps.ctypes.data_as(C.c_void_p), C1, C2,
           _ptr(ws), nbytes, _ptr(out), _stream())
    return out.cpu().numpy()


def _u8_pair():
    k = M.grid((2, 40, 37, 3), seed=9, tensor_index=7200)
    d = M.grid((2, 40, 37, 3), seed=9, tensor_index=7201) % 41 - 20
    return torch.from_numpy(k.astype(np.uint8)), torch.from_numpy(np.clip(k + d, 0, 255).astype(np.uint8))


def _fp32_near(u):
    """an fp32 NCHW image in [-1, 1] near the u8 one (RGB order), off the 1/255 lattice"""
    from tests._hpe_oracle import hashed
    rgb = u.flip(-1).permute(0, 3, 1, 2).double().numpy() / 255.0
    noise = 0.1 * hashed(7300, rgb.size).reshape(rgb.shape)
    return torch.from_numpy(np.clip(2.0 * rgb - 1.0 + noise, -1, 1).astype(np.float32))


def test_u8_against_fp32_through_the_c_abi(dev):
    """u8 x fp32 and fp32 x u8: the u8 side B,G,R bytes with 1/255, 0 (scored as RGB), the fp32 side NCHW with 0.5, 0.5"""
    from mmhand_amd.metrics import _src
    u, _ = _u8_pair()
    f = _fp32_near(u)
    du, df = u.to(dev), f.to(dev)
    su, shape_u = _src(du, "u8_bgr_hwc")
    sf, shape_f = _src(df, "pm1")
    assert shape_u == shape_f == (2, 3, 40, 37)
    u01, f01 = M.mapped(u, "u8_bgr_hwc"), M.mapped(f, "pm1")
    want = M.ssim_map(u01, f01, 11).mean(axis=(1, 2, 3))
    uf, fu = _abi(su, sf, shape_u, 11, dev), _abi(sf, su, shape_u, 11, dev)
    err = float(np.abs(uf[:, 0] - want).max())
    print(f"\n[u8 x f32] |ssim - oracle| = {err:.2e}")
    assert err <= BAR, (uf[:, 0], want)
    _check_sums_close(uf[:, 1], uf[:, 2], u01, f01, "u8 x f32")
    assert np.array_equal(_bits(uf), _bits(fu))


def test_u8_pair_l1_and_mse(dev):
    """u8 / 255 is not dyadic: the oracle applies the kernel's fp32 map, the sums agree to 1e-13 relative"""
    from mmhand_amd.metrics import image_metrics
    a, b = _u8_pair()
    a01, b01 = M.mapped(a, "u8_bgr_hwc"), M.mapped(b, "u8_bgr_hwc")
    want = M.ssim_map(a01, b01, 11).mean(axis=(1, 2, 3))
    m = image_metrics(a.to(dev), b.to(dev), range="u8_bgr_hwc", window=11)
    got = _host(m)
    assert np.abs(got["ssim"] - want).max() <= BAR, (got["ssim"], want)
    _check_sums_close(got["l1"], got["mse"], a01, b01, "u8 x u8")
    _check_psnr(m)
