"""Element-wise, integer-exact checks of the convolution kernels against the float64 oracle (tests/_exact.py).

The rel-L1 tests of tests/test_conv_gpu.py answer "is the rounding right on average"; one wrong corner pixel, a dropped tap
at a ragged tile edge or one unwritten element passes them.  On inputs in {-1, 0, 1} every product and partial sum is an
exact integer, so a correct DIRECT kernel - fp32, or bf16 / fp16 operands with fp32 accumulation - equals the oracle bit for
bit whatever its order of summation (assert_exact, which names the first differing element); fp32 Winograd (non-dyadic
transform constants) must ROUND to the oracle, element by element (assert_rounds: a derived bound of 0.5).

One parametrised test per kernel family, through the wrapper the family's rel-L1 test uses, with that test's check that the
intended kernel ran, at the smallest ragged shapes the family already has.  The cases live in tests/_exact.py; the caps
(results integer-valued and within the exact range of the type that stores them) are asserted inside E.case_problem on the
oracle alone, before anything is compared, and again without a GPU by tests/test_conv_exact_cpu.py.
These capped families test the SUMS: with every result inside the exact range of its storage type no 16-bit store here ever
rounds, so a kernel that truncates, rounds twice or saturates passes this file.  The STORE is tested by the round-once families
of tests/_exact.py in tests/test_conv_round16_gpu.py (results that do not fit the 16-bit type, held to RNE bit for bit).
Statistics by-products of epilogues are not integer quantities: only conv outputs are compared here.
The templates, work partitions and mmh_set_option knobs that only larger shapes select are in tests/test_conv_variants_gpu.py."""
import ctypes
from collections import Counter

import pytest
import torch

from tests import _exact as E

pytestmark = pytest.mark.gpu

LP = pytest.mark.parametrize("lp", [True, 2], ids=["bf16", "fp16"])


def _spy(monkeypatch):
    """C-ABI call names -> counts, from here to the end of the test"""
    from mmhand_amd import lib
    calls = Counter()
    real = lib.call

    def spy(name, *a):
        calls[name] += 1
        return real(name, *a)
    monkeypatch.setattr(lib, "call", spy)
    return calls


def _dev(P, dev):
    return P.x.to(dev), P.w.to(dev), P.bias.to(dev), P.dy.to(dev)


def _relu(t):
    return t.clamp_min(0.0)


# ============================================================================================ fp32 direct kernels
@pytest.mark.parametrize("case", E.IGEMM)
def test_exact_igemm_fprop_dgrad_wgrad_colsum(case, dev, monkeypatch):
    """raw_conv_fprop / raw_conv_dgrad / raw_conv_wgrad / raw_colsum with Winograd off (the 7x7 cases take the stem, thin and
    generic kernels exactly as tests/test_conv_gpu.py::test_conv2d_fprop_dgrad_wgrad routes them)"""
    from mmhand_amd import ops
    B, H, W, Cin, Cout, k, s, p, refl = case
    monkeypatch.setattr(ops, "USE_WINOGRAD", False)
    assert ops._wino_tile(B, H, W, Cin, Cout, k, s, p, False) == 0
    P = E.case_problem("igemm", case)
    x, w, bias, dy = _dev(P, dev)
    E.assert_exact(ops.raw_conv_fprop(x, w, bias, s, p, refl, 0), P.y, "fprop")
    E.assert_exact(ops.raw_conv_fprop(x, w, bias, s, p, refl, 1), _relu(P.y), "fprop + relu")
    E.assert_exact(ops.raw_conv_dgrad(dy, w, x.shape, s, p, refl), P.dx, "dgrad")
    E.assert_exact(ops.raw_conv_wgrad(x, dy, k, s, p, refl), P.dw, "wgrad")
    E.assert_exact(ops.raw_colsum(dy.numel() // Cout, Cout, dy), P.db, "bias gradient")


@pytest.mark.parametrize("case", E.IGEMM[3:5])
def test_exact_igemm_generic_kernels_of_the_7x7_shapes(case, dev, monkeypatch):
    """the same 7x7 shapes on the generic implicit-GEMM kernels they had before the stem / thin kernels took them"""
    from mmhand_amd import lib, ops
    B, H, W, Cin, Cout, k, s, p, refl = case
    monkeypatch.setattr(ops, "USE_THIN", False)
    monkeypatch.setattr(ops, "USE_STEM_WGRAD", False)
    P = E.case_problem("igemm", case)
    x, w, bias, dy = _dev(P, dev)
    calls = _spy(monkeypatch)
    lib.call("mmh_set_option", b"stem_f32", 0)
    try:
        y = ops.raw_conv_fprop(x, w, bias, s, p, refl, 0)
    finally:
        lib.call("mmh_set_option", b"stem_f32", 1)
    dx = ops.raw_conv_dgrad(dy, w, x.shape, s, p, refl)
    dw = ops.raw_conv_wgrad(x, dy, k, s, p, refl)
    assert calls["mmh_conv2d_fprop"] == 1 and calls["mmh_conv2d_dgrad_folded"] == 1 and calls["mmh_conv2d_wgrad"] == 1, calls
    E.assert_exact(y, P.y, "fprop"); E.assert_exact(dx, P.dx, "dgrad"); E.assert_exact(dw, P.dw, "wgrad")


@pytest.mark.parametrize("case", E.LEVELS2, ids=lambda c: c[0])
def test_exact_two_level_direct_fprop(case, dev, monkeypatch):
    """mmh_set_option("conv_levels", 2): a fresh MFMA chain per k-step folded by vector adds - another order, the same integers"""
    from mmhand_amd import lib, ops
    kind, B, H, W, Cin, Cout = case
    s, refl = (2, False) if kind == "s2" else (1, True)
    monkeypatch.setattr(ops, "USE_WINOGRAD", False)
    P = E.case_problem("levels2", case)
    x, w, bias, _ = _dev(P, dev)
    ops.bump_weights_epoch()
    lib.call("mmh_set_option", b"conv_levels", 2)
    try:
        y2 = ops.raw_conv_fprop(x, w, bias, s, 1, refl, 1)
    finally:
        lib.call("mmh_set_option", b"conv_levels", 1)
    y1 = ops.raw_conv_fprop(x, w, bias, s, 1, refl, 1)
    E.assert_exact(y2, _relu(P.y), "two-level fprop + relu")
    E.assert_exact(y1, _relu(P.y), "one-level fprop + relu")


@pytest.mark.parametrize("case", E.CONVT)
def test_exact_convT(case, dev):
    from mmhand_amd import ops
    B, h, w_, CinT, CoutT = case
    P = E.case_problem("convT", case)
    x, w, bias, dy = _dev(P, dev)
    y = ops.raw_convT_fprop(x, w, bias)
    assert tuple(y.shape) == (B, 2 * h, 2 * w_, CoutT)
    E.assert_exact(y, P.y, "convT fprop")
    E.assert_exact(ops.raw_convT_dgrad(dy, w, x.shape), P.dx, "convT dgrad")
    E.assert_exact(ops.raw_convT_wgrad(x, dy), P.dw, "convT wgrad")


@pytest.mark.parametrize("case", E.DGRAD_S2 + E.DGRAD_S2_PERSISTENT)
def test_exact_dgrad_s2_halo(case, dev):
    """dgrad_s2.hip: whole and ragged 8 x 16 tiles, one-tile images, and 384 tiles on 256 CUs (the persistent loop's second
    tile, whose halo chunks are requested while the first tile multiplies)"""
    from mmhand_amd import lib, ops
    B, H, W, Cin, Cout = case
    assert lib.load().mmh_dgrad_s2_halo_supported(ctypes.byref(ops.conv_desc(B, H, W, Cin, Cout, 3, 2, 1, False)), Cin) == 1
    P = E.case_problem("dgrad_s2", case)
    _, w, _, dy = _dev(P, dev)
    E.assert_exact(ops.raw_conv_dgrad(dy, w, (B, H, W, Cin), 2, 1, False), P.dx, "dgrad_s2")


@pytest.mark.parametrize("case", E.WGRAD_S2)
def test_exact_wgrad_s2_strip(case, dev, monkeypatch):
    """wgrad_s2.hip (ragged strips of 16 dy positions, split row ranges) and, with the option off, the generic kernel"""
    from mmhand_amd import lib, ops
    B, H, W, Cin, Cout = case
    P = E.case_problem("wgrad_s2", case)
    x, _, _, dy = _dev(P, dev)
    E.assert_exact(ops.raw_conv_wgrad(x, dy, 3, 2, 1, False), P.dw, "wgrad_s2 strip kernel")
    lib.call("mmh_set_option", b"wgrad_s2_strip", 0)
    try:
        dw0 = ops.raw_conv_wgrad(x, dy, 3, 2, 1, False)
    finally:
        lib.call("mmh_set_option", b"wgrad_s2_strip", 1)
    E.assert_exact(dw0, P.dw, "wgrad_s2 generic kernel")


@pytest.mark.parametrize("case", E.STEM_F32)
def test_exact_conv_stem_f32(case, dev, monkeypatch):
    """conv_stem_f32.hip: ragged 16 x 16 tiles, reflect and zero padding, one to four filter phases; one and two levels"""
    from mmhand_amd import lib, ops
    B, H, W, Cin, refl = case
    P = E.case_problem("stem_f32", case)
    x, w, bias, _ = _dev(P, dev)
    calls = _spy(monkeypatch)
    E.assert_exact(ops.raw_conv_fprop(x, w, bias, 1, 3, refl, 0), P.y, "stem fprop")
    E.assert_exact(ops.raw_conv_fprop(x, w, bias, 1, 3, refl, 1), _relu(P.y), "stem fprop + relu")
    assert calls["mmh_conv2d_fprop"] == 2 and len(calls) == 1, calls
    lib.call("mmh_set_option", b"conv_levels", 2)
    try:
        y2 = ops.raw_conv_fprop(x, w, bias, 1, 3, refl, 0)
    finally:
        lib.call("mmh_set_option", b"conv_levels", 1)
    E.assert_exact(y2, P.y, "stem fprop, two levels")


@pytest.mark.parametrize("case", E.STEM_WGRAD_F32)
def test_exact_stem_wgrad_f32(case, dev, monkeypatch):
    from mmhand_amd import lib, ops
    B, H, W, Cin = case
    assert lib.load().mmh_conv7_stem_wgrad_supported(ctypes.byref(ops.conv_desc(B, H, W, Cin, 64, 7, 1, 3, True))) == 1
    P = E.case_problem("stem_wgrad_f32", case)
    x, _, _, dy = _dev(P, dev)
    calls = _spy(monkeypatch)
    dw = ops.raw_conv_wgrad(x, dy, 7, 1, 3, True)
    assert calls["mmh_conv7_stem_wgrad"] == 1 and "mmh_conv2d_wgrad" not in calls, calls
    E.assert_exact(dw, P.dw, "stem wgrad")


@pytest.mark.parametrize("case", E.THIN)
def test_exact_thin_conv7(case, dev, monkeypatch):
    """conv_thin.hip: fprop of a 4-column 7x7 conv, its dgrad restricted to the first input channels (the other channels
    come back as zeros) and, at 64-channel chunks, its wgrad"""
    from mmhand_amd import ops
    B, H, W, Cin, Cout, refl = case
    assert ops.USE_THIN
    P = E.case_problem("thin", case)
    x, w, bias, dy = _dev(P, dev)
    calls = _spy(monkeypatch)
    E.assert_exact(ops.raw_conv_fprop(x, w, bias, 1, 3, refl, 0), P.y, "thin fprop")
    E.assert_exact(ops.raw_conv_fprop(x, w, bias, 1, 3, refl, 1), _relu(P.y), "thin fprop + relu")
    assert calls["mmh_conv7_thin_fprop"] == 2, calls
    dx = ops.raw_conv_dgrad(dy, w, (B, H, W, Cin), 1, 3, refl, dx_channels=3)
    assert calls["mmh_conv7_thin_dgrad"] == 1, calls
    E.assert_exact(dx[..., :4], P.dx[..., :4].contiguous(), "thin dgrad, channels [0, 4)")
    assert not dx[..., 4:].any()
    if Cin % 64 == 0:
        dw = ops.raw_conv_wgrad(x, dy, 7, 1, 3, refl)
        assert calls["mmh_conv7_thin_wgrad"] == 1, calls
        E.assert_exact(dw, P.dw, "thin wgrad")


@pytest.mark.parametrize("case", E.THIN_WGRAD)
def test_exact_thin_conv7_wgrad(case, dev, monkeypatch):
    from mmhand_amd import ops
    B, H, W, Cin = case
    assert ops.USE_THIN
    P = E.case_problem("thin_wgrad", case)
    x, _, _, dy = _dev(P, dev)
    calls = _spy(monkeypatch)
    dw = ops.raw_conv_wgrad(x, dy, 7, 1, 3, True)
    assert calls["mmh_conv7_thin_wgrad"] == 1, calls
    E.assert_exact(dw, P.dw, "thin wgrad")


def test_exact_colsum(dev):
    """5000 x 256 integers: the fixed-order split sums are exact, in fp32 and from both 16-bit types"""
    from mmhand_amd import ops
    rows, cols = E.COLSUM
    t = E.ints((rows, cols), 11)
    want = t.double().sum(0)
    E.assert_exact(ops.raw_colsum(rows, cols, t.to(dev)), want, "colsum fp32")
    for lp in (True, 2):
        E.assert_exact(ops.raw_colsum(rows, cols, t.to(dev).to(ops._wd(lp))), want, f"colsum {ops._wd(lp)}")
    acc = E.ints((cols,), 12, lo=-8, hi=8)
    E.assert_exact(ops.raw_colsum(rows, cols, t.to(dev), out=acc.to(dev)), want + acc.double(), "colsum, accumulating")


# ============================================================================================ 16-bit kernels
def _twins(ops, lp, *ts):
    out = [ops.lp16_twin(t, lp) for t in ts]
    return out if len(out) > 1 else out[0]


@LP
@pytest.mark.parametrize("shape", [17, 19], ids=["rowtile", "halo"])
@pytest.mark.parametrize("case", E.HALO_FPROP)
def test_exact_conv3x3_lp16_fprop(case, shape, lp, dev):
    """conv_lp16_halo.hip (19) and the row-tile kernel of conv_lp16.hip (17, which images below 16 x 16 always take): fp32
    and 16-bit epilogues, bias + ReLU"""
    from mmhand_amd import lib, ops
    B, H, W, Cin, Cout, refl = case
    P = E.case_problem("halo_fprop", case)
    x, w, bias, _ = _dev(P, dev)
    lib.check(lib.load().mmh_set_option(b"lp16_shape", shape), "set")
    try:
        ops.bump_weights_epoch()
        x16 = _twins(ops, lp, x)
        E.assert_exact(x16, P.x.double(), "16-bit twin of x")
        y = ops.raw_conv3x3_lp16(x16, w, bias, refl, 1, lp, 0)
        y16 = ops.raw_conv3x3_lp16(x16, w, bias, refl, 0, lp, 0, out16=True)
    finally:
        lib.check(lib.load().mmh_set_option(b"lp16_shape", 19), "set")
    assert y16.dtype == ops._wd(lp)
    E.assert_exact(y, _relu(P.y), "fprop + relu, fp32 out")
    E.assert_exact(y16, P.y, "fprop, 16-bit out")


@LP
@pytest.mark.parametrize("out16", [False, True], ids=["dx32", "dx16"])
@pytest.mark.parametrize("case", E.FOLD_DGRAD)
def test_exact_conv3x3_lp16_reflect_dgrad(case, out16, lp, dev, monkeypatch):
    """the dgrad of a ReflectionPad2d(1) conv from a 16-bit dy: in-kernel fold where the image has two tiles each way, else
    the zero-pad kernel + mmh_conv2d_dgrad_border (the route of these one-tile-in-one-direction shapes)"""
    from mmhand_amd import lib, ops
    B, H, W, Cin, Cout = case
    P = E.case_problem("fold_dgrad", case)
    _, w, _, dy = _dev(P, dev)
    ops.bump_weights_epoch()
    dy16 = _twins(ops, lp, dy)
    d = ops.conv_desc(B, H, W, Cin, Cout, 3, 1, 1, True)
    d.dtype = ops._dt(lp)
    folds = min(H, W) >= 32
    assert lib.load().mmh_conv3x3_lp16_fold_supported(ctypes.byref(d)) == int(folds)
    calls = _spy(monkeypatch)
    dx = ops.raw_conv_dgrad(None, w, (B, H, W, Cin), 1, 1, True, bf16=lp, dy16=dy16, out16=out16)
    assert calls["mmh_conv3x3_lp16"] == 1 and ("mmh_conv2d_dgrad_border" not in calls) == folds, calls
    assert dx.dtype == (ops._wd(lp) if out16 else torch.float32)
    E.assert_exact(dx, P.dx, "reflect dgrad")


@LP
@pytest.mark.parametrize("case", E.FOLD_IN_KERNEL)
def test_exact_conv3x3_lp16_in_kernel_fold(case, lp, dev, monkeypatch):
    """mode 2 itself (ring rows, columns and corners folded inside the halo kernel): 2 x 2 tiles, every tile a corner, and
    2 x 3 tiles with an edge tile that folds one term - the smallest shapes that take it, with and without the addend"""
    from mmhand_amd import lib, ops
    B, H, W, Cin, Cout = case
    P = E.case_problem("fold_in_kernel", case)
    _, w, _, dy = _dev(P, dev)
    ops.bump_weights_epoch()
    dy16 = _twins(ops, lp, dy)
    d = ops.conv_desc(B, H, W, Cin, Cout, 3, 1, 1, True)
    d.dtype = ops._dt(lp)
    assert lib.load().mmh_conv3x3_lp16_fold_supported(ctypes.byref(d)) == 1
    calls = _spy(monkeypatch)
    for out16 in (False, True):
        dx = ops.raw_conv_dgrad(None, w, (B, H, W, Cin), 1, 1, True, bf16=lp, dy16=dy16, out16=out16)
        E.assert_exact(dx, P.dx, f"in-kernel fold, out16={out16}")
    addend = E.ints((B, H, W, Cin), E.SEED_ADD, lo=-8, hi=8)
    dxa = ops.raw_conv_dgrad(None, w, (B, H, W, Cin), 1, 1, True, bf16=lp, dy16=dy16, addend=addend.to(dev))
    assert calls["mmh_conv3x3_lp16"] == 2 and calls["mmh_conv3x3_lp16_dgrad_add"] == 1 and "mmh_conv2d_dgrad_border" not in calls, calls
    E.assert_exact(dxa, P.dx + addend.double(), "in-kernel fold + addend")


@LP
@pytest.mark.parametrize("case", E.DGRAD_ADD)
def test_exact_conv3x3_lp16_dgrad_with_addend(case, lp, dev, monkeypatch):
    from mmhand_amd import ops
    B, H, W, Cin, Cout, refl = case
    P = E.case_problem("dgrad_add", case)
    _, w, _, dy = _dev(P, dev)
    addend = E.ints((B, H, W, Cin), E.SEED_ADD, lo=-8, hi=8)
    ops.bump_weights_epoch()
    dy16 = _twins(ops, lp, dy)
    calls = _spy(monkeypatch)
    dx = ops.raw_conv_dgrad(None, w, (B, H, W, Cin), 1, 1, refl, bf16=lp, dy16=dy16, addend=addend.to(dev))
    fused = H >= 16 and W >= 16 and (not refl or (H % 16 == 0 and W % 16 == 0 and min(H, W) >= 32))
    assert (calls["mmh_conv3x3_lp16_dgrad_add"] == 1) == fused, calls
    assert ("mmh_conv2d_dgrad_border" in calls) == (refl and not fused), calls
    E.assert_exact(dx, P.dx + addend.double(), "dgrad + addend")


@LP
@pytest.mark.parametrize("case", E.SLICE)
def test_exact_conv3x3_lp16_reads_a_channel_slice(case, lp, dev):
    """the halo fprop and the nine-tap wgrad read x in place from the second half of a twice-as-wide 16-bit tensor"""
    from mmhand_amd import ops
    B, H, W, Cin, Cout, refl = case
    P = E.case_problem("slice", case)
    x, w, bias, dy = _dev(P, dev)
    wide = _twins(ops, lp, torch.cat((E.ints((B, H, W, Cin), 9).to(dev), x), 3).contiguous())
    view = wide[..., Cin:]
    assert not view.is_contiguous()
    ops.bump_weights_epoch()
    y16 = ops.raw_conv3x3_lp16(view, w, bias, refl, 0, lp, 0, out16=True)
    E.assert_exact(y16, P.y, "fprop from a channel slice, 16-bit out")
    ops._pending_stats.clear()
    ys = ops.raw_conv3x3_lp16(view, w, bias, refl, 0, lp, 0, out16=True, want_stats=True)
    ops._pending_stats.clear()
    E.assert_exact(ys, P.y, "fprop with the statistics epilogue from a channel slice")
    dw = ops.raw_wgrad3x3_lp16(view, _twins(ops, lp, dy), refl, lp)
    E.assert_exact(dw, P.dw, "nine-tap wgrad from a channel slice")


def _lp16g_fprop(ops, P, d_of, lp, dev, what):
    """fprop (fp32 + ReLU, and 16-bit output) of conv d on mmh_conv_lp16"""
    x, w, bias, _ = _dev(P, dev)
    ops.bump_weights_epoch()
    assert ops.lp16g_ok(d_of(), 0, lp)
    x16 = _twins(ops, lp, x)
    E.assert_exact(ops.raw_conv_lp16g(d_of(), 0, x16, w, bias, 1, lp), _relu(P.y), what + " fprop + relu")
    E.assert_exact(ops.raw_conv_lp16g(d_of(), 0, x16, w, bias, 0, lp, out16=True), P.y, what + " fprop, 16-bit out")


def _lp16g_dgrad(ops, P, d_of, lp, dev, what):
    """dgrad (fp32 and 16-bit output) of the zero-padded conv d on mmh_conv_lp16; returns (dy16, w)"""
    _, w, _, dy = _dev(P, dev)
    assert ops.lp16g_ok(d_of(), 1, lp)
    dy16 = _twins(ops, lp, dy)
    E.assert_exact(ops.raw_conv_lp16g(d_of(), 1, dy16, w, None, 0, lp), P.dx, what + " dgrad")
    E.assert_exact(ops.raw_conv_lp16g(d_of(), 1, dy16, w, None, 0, lp, out16=True), P.dx, what + " dgrad, 16-bit out")
    return dy16, w


@LP
@pytest.mark.parametrize("case", E.LP16G)
def test_exact_conv_lp16g(case, lp, dev):
    """conv_lp16g_kernel: stride-2 fprop, the four parity classes of its dgrad, and the ConvTranspose2d forward (that dgrad)
    through raw_convT_fprop"""
    from mmhand_amd import ops
    B, H, W, Cin, Cout, stride, refl = case
    P = E.case_problem("lp16g", case)
    mk = lambda: ops.conv_desc(B, H, W, Cin, Cout, 3, stride, 1, refl)     # noqa: E731
    _lp16g_fprop(ops, P, mk, lp, dev, "lp16g")
    if not refl:
        dy16, w = _lp16g_dgrad(ops, P, mk, lp, dev, "lp16g")
        E.assert_exact(ops.raw_convT_fprop(dy16, w, None, 0, bf16=lp), P.dx, "ConvTranspose2d fprop on the 16-bit dgrad")
        E.assert_exact(ops.raw_conv_dgrad(P.dy.to(dev), w, (B, H, W, Cin), stride, 1, False, lp), P.dx, "raw_conv_dgrad routing")


@LP
@pytest.mark.parametrize("case", E.S2_LP16)
def test_exact_conv_s2_lp16(case, lp, dev):
    """conv_s2_lp16.hip (register-resident weights, de-interleaved LDS halo) behind mmh_conv_lp16: fprop at 64 and - option
    lp16_s2f = 2 - 128 input channels, and the 64 <- 128 dgrad"""
    from mmhand_amd import lib, ops
    B, H, W, Cin, Cout = case
    P = E.case_problem("s2_lp16", case)
    mk = lambda: ops.conv_desc(B, H, W, Cin, Cout, 3, 2, 1, False)     # noqa: E731
    lib.check(lib.load().mmh_set_option(b"lp16_s2f", 2), "set_option")
    try:
        _lp16g_fprop(ops, P, mk, lp, dev, "s2_lp16")
    finally:
        lib.check(lib.load().mmh_set_option(b"lp16_s2f", 1), "set_option")
    _lp16g_dgrad(ops, P, mk, lp, dev, "s2_lp16")


@LP
@pytest.mark.parametrize("case", E.S1_LP16)
def test_exact_conv_s2_lp16_stride1_64_to_64(case, lp, dev):
    """the stride-1 form (VGG conv1_2, 64 -> 64, zero padding) and its input gradient; 40 x 40 stays on the general kernel"""
    from mmhand_amd import ops
    B, H, W = case
    P = E.case_problem("s1_lp16", case)
    mk = lambda: ops.conv_desc(B, H, W, 64, 64, 3, 1, 1, False)     # noqa: E731
    _lp16g_fprop(ops, P, mk, lp, dev, "s1_lp16")
    _lp16g_dgrad(ops, P, mk, lp, dev, "s1_lp16")


@LP
@pytest.mark.parametrize("case", E.FLAT_STEMS)
def test_exact_conv_lp16_flat_stems(case, lp, dev, monkeypatch):
    """conv_lp16f_kernel (flat (tap, channel) contraction, channels padded to 8) - the stem kernel that replaced it off"""
    from mmhand_amd import ops
    B, H, W, Cin, Cout, k, refl = case
    monkeypatch.setattr(ops, "USE_STEM_FPROP16", False)
    P = E.case_problem("flat_stems", case)
    x, w, bias, _ = _dev(P, dev)
    ops.bump_weights_epoch()
    mk = lambda: ops.conv_desc(B, H, W, Cin, Cout, k, 1, k // 2, refl)     # noqa: E731
    assert ops.lp16_flat_ok(mk(), lp)
    calls = _spy(monkeypatch)
    y = ops.raw_conv_lp16_flat(mk(), x, w, bias, 1, lp)
    y16 = ops.raw_conv_lp16_flat(mk(), x, w, bias, 0, lp, out16=True)
    assert calls["mmh_conv_lp16_flat"] == 2 and "mmh_conv_stem16" not in calls, calls
    E.assert_exact(y, _relu(P.y), "flat-K fprop + relu")
    E.assert_exact(y16, P.y, "flat-K fprop, 16-bit out")


@LP
@pytest.mark.parametrize("case", E.STEM16)
def test_exact_conv_stem16(case, lp, dev, monkeypatch):
    from mmhand_amd import ops
    B, H, W, Cin, refl = case
    P = E.case_problem("stem16", case)
    x, w, bias, _ = _dev(P, dev)
    ops.bump_weights_epoch()
    calls = _spy(monkeypatch)
    y = ops.raw_conv_fprop(x, w, bias, 1, 3, refl, 1, lp)
    assert calls["mmh_conv_stem16"] == 1 and "mmh_conv_lp16_flat" not in calls, calls
    y16 = ops.raw_conv_lp16_flat(ops.conv_desc(B, H, W, Cin, 64, 7, 1, 3, refl), x, w, bias, 0, lp, out16=True)
    assert calls["mmh_conv_stem16"] == 2 and "mmh_conv_lp16_flat" not in calls, calls
    E.assert_exact(y, _relu(P.y), "stem16 fprop + relu")
    E.assert_exact(y16, P.y, "stem16 fprop, 16-bit out")


@LP
@pytest.mark.parametrize("case", E.STEM16_3X3)
def test_exact_conv_stem16_3x3_form(case, lp, dev, monkeypatch):
    """VGG conv1_1 (3 -> 64, 3x3, zero padding) on conv_stem16_kernel with a 3-row filter"""
    from mmhand_amd import ops
    B, H, W, Cin = case
    P = E.case_problem("stem16_3x3", case)
    x, w, bias, _ = _dev(P, dev)
    ops.bump_weights_epoch()
    mk = lambda: ops.conv_desc(B, H, W, Cin, 64, 3, 1, 1, False)     # noqa: E731
    calls = _spy(monkeypatch)
    y = ops.raw_conv_lp16_flat(mk(), x, w, bias, 1, lp)
    y16 = ops.raw_conv_lp16_flat(mk(), x, w, bias, 0, lp, out16=True)
    assert calls["mmh_conv_stem16"] == 2 and "mmh_conv_lp16_flat" not in calls, calls
    E.assert_exact(y, _relu(P.y), "3x3 stem form + relu")
    E.assert_exact(y16, P.y, "3x3 stem form, 16-bit out")


@LP
@pytest.mark.parametrize("case", E.WGRAD3X3)
def test_exact_wgrad3x3_lp16(case, lp, dev):
    """wgrad_lp16t_kernel: all nine taps resident, ragged 4 x 16 pixel blocks, images smaller than a block; accumulating"""
    from mmhand_amd import lib, ops
    B, H, W, Cin, Cout, refl = case
    assert lib.load().mmh_set_option(b"lp16_wgrad_ring", 2) == 0
    P = E.case_problem("wgrad3x3", case)
    x, _, _, dy = _dev(P, dev)
    x16, dy16 = _twins(ops, lp, x, dy)
    E.assert_exact(ops.raw_wgrad3x3_lp16(x16, dy16, refl, lp), P.dw, "nine-tap wgrad")
    acc = E.ints((3, 3, Cin, Cout), 12, lo=-8, hi=8)
    E.assert_exact(ops.raw_wgrad3x3_lp16(x16, dy16, refl, lp, out=acc.to(dev)), P.dw + acc.double(), "nine-tap wgrad, accumulating")


@LP
@pytest.mark.parametrize("case", E.WGRAD_S2_9TAP)
def test_exact_stride2_wgrad_on_the_nine_tap_kernel(case, lp, dev):
    """wgrad_lp16t_kernel<., 2> and, with lp16_wgrad_s2 off, the flat-row kernel it replaced"""
    from mmhand_amd import lib, ops
    B, H, W, Cin, Cout = case
    P = E.case_problem("wgrad_s2_9tap", case)
    x, _, _, dy = _dev(P, dev)
    mk = lambda: ops.conv_desc(B, H, W, Cin, Cout, 3, 2, 1, False)     # noqa: E731
    x16, dy16 = _twins(ops, lp, x, dy)
    E.assert_exact(ops.raw_wgrad_lp16_flat(mk(), x16, Cin, dy16, lp), P.dw, "stride-2 nine-tap wgrad")
    lib.check(lib.load().mmh_set_option(b"lp16_wgrad_s2", 0), "mmh_set_option")
    try:
        flat = ops.raw_wgrad_lp16_flat(mk(), x16, Cin, dy16, lp)
    finally:
        lib.check(lib.load().mmh_set_option(b"lp16_wgrad_s2", 1), "mmh_set_option")
    E.assert_exact(flat, P.dw, "stride-2 flat-row wgrad")


@LP
@pytest.mark.parametrize("case", E.WGRAD_FLAT)
def test_exact_wgrad_lp16_flat(case, lp, dev):
    from mmhand_amd import ops
    B, H, W, Cin, Cout, k, stride, refl = case
    P = E.case_problem("wgrad_flat", case)
    x, _, _, dy = _dev(P, dev)
    mk = lambda: ops.conv_desc(B, H, W, Cin, Cout, k, stride, k // 2, refl)     # noqa: E731
    c8 = (Cin + 7) // 8 * 8
    assert ops.lp16_flat_wgrad_ok(mk(), c8, lp, any_cin=True)
    x16p, dy16 = ops.lp16_pad8(x, lp), _twins(ops, lp, dy)
    E.assert_exact(ops.raw_wgrad_lp16_flat(mk(), x16p, c8, dy16, lp), P.dw, "flat-row wgrad")
    E.assert_exact(ops.raw_conv_wgrad_lp16_gen1(x16p, dy16, Cin, k, stride, k // 2, refl, lp), P.dw, "first-generation 16-bit wgrad")


@LP
@pytest.mark.parametrize("case", E.WGRAD_STEM16)
def test_exact_wgrad_stem_lp16(case, lp, dev):
    """wgrad_stem.hip at 44 -> 48 channels (the two work-group kinds), ragged 4 x 16 pixel blocks"""
    from mmhand_amd import ops
    B, H, W, Cin, refl = case
    P = E.case_problem("wgrad_stem16", case)
    x, _, _, dy = _dev(P, dev)
    x16p, dy16 = ops.lp16_pad8(x, lp), _twins(ops, lp, dy)
    d = ops.conv_desc(B, H, W, Cin, 64, 7, 1, 3, refl)
    assert ops.stem_wgrad16_ok(d, x16p.shape[3], lp)
    E.assert_exact(ops.raw_wgrad_stem_lp16(d, x16p, dy16, lp), P.dw, "stem wgrad")


@LP
@pytest.mark.parametrize("case", E.HEAD_WGRAD)
def test_exact_head_wgrad_on_the_stem_wgrad_kernel(case, lp, dev, monkeypatch):
    from mmhand_amd import ops
    B, H, W = case
    P = E.case_problem("head_wgrad", case)
    x, _, _, dy = _dev(P, dev)
    x16 = _twins(ops, lp, x)
    calls = _spy(monkeypatch)
    dw = ops.raw_head_wgrad16(x16, dy, lp)
    assert dict(calls) == {"mmh_conv7_head_wgrad_lp16": 1}, calls
    E.assert_exact(dw, P.dw, "head wgrad")


@LP
@pytest.mark.parametrize("out16", [False, True], ids=["dx32", "dx16"])
@pytest.mark.parametrize("case", E.HEAD_DGRAD)
def test_exact_head_dgrad_on_the_stem_kernel(case, out16, lp, dev, monkeypatch):
    """the padded-domain gradient is stored in 16 bits before the ring is folded back: exact here, every value being an
    integer below the 16-bit cap"""
    from mmhand_amd import ops
    B, H, W = case
    P = E.case_problem("head_dgrad", case)
    _, w, _, dy = _dev(P, dev)
    ops.bump_weights_epoch()
    calls = _spy(monkeypatch)
    dx = ops.raw_conv_dgrad(dy, w, (B, H, W, 64), 1, 3, True, bf16=lp, out16=out16)
    assert dict(calls) == {"mmh_conv7_head_dgrad_lp16": 1}, calls
    assert dx.dtype == (ops._wd(lp) if out16 else torch.float32)
    E.assert_exact(dx, P.dx, "head dgrad")


@LP
@pytest.mark.parametrize("case", E.N4_HEAD)
def test_exact_conv7_n4_head_fprop(case, lp, dev, monkeypatch):
    from mmhand_amd import ops
    B, H, W, refl = case
    P = E.case_problem("n4_head", case)
    x, w, bias, _ = _dev(P, dev)
    calls = _spy(monkeypatch)
    y = ops.raw_conv_fprop(x, w, bias, 1, 3, refl, 0, bf16=lp)
    yr = ops.raw_conv_fprop(x, w, bias, 1, 3, refl, 1, bf16=lp)
    assert calls["mmh_conv7_n4_lp16"] == 2 and "mmh_conv7_thin_fprop" not in calls, calls
    E.assert_exact(y, P.y, "four-column head fprop")
    E.assert_exact(yr, _relu(P.y), "four-column head fprop + relu")


@LP
@pytest.mark.parametrize("case", E.N4_STEM_DGRAD)
def test_exact_conv7_n4_stem_dgrad(case, lp, dev, monkeypatch):
    from mmhand_amd import ops
    B, H, W, Cin, refl = case
    P = E.case_problem("n4_stem_dgrad", case)
    _, w, _, dy = _dev(P, dev)
    dy16 = _twins(ops, lp, dy)
    calls = _spy(monkeypatch)
    dx = ops.raw_conv_dgrad_thin(dy16, w, (B, H, W, Cin), refl)
    assert calls["mmh_conv7_n4_lp16"] == 1 and "mmh_conv7_thin_dgrad" not in calls, calls
    E.assert_exact(dx[..., :4], P.dx[..., :4].contiguous(), "stem gradient towards channels [0, 4)")
    assert not dx[..., 4:].any()


@LP
@pytest.mark.parametrize("case", E.N4_VGG_DGRAD)
def test_exact_conv7_n4_vgg_conv1_dgrad(case, lp, dev, monkeypatch):
    from mmhand_amd import ops
    B, H, W = case
    P = E.case_problem("n4_vgg_dgrad", case)
    _, w, _, dy = _dev(P, dev)
    calls = _spy(monkeypatch)
    dx = ops.raw_conv_dgrad(dy, w, (B, H, W, 4), 1, 1, False, bf16=lp)
    assert calls["mmh_conv7_n4_lp16"] == 1 and "mmh_conv2d_dgrad_folded" not in calls, calls
    E.assert_exact(dx, P.dx, "VGG conv1_1 image gradient")


# ============================================================================================ fp32 Winograd: rounds to the oracle
@pytest.mark.parametrize("case", E.WINO6)
def test_rounds_winograd_f6x6(case, dev, monkeypatch):
    """all three passes through F(6x6,3x3) (forced): ragged tiles, the reflect-fold dgrad and the border-GEMM path"""
    from mmhand_amd import ops
    B, H, W, Cin, Cout, refl = case
    monkeypatch.setattr(ops, "WINOGRAD_TILE", 6)
    monkeypatch.setattr(ops, "WINO6_MIN", 0)
    assert ops._wino_tile(B, H, W, Cin, Cout, 3, 1, 1, False) == 6
    P = E.case_problem("wino6", case)
    x, w, bias, dy = _dev(P, dev)
    ops.bump_weights_epoch()
    y = ops.raw_conv_fprop(x, w, bias, 1, 1, refl, 1)
    dx = ops.raw_conv_dgrad(dy, w, x.shape, 1, 1, refl)
    dw = ops.raw_conv_wgrad(x, dy, 3, 1, 1, refl)
    E.assert_rounds(y, _relu(P.y), f"F(6x6) fprop + relu {case}")
    E.assert_rounds(dx, P.dx, f"F(6x6) dgrad {case} fold={refl and ops._fold_ok(H, W)}")
    E.assert_rounds(dw, P.dw, f"F(6x6) wgrad {case}")


@pytest.mark.parametrize("case", E.WINO6_FUSED)
def test_rounds_winograd_f6x6_fused_backward(case, dev, monkeypatch):
    from mmhand_amd import ops
    B, H, W, Cin, Cout, refl = case
    monkeypatch.setattr(ops, "WINOGRAD_TILE", 6)
    monkeypatch.setattr(ops, "WINO6_MIN", 0)
    monkeypatch.setattr(ops, "FUSE_WINO6_BWD", True)
    P = E.case_problem("wino6", case)
    x, w, _, dy = _dev(P, dev)
    ops.bump_weights_epoch()
    x.requires_grad_(True); w.requires_grad_(True)
    calls = _spy(monkeypatch)
    y = ops.Conv2dFn.apply(x, w, None, 1, 1, refl, 0)
    y.backward(dy)
    assert calls["mmh_wino_input_dy"] == 1, calls
    E.assert_rounds(x.grad, P.dx, f"fused F(6x6) backward, dx {case}")
    E.assert_rounds(w.grad, P.dw, f"fused F(6x6) backward, dw {case}")


@pytest.mark.parametrize("tile", [2, 4])
@pytest.mark.parametrize("case", E.WINO24)
def test_rounds_winograd_f2_f4(case, tile, dev):
    from mmhand_amd import ops
    B, H, W, Cin, Cout, refl = case
    P = E.case_problem("wino24", case)
    x, w, bias, dy = _dev(P, dev)
    ops.bump_weights_epoch()
    E.assert_rounds(ops.raw_conv_fprop_wino(x, w, bias, refl, 1, tile), _relu(P.y), f"F({tile}x{tile}) fprop + relu {case}")
    E.assert_rounds(ops.raw_conv_dgrad_wino(dy, w, x.shape, refl, tile), P.dx, f"F({tile}x{tile}) dgrad {case}")
    E.assert_rounds(ops.raw_conv_wgrad_wino(x, dy, refl, tile), P.dw, f"F({tile}x{tile}) wgrad {case}")


@pytest.mark.parametrize("case", E.WINO2_FWD)
def test_rounds_two_level_f2x2_forward(case, dev, monkeypatch):
    """mode bwd_f2 (mmh_wino_gemm_levels16), its speed threshold lowered as tests/test_wino2_fwd_gpu.py does"""
    from mmhand_amd import ops
    B, H, W, Cin, Cout, refl = case
    P = E.case_problem("wino2_fwd", case)
    x, w, bias, _ = _dev(P, dev)
    ops.set_winograd_mode("bwd_f2")
    try:
        monkeypatch.setattr(ops, "WINO2_FWD_MIN", 0)
        calls = _spy(monkeypatch)
        y = ops.raw_conv_fprop(x, w, bias, 1, 1, refl, 1)
        assert calls["mmh_wino_gemm_levels16"] == 1 and calls["mmh_conv2d_fprop"] == 0, calls
    finally:
        ops.set_winograd_mode("all")
    E.assert_rounds(y, _relu(P.y), f"two-level F(2x2) forward {case}")


def test_exact_wino_wgrad_dma_gemm(dev):
    """wino_wgrad_dma.hip at the stage level (the shape tests/test_wino_gemm_gpu.py reaches it with): dU[p] = V[p]^T Yh[p] is a
    plain GEMM, so on integers it is exact - held to `equal`, which implies the rounding check.  (At the conv level the
    F(2x2) wgrad of (1, 12, 20, 256, 256) above runs on it too: 60 tiles, 256 x 256 channels.)"""
    from mmhand_amd import lib
    P_, T, Cin, Cout = E.WINO_WGRAD_DMA
    assert Cin % 256 == 0 and Cout % 256 == 0 and T >= 32          # the kernel's own conditions (wino_wgrad_dma_ok)
    V, Y = E.ints((P_, T, Cin), 21), E.ints((P_, T, Cout), 22)
    want = torch.bmm(V.double().transpose(1, 2), Y.double())
    Vd, Yd = V.to(dev), Y.to(dev)
    L_ = lib.load()
    outs = {}
    for dma in (1, 0):
        lib.check(L_.mmh_set_option(b"wino_wgrad_dma", dma), "mmh_set_option")
        try:
            nws = L_.mmh_wino_wgrad_gemm_ws_bytes(T, Cin, Cout, P_)
            ws = torch.full((nws // 4 + 4,), float("nan"), device=dev)
            dU = torch.full((P_, Cin, Cout), 7.0, device=dev)
            lib.call("mmh_wino_wgrad_gemm", Vd.data_ptr(), Yd.data_ptr(), T, Cin, Cout, P_, lib.F32, ws.data_ptr(), nws,
                     dU.data_ptr(), torch.cuda.current_stream().cuda_stream)
            outs[dma] = dU
        finally:
            lib.check(L_.mmh_set_option(b"wino_wgrad_dma", 1), "mmh_set_option")
    E.assert_exact(outs[1], want, "Winograd-domain wgrad GEMM, DMA ring")
    E.assert_exact(outs[0], want, "Winograd-domain wgrad GEMM, persistent TN kernel")
