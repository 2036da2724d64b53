"""Bit-exact rounding tests for the 16-bit stores of the convolution kernels (the round-once problems of tests/_exact.py).

The capped families of tests/test_conv_exact_gpu.py test the sums: nothing there rounds.  Here the exact fp32 sum does not fit
the 16-bit type, and the one correct stored value is RNE(exact sum + bias, after the activation) - compared bit for bit,
element by element (E.assert_rounded_once); zeros with their sign, NaN by NaN-ness.  No tolerance anywhere.  One parametrised
test per 16-bit store site, through the wrapper and with the "the intended kernel ran" check of its exact test.

Epilogue families (one distinct store helper or hand-written epilogue each), the kernels that use them, roundings found:
  A  pair_swap8 + bias + act_apply + store8_lp16 (device_prims.h), 16-byte stores: the halo kernel conv_lp16h2_kernel
     (conv_lp16_halo.hip; mmh_conv3x3_lp16 modes 0, 1 and 2 - the in-kernel fold adds its border terms to the fp32
     accumulators first - and its statistics form) and conv_lp16g_body (conv_lp16.hip; mmh_conv_lp16: stride-2 fprop, its
     four-class dgrad = ConvTranspose2d fprop, 64-column stride-1 convs).  One rounding.
  B  store4 (device_prims.h; bias, act_apply, one 8-byte store): conv_stem16_kernel (conv_stem16.hip; mmh_conv_stem16, 7x7 and
     3x3 forms), conv_lp16f_kernel (conv_lp16.hip; mmh_conv_lp16_flat), conv_s2f_kernel and the stride-2 dgrad kernel of
     conv_s2_lp16.hip (behind mmh_conv_lp16: 64 -> 128 stride 2, 64 -> 64 stride 1), the halo kernel with lp16_dbg = 128.
     One rounding.
  C  the scalar store of conv_lp16p_kernel (conv_lp16.hip: the row-tile kernel, images below 16 x 16 and lp16_shape 17, with
     and without lp16_tap_inner).  One rounding.
  D  border_add_kernel<LP> (conv_igemm.hip; mmh_conv2d_dgrad_border behind the mode-1 dgrad of a reflect-padded conv): reads
     the 16-bit dx that A or C stored, adds the border terms, stores again.  TWO roundings at the ring pixels, by design
     (E.border_sequence).
  E  head_dgrad_fold_kernel (conv_stem16.hip; mmh_conv7_head_dgrad_lp16): sums up to nine 16-bit values of the padded-domain
     gradient that B stored.  dx fp32: one rounding per TERM; dx 16-bit: one more of the sum (E.head_dgrad_sequence).
Edges per family: the scaled problem (fp16: results on the subnormal grid below 2^-14; bf16: results around 2^120), fp16
overflow (steered elements of one row either side of 65520: E.overflow_problem) and a NaN and an inf in one operand, the NaN
in the last pixel (E.special_problem); all three through exactly the launches of the main problem.
The fp32 -> 16-bit conversion kernels run a fixed corner table (E.corner_table); the in-kernel conversions of fp32 operands
(head wgrad's dy, the w of mmh_conv7_n4_lp16 and of the head dgrad) run operands that are ties of the 16-bit type.
Not covered: the norm-backward-sums form of the halo dgrad (mmh_conv3x3_lp16_dgrad_nbr: family A's store with no bias)."""
import ctypes
from collections import Counter

import pytest
import torch

from tests import _exact as E

pytestmark = pytest.mark.gpu

NAME = {True: "bf16", 2: "fp16"}
LP = pytest.mark.parametrize("lp", [True, 2], ids=["bf16", "fp16"])


@pytest.fixture(scope="module", autouse=True)
def _give_memory_back():
    """this module frees blocks that hold NaN, inf and values near 2^120 on purpose; when it ends they go back to the driver
    (as tests/test_inception_gpu.py and tests/test_fid_gpu.py do), so that the modules after it start from the allocator they
    would have found without this one.  (a read of never-written memory in the --graph_step / wino2 batch-norm path
    is known and not located; tests/test_wino2_coherence_gpu.py::test_graph_replay_then_test[batch] finds it when such
    blocks are handed to it.)"""
    yield
    import gc
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _params(fam, overflow=None):
    """(case, edge, lp) of one family: every case as the main problem, its first case scaled and with a NaN / inf, in both
    types; the steered fp16 overflow problem of family `overflow` (default: the family itself)"""
    cases = E.ROUND_FAMILIES[fam][0]
    out = []
    for lp in (True, 2):
        out += [pytest.param(c, None, lp, id=f"{'x'.join(map(str, c))}-main-{NAME[lp]}") for c in cases]
        if "persist" not in fam:
            out += [pytest.param(cases[0], edge, lp, id=f"{'x'.join(map(str, cases[0]))}-{edge}-{NAME[lp]}") for edge in ("scaled", "special")]
    ofam = overflow or fam
    if ofam in E.OVERFLOW_CASES:
        c = E.OVERFLOW_CASES[ofam]
        out.append(pytest.param(c, "overflow:" + ofam, 2, id=f"{'x'.join(map(str, c))}-overflow-fp16"))
    return out


def _problem(fam, case, edge, lp):
    if edge and edge.startswith("overflow"):
        return E.overflow_problem(edge.split(":")[1], case)
    if edge == "special":
        return E.special_problem(fam, case, NAME[lp])
    return E.round_problem(fam, case, NAME[lp], edge)


def _spy(monkeypatch):
    from mmhand_amd import lib
    calls = Counter()
    real = lib.call

    def spy(name, *a):
        calls[name] += 1
        return real(name, *a)
    monkeypatch.setattr(lib, "call", spy)
    return calls


def _relu(t):
    return t.clamp_min(0.0)


def _twin(ops, P, t, lp, dev):
    """the 16-bit copy of an operand (mmh_cvt_lp16), which the problem guarantees to be exact"""
    t16 = ops.lp16_twin(t.to(dev), lp)
    E.assert_bits16(t16, t.to(P.td), "16-bit twin of an operand")
    return t16


def _nobias(P):
    return P.y - P.bias.double()            # exact: both are fp32 values and so is the sum without the bias


# ============================================================================================ mmh_conv3x3_lp16, fprop
@pytest.mark.parametrize("shape", [17, 19], ids=["rowtile", "halo"])
@pytest.mark.parametrize("case,edge,lp", _params("halo_fprop"))
def test_round_conv3x3_lp16_fprop(case, edge, lp, shape, dev, monkeypatch):
    """families C (row tiles: lp16_shape 17, and every image below 16 x 16) and A (the halo kernel at 16 x 16): plain, ReLU,
    with and without bias; where the shape has it, the statistics form of the same store.  One rounding."""
    from mmhand_amd import lib, ops
    B, H, W, Cin, Cout, refl = case
    P = _problem("halo_fprop", case, edge, lp)
    w, bias = P.w.to(dev), P.bias.to(dev)
    d = ops.conv_desc(B, H, W, Cin, Cout, 3, 1, 1, refl)
    d.dtype = ops._dt(lp)
    assert lib.load().mmh_conv3x3_lp16_supported(ctypes.byref(d)) == 1
    with E.option("lp16_shape", shape):
        ops.bump_weights_epoch()
        x16 = _twin(ops, P, P.x, lp, dev)
        calls = _spy(monkeypatch)
        y = ops.raw_conv3x3_lp16(x16, w, bias, refl, 0, lp, 0, out16=True)
        yr = ops.raw_conv3x3_lp16(x16, w, bias, refl, 1, lp, 0, out16=True)
        y0 = ops.raw_conv3x3_lp16(x16, w, None, refl, 0, lp, 0, out16=True)
        assert calls["mmh_conv3x3_lp16"] == 3 and "mmh_conv3x3_lp16_fprop_stats" not in calls, calls
        ys = None
        if shape == 19 and lib.load().mmh_conv3x3_lp16_stats_chunks(ctypes.byref(d)) > 0 and ops.FUSE_NORM_STATS:
            ops._pending_stats.clear()
            ys = ops.raw_conv3x3_lp16(x16, w, bias, refl, 0, lp, 0, out16=True, want_stats=True)
            ops._pending_stats.clear()
            assert calls["mmh_conv3x3_lp16_fprop_stats"] == 1, calls
    E.assert_rounded_once(y, P.y, P.td, "fprop + bias")
    E.assert_rounded_once(yr, _relu(P.y), P.td, "fprop + bias + relu")
    E.assert_rounded_once(y0, _nobias(P), P.td, "fprop, no bias")
    if ys is not None:
        E.assert_rounded_once(ys, P.y, P.td, "fprop + bias, statistics form")


@LP
@pytest.mark.parametrize("case", E.HALO_FPROP)
def test_round_conv3x3_lp16_row_tiles_tap_inner(case, lp, dev):
    """family C with lp16_tap_inner = 1 (the k loop walks the nine taps inside a 64-channel chunk)"""
    from mmhand_amd import ops
    B, H, W, Cin, Cout, refl = case
    P = E.round_problem("halo_fprop", case, NAME[lp])
    with E.options(lp16_shape=17, lp16_tap_inner=1):
        ops.bump_weights_epoch()
        x16 = _twin(ops, P, P.x, lp, dev)
        yr = ops.raw_conv3x3_lp16(x16, P.w.to(dev), P.bias.to(dev), refl, 1, lp, 0, out16=True)
    E.assert_rounded_once(yr, _relu(P.y), P.td, "fprop + bias + relu, tap-inner")


@LP
def test_round_conv3x3_lp16_halo_8_byte_stores(lp, dev):
    """family B inside the halo kernel: lp16_dbg = 128 stores through store4 instead of the lane-pair trade"""
    from mmhand_amd import ops
    case = E.HALO_FPROP[2]
    B, H, W, Cin, Cout, refl = case
    P = E.round_problem("halo_fprop", case, NAME[lp])
    ops.bump_weights_epoch()
    x16 = _twin(ops, P, P.x, lp, dev)
    with E.option("lp16_dbg", 128):
        yr = ops.raw_conv3x3_lp16(x16, P.w.to(dev), P.bias.to(dev), refl, 1, lp, 0, out16=True)
    E.assert_rounded_once(yr, _relu(P.y), P.td, "fprop + bias + relu, 8-byte stores")


def _halo_tiles(B, H, W, N):
    return B * -(-H // E.HALO_TILE) * -(-W // E.HALO_TILE) * (N // E.HALO_TBN)


def _persistent_grid(dev):
    return 8 * (torch.cuda.get_device_properties(dev).multi_processor_count // 8)


@LP
def test_round_conv3x3_lp16_halo_second_tile_fprop(lp, dev):
    """family A in the persistent loop: 288 ragged tiles for 256 workgroups, the second tile's store"""
    from mmhand_amd import ops
    case = E.HALO_PERSIST_FPROP[0]
    B, H, W, Cin, Cout, refl = case
    assert _halo_tiles(B, H, W, Cout) > _persistent_grid(dev)
    P = E.round_problem("halo_persist_fprop", case, NAME[lp])
    ops.bump_weights_epoch()
    x16 = _twin(ops, P, P.x, lp, dev)
    yr = ops.raw_conv3x3_lp16(x16, P.w.to(dev), P.bias.to(dev), refl, 1, lp, 0, out16=True)
    E.assert_rounded_once(yr, _relu(P.y), P.td, "fprop + bias + relu, persistent")


# ============================================================================================ mmh_conv3x3_lp16, dgrad
def _border_params():
    """every problem of the family on the default border tiles; the main problems again with border_bn64 = 0"""
    ps = _params("fold_dgrad")
    return ([pytest.param(*p.values, False, id=p.id + "-bn64") for p in ps] +
            [pytest.param(*p.values, True, id=p.id + "-wide") for p in ps if p.values[1] is None])


@pytest.mark.parametrize("case,edge,lp,wide", _border_params())
def test_round_conv3x3_lp16_reflect_dgrad_border(case, edge, lp, wide, dev, monkeypatch):
    """family D behind A (32 x 16: the halo kernel, mode 1) and behind A at 16 x 48.  TWO roundings at the ring pixels, by
    design and in a fixed sequence: conv_lp16h2_kernel (conv_lp16_halo.hip) stores RNE(main term); border_add_kernel
    (conv_igemm.hip) reads it back, adds the fp32 sum of the eight border pieces (exact here in any order) and stores RNE
    again.  The contract of raw_conv_dgrad(out16=True) does not promise the rounding of the fp32 result on this route
    (tests/test_lp16_edges_gpu.py: "border_add works on a 16-bit dx"), so the test holds the kernel to the sequence.
    wide: border_bn64 = 0, the border GEMMs on 128-wide tiles."""
    from mmhand_amd import lib, ops
    B, H, W, Cin, Cout = case
    P = _problem("fold_dgrad", case, edge, lp)
    d = ops.conv_desc(B, H, W, Cin, Cout, 3, 1, 1, True)
    d.dtype = ops._dt(lp)
    assert lib.load().mmh_conv3x3_lp16_fold_supported(ctypes.byref(d)) == 0
    ops.bump_weights_epoch()
    dy16 = _twin(ops, P, P.dy, lp, dev)
    calls = _spy(monkeypatch)
    with E.option("border_bn64", 0 if wide else 1):
        dx = ops.raw_conv_dgrad(None, P.w.to(dev), (B, H, W, Cin), 1, 1, True, bf16=lp, dy16=dy16, out16=True)
    assert calls["mmh_conv3x3_lp16"] == 1 and calls["mmh_conv2d_dgrad_border"] == 1, calls
    want, share = E.border_sequence(P, P.td)
    print(f"\n[two roundings] {case} {NAME[lp]} {edge}: {share:.4f} of the elements differ from RNE(dx)")
    E.assert_bits16(dx, want, "reflect dgrad: RNE(RNE(main) + border)", P.dx)


@pytest.mark.parametrize("case,edge,lp", _params("fold_in_kernel"))
def test_round_conv3x3_lp16_in_kernel_fold(case, edge, lp, dev, monkeypatch):
    """family A, mode 2: ring rows, columns and corners are added to the fp32 accumulators inside the halo kernel - one rounding"""
    from mmhand_amd import lib, ops
    B, H, W, Cin, Cout = case
    P = _problem("fold_in_kernel", case, edge, lp)
    d = ops.conv_desc(B, H, W, Cin, Cout, 3, 1, 1, True)
    d.dtype = ops._dt(lp)
    assert lib.load().mmh_conv3x3_lp16_fold_supported(ctypes.byref(d)) == 1
    ops.bump_weights_epoch()
    dy16 = _twin(ops, P, P.dy, lp, dev)
    calls = _spy(monkeypatch)
    dx = ops.raw_conv_dgrad(None, P.w.to(dev), (B, H, W, Cin), 1, 1, True, bf16=lp, dy16=dy16, out16=True)
    assert calls["mmh_conv3x3_lp16"] == 1 and "mmh_conv2d_dgrad_border" not in calls, calls
    E.assert_rounded_once(dx, P.dx, P.td, "in-kernel fold")


@LP
def test_round_conv3x3_lp16_halo_second_tile_dgrad(lp, dev, monkeypatch):
    """family A, mode 2, 288 tiles for 256 workgroups"""
    from mmhand_amd import ops
    case = E.HALO_PERSIST_DGRAD[0]
    B, H, W, Cin, Cout = case
    assert _halo_tiles(B, H, W, Cin) > _persistent_grid(dev)
    P = E.round_problem("halo_persist_dgrad", case, NAME[lp])
    ops.bump_weights_epoch()
    dy16 = _twin(ops, P, P.dy, lp, dev)
    calls = _spy(monkeypatch)
    dx = ops.raw_conv_dgrad(None, P.w.to(dev), (B, H, W, Cin), 1, 1, True, bf16=lp, dy16=dy16, out16=True)
    assert calls["mmh_conv3x3_lp16"] == 1 and "mmh_conv2d_dgrad_border" not in calls, calls
    E.assert_rounded_once(dx, P.dx, P.td, "in-kernel fold, persistent")


# ============================================================================================ mmh_conv_lp16
def _lp16g_both(ops, P, mk, lp, dev, what, fprop_options=None):
    """fprop (bias; bias + ReLU) and, for a zero-padded conv, dgrad of conv mk() on mmh_conv_lp16, all with 16-bit output"""
    w, bias = P.w.to(dev), P.bias.to(dev)
    ops.bump_weights_epoch()
    assert ops.lp16g_ok(mk(), 0, lp)
    x16 = _twin(ops, P, P.x, lp, dev)
    with E.options(**(fprop_options or {})):
        y = ops.raw_conv_lp16g(mk(), 0, x16, w, bias, 0, lp, out16=True)
        yr = ops.raw_conv_lp16g(mk(), 0, x16, w, bias, 1, lp, out16=True)
    E.assert_rounded_once(y, P.y, P.td, what + " fprop + bias")
    E.assert_rounded_once(yr, _relu(P.y), P.td, what + " fprop + bias + relu")
    if "dx" in P.spec[-1]:
        assert ops.lp16g_ok(mk(), 1, lp)
        dy16 = _twin(ops, P, P.dy, lp, dev)
        dx = ops.raw_conv_lp16g(mk(), 1, dy16, w, None, 0, lp, out16=True)
        E.assert_rounded_once(dx, P.dx, P.td, what + " dgrad")


def _s2f_chunks(ops, lib, d, lp):
    d.dtype = ops._dt(lp)
    return lib.load().mmh_conv_lp16_stats_chunks(ctypes.byref(d))      # > 0: conv_s2f_kernel takes the fprop of d


@pytest.mark.parametrize("case,edge,lp", _params("lp16g"))
def test_round_conv_lp16g(case, edge, lp, dev):
    """family A in conv_lp16g_body: the stride-2 fprop and the four parity classes of its dgrad (shapes conv_s2_lp16.hip leaves
    to it)"""
    from mmhand_amd import lib, ops
    B, H, W, Cin, Cout, stride, refl = case
    P = _problem("lp16g", case, edge, lp)
    mk = lambda: ops.conv_desc(B, H, W, Cin, Cout, 3, stride, 1, refl)     # noqa: E731
    assert _s2f_chunks(ops, lib, mk(), lp) == 0
    _lp16g_both(ops, P, mk, lp, dev, "lp16g")


@pytest.mark.parametrize("case,edge,lp", _params("s2_lp16"))
def test_round_conv_s2_lp16(case, edge, lp, dev):
    """family B in conv_s2_lp16.hip: conv_s2f_kernel (fprop at 64 and, lp16_s2f = 2, 128 input channels) and the 64 <- 128
    stride-2 dgrad kernel; the 128 <- 256 dgrad stays on conv_lp16g_body (family A)"""
    from mmhand_amd import lib, ops
    B, H, W, Cin, Cout = case
    P = _problem("s2_lp16", case, edge, lp)
    mk = lambda: ops.conv_desc(B, H, W, Cin, Cout, 3, 2, 1, False)     # noqa: E731
    with E.option("lp16_s2f", 2):
        assert _s2f_chunks(ops, lib, mk(), lp) > 0
    _lp16g_both(ops, P, mk, lp, dev, "s2_lp16", fprop_options=dict(lp16_s2f=2))


@pytest.mark.parametrize("case,edge,lp", _params("s1_lp16"))
def test_round_conv_s2_lp16_stride1_64_to_64(case, edge, lp, dev):
    """family B: the stride-1 form of conv_s2f_kernel (8 x 16 and 24 x 48) and its input gradient; 40 x 40 is off the tile and
    stays on conv_lp16g_body (family A)"""
    from mmhand_amd import ops
    B, H, W = case
    P = _problem("s1_lp16", case, edge, lp)
    mk = lambda: ops.conv_desc(B, H, W, 64, 64, 3, 1, 1, False)     # noqa: E731
    _lp16g_both(ops, P, mk, lp, dev, "s1_lp16")


@pytest.mark.parametrize("case,edge,lp", _params("convT"))
def test_round_convT_fprop_and_dgrad(case, edge, lp, dev, monkeypatch):
    """raw_convT_fprop (mode 1 of the stride-2 conv it is the adjoint of, WITH bias and activation) and raw_convT_dgrad (mode 0),
    16-bit outputs: family A"""
    from mmhand_amd import ops
    B, h, w_, CinT, CoutT = case
    P = _problem("convT", case, edge, lp)
    w, bias = P.w.to(dev), P.bias.to(dev)
    assert ops.convT_lp16_ok(CinT, CoutT, lp)
    ops.bump_weights_epoch()
    x16, dy16 = _twin(ops, P, P.x, lp, dev), _twin(ops, P, P.dy, lp, dev)
    calls = _spy(monkeypatch)
    y = ops.raw_convT_fprop(x16, w, bias, 0, bf16=lp, out16=True)
    yr = ops.raw_convT_fprop(x16, w, bias, 1, bf16=lp, out16=True)
    dx = ops.raw_convT_dgrad(dy16, w, (B, h, w_, CinT), bf16=lp, out16=True)
    assert calls["mmh_conv_lp16"] == 3 and "mmh_convT2d_fprop" not in calls and "mmh_convT2d_dgrad" not in calls, calls
    assert tuple(y.shape) == (B, 2 * h, 2 * w_, CoutT)
    E.assert_rounded_once(y, P.y, P.td, "convT fprop + bias")
    E.assert_rounded_once(yr, _relu(P.y), P.td, "convT fprop + bias + relu")
    E.assert_rounded_once(dx, P.dx, P.td, "convT dgrad")


# ============================================================================================ the stems
def _stem_fprop(ops, P, mk, lp, dev, what):
    x, w, bias = P.x.to(dev), P.w.to(dev), P.bias.to(dev)
    ops.bump_weights_epoch()
    y = ops.raw_conv_lp16_flat(mk(), x, w, bias, 0, lp, out16=True)
    yr = ops.raw_conv_lp16_flat(mk(), x, w, bias, 1, lp, out16=True)
    y0 = ops.raw_conv_lp16_flat(mk(), x, w, None, 0, lp, out16=True)
    E.assert_rounded_once(y, P.y, P.td, what + " + bias")
    E.assert_rounded_once(yr, _relu(P.y), P.td, what + " + bias + relu")
    E.assert_rounded_once(y0, _nobias(P), P.td, what + ", no bias")


@pytest.mark.parametrize("case,edge,lp", _params("flat_stems"))
def test_round_conv_lp16_flat_stems(case, edge, lp, dev, monkeypatch):
    """family B in conv_lp16f_kernel (the stem kernel that replaced it off); x goes through mmh_lp16_pad_cvt"""
    from mmhand_amd import ops
    B, H, W, Cin, Cout, k, refl = case
    monkeypatch.setattr(ops, "USE_STEM_FPROP16", False)
    monkeypatch.setattr(ops, "USE_PACK_TWIN", False)
    P = _problem("flat_stems", case, edge, lp)
    mk = lambda: ops.conv_desc(B, H, W, Cin, Cout, k, 1, k // 2, refl)     # noqa: E731
    assert ops.lp16_flat_ok(mk(), lp)
    calls = _spy(monkeypatch)
    _stem_fprop(ops, P, mk, lp, dev, "flat-K fprop")
    assert calls["mmh_conv_lp16_flat"] == 3 and "mmh_conv_stem16" not in calls, calls


@pytest.mark.parametrize("case,edge,lp", _params("stem16"))
def test_round_conv_stem16(case, edge, lp, dev, monkeypatch):
    """family B in conv_stem16_kernel, y_is16"""
    from mmhand_amd import ops
    B, H, W, Cin, refl = case
    monkeypatch.setattr(ops, "USE_PACK_TWIN", False)
    P = _problem("stem16", case, edge, lp)
    mk = lambda: ops.conv_desc(B, H, W, Cin, 64, 7, 1, 3, refl)     # noqa: E731
    calls = _spy(monkeypatch)
    _stem_fprop(ops, P, mk, lp, dev, "stem16 fprop")
    assert calls["mmh_conv_stem16"] == 3 and "mmh_conv_lp16_flat" not in calls, calls


@pytest.mark.parametrize("case,edge,lp", _params("stem16_3x3", overflow="none"))
def test_round_conv_stem16_3x3_form(case, edge, lp, dev, monkeypatch):
    """family B in conv_stem16_kernel with a 3-row filter (VGG conv1_1, 3 -> 64).  27 products of |x| <= 2048 cannot reach the
    fp16 threshold: the overflow edge of this epilogue is the 7x7 form's"""
    from mmhand_amd import ops
    B, H, W, Cin = case
    monkeypatch.setattr(ops, "USE_PACK_TWIN", False)
    P = _problem("stem16_3x3", case, edge, lp)
    mk = lambda: ops.conv_desc(B, H, W, Cin, 64, 3, 1, 1, False)     # noqa: E731
    calls = _spy(monkeypatch)
    _stem_fprop(ops, P, mk, lp, dev, "3x3 stem form")
    assert calls["mmh_conv_stem16"] == 3 and "mmh_conv_lp16_flat" not in calls, calls


# ============================================================================================ the head dgrad
def _head_dgrad(ops, P, case, lp, dev, monkeypatch, what):
    B, H, W = case
    ops.bump_weights_epoch()
    calls = _spy(monkeypatch)
    got = {o: ops.raw_conv_dgrad(P.dy.to(dev), P.w.to(dev), (B, H, W, 64), 1, 3, True, bf16=lp, out16=o) for o in (False, True)}
    assert dict(calls) == {"mmh_conv7_head_dgrad_lp16": 2}, calls
    assert got[True].dtype == P.td and got[False].dtype == torch.float32
    return got


@pytest.mark.parametrize("fam,case,edge,lp", [pytest.param(f, *p.values, id=f + "-" + p.id) for f in ("head_dgrad", "head_dgrad_dense")
                                              for p in _params(f)])
def test_round_head_dgrad(fam, case, edge, lp, dev, monkeypatch):
    """family E behind B.  By design (conv_stem16.hip: "transpose of ReflectionPad2d(3) on a 16-bit padded-domain gradient";
    tests/test_conv_exact_gpu.py says the same of its capped form): conv_stem16_kernel stores every element of the padded-domain
    gradient [B][H + 6][W + 6][64] as RNE (store4); head_dgrad_fold_kernel adds the up to nine of them that fold onto a pixel in
    fp32 - exact here, in any order - and stores fp32 (dx_is16 = 0: as many roundings as terms, none of the sum) or RNE of that
    sum (dx_is16 = 1: one more).  The sequence is deterministic, so both outputs are held to it bit for bit."""
    from mmhand_amd import ops
    P = _problem(fam, case, edge, lp)
    got = _head_dgrad(ops, P, case, lp, dev, monkeypatch, fam)
    want32 = E.head_dgrad_sequence(P, P.td, False)
    g32 = got[False].detach().double().cpu()
    ok = E._same(g32, want32)
    if not bool(ok.all()):
        idx = tuple(int(i) for i in (~ok).nonzero()[0])
        raise AssertionError(f"head dgrad, fp32 dx: {int((~ok).sum())} of {ok.numel()} elements differ from the sum of the rounded terms; "
                             f"first at index {idx}: got {float(g32[idx])!r}, want {float(want32[idx])!r} (exact value {float(P.dx[idx])!r})")
    E.assert_bits16(got[True], E.head_dgrad_sequence(P, P.td, True), "head dgrad, 16-bit dx: RNE(sum of RNE(padded terms))", P.dx)


# ============================================================================================ fp32 -> 16-bit conversions
def _table(td, dev):
    """corner table + its first two entries: whole 8-element vectors, and the LAST element of the buffer is a tie"""
    t = E.corner_table(td)
    buf = torch.cat([t, t[:2]])
    assert buf.numel() % 8 == 0 and E.round_shares(buf[-1:].double(), td)["ties"] == 1.0
    return buf, E.rne16(buf.double(), td), buf.to(dev)


@LP
def test_corner_table_cvt_lp16(lp, dev):
    """mmh_cvt_lp16: whole vectors; the same table behind 8 and 16 leading elements (other lanes, other blocks' tails)"""
    from mmhand_amd import ops
    td = ops._wd(lp)
    buf, want, x = _table(td, dev)
    E.assert_bits16(ops.lp16_twin(x, lp), want, "mmh_cvt_lp16")
    for lead in (8, 2048 + 16):
        xx = torch.cat([torch.ones(lead, device=dev), x])
        E.assert_bits16(ops.lp16_twin(xx, lp)[lead:], want, f"mmh_cvt_lp16 behind {lead} elements")


@LP
@pytest.mark.parametrize("C", [3, 8, 44])
def test_corner_table_lp16_pad_cvt_and_pack(C, lp, dev, monkeypatch):
    """mmh_lp16_pad_cvt (real lanes converted, pad lanes +0) and mmh_pack_nhwc_lp16 of the same values: rows of C channels cut
    from the table, so every entry meets every lane position; the last real lane of the buffer is the table's closing tie"""
    from mmhand_amd import ops
    monkeypatch.setattr(ops, "USE_PACK_TWIN", True)
    td = ops._wd(lp)
    buf, want, _ = _table(td, dev)
    rows = -(-buf.numel() // C)
    flat = torch.cat([buf, buf])[-rows * C:]                      # ends with the closing tie
    Hh, Ww = 1, rows
    x = flat.reshape(1, Hh, Ww, C).to(dev)
    c8 = (C + 7) // 8 * 8
    want16 = torch.zeros(1, Hh, Ww, c8, dtype=td)
    want16[..., :C] = E.rne16(flat.double(), td).reshape(1, Hh, Ww, C)
    got = torch.full((1, Hh, Ww, c8), 7.0, dtype=td, device=dev)
    ops.lp16_pad8(x, lp, out=got)
    E.assert_bits16(got, want16, f"mmh_lp16_pad_cvt C={C}")
    Cd = (C + 3) // 4 * 4
    src = x.permute(0, 3, 1, 2).contiguous()                      # logical NCHW plane source
    only = ops.raw_pack([(src, True, C)], 1, Hh, Ww, Cd, dev, twin=lp, only16=True)
    E.assert_bits16(only, want16, f"mmh_pack_nhwc_lp16 C={C}")


def _table_weights(td, taps, cin, cout):
    t = E.corner_table(td)
    n = taps * cin * cout
    rep = torch.cat([t] * (-(-n // t.numel()) + 1))
    return rep[rep.numel() - n:].reshape(taps, cin, cout).contiguous()          # the last element of the buffer is a table entry too


@LP
@pytest.mark.parametrize("shape", [(9, 64, 64), (1, 128, 192), (9, 24, 64)])
def test_corner_table_prep_weights(shape, lp, dev):
    """mmh_prep_weights_bf16 / _fp16, both layouts, the flat layout of the same entry points (Cin % 64 != 0), and
    mmh_prep_weights_lp16_multi"""
    from mmhand_amd import lib as L, ops
    taps, cin, cout = shape
    td = ops._wd(lp)
    fn = "mmh_prep_weights_" + NAME[lp]
    w = _table_weights(td, taps, cin, cout)
    want = E.rne16(w.double(), td)
    wd = w.to(dev)
    wp = torch.full((taps, cin, cout), 7.0, dtype=td, device=dev)
    if cin % 64 == 0:
        wt = torch.full((taps, cout, cin), 7.0, dtype=td, device=dev)
        L.call(fn, ops._ptr(wd), taps, cin, cout, ops._ptr(wp), ops._ptr(wt), ops._stream())
        E.assert_bits16(wp, want, fn + " plain")
        E.assert_bits16(wt, want.transpose(1, 2).contiguous(), fn + " transposed")
        wp2, wt2 = torch.full_like(wp, 7.0), torch.full_like(wt, 7.0)
        table = torch.tensor([[wd.data_ptr(), wp2.data_ptr(), wt2.data_ptr(), taps, cin, cout, 0, int(lp == 2)]], dtype=torch.int64).to(dev)
        L.call("mmh_prep_weights_lp16_multi", ops._ptr(table), 1, taps * ((cin + 63) // 64) * ((cout + 63) // 64), ops._stream())
        E.assert_bits16(wp2, want, "mmh_prep_weights_lp16_multi plain")
        E.assert_bits16(wt2, want.transpose(1, 2).contiguous(), "mmh_prep_weights_lp16_multi transposed")
    else:
        L.call(fn, ops._ptr(wd), taps, cin, cout, ops._ptr(wp), None, ops._stream())
        E.assert_bits16(wp, want, fn + " plain")
        kpad = (taps * cin + 63) // 64 * 64
        wf = torch.full((cout, kpad), 7.0, dtype=td, device=dev)
        L.call(fn + "_flat", ops._ptr(wd), taps, cin, cout, ops._ptr(wf), ops._stream())
        wantf = torch.zeros(cout, kpad, dtype=td)
        wantf[:, :taps * cin] = want.reshape(taps * cin, cout).t()
        E.assert_bits16(wf, wantf, fn + "_flat")


@LP
@pytest.mark.parametrize("ks,cin", [(7, 44), (7, 3), (3, 3)])
def test_corner_table_prep_weights_stem16_and_flat8(ks, cin, lp, dev):
    """mmh_prep_weights_stem16_k ([ks][64][pitch], k = kw C8 + c, zero padded) and mmh_prep_weights_lp16_flat8
    ([Cout][Kpad], k = tap C8 + c)"""
    from mmhand_amd import lib as L, ops
    td = ops._wd(lp)
    w = _table_weights(td, ks * ks, cin, 64).reshape(ks, ks, cin, 64)
    want = E.rne16(w.double(), td)
    wd = w.to(dev)
    c8 = (cin + 7) // 8 * 8
    pitch = 32 * ((ks * c8 + 31) // 32) + 8
    n = L.load().mmh_conv_stem16_weights_bytes_k(c8, ks) // 2
    assert n == ks * 64 * pitch
    out = torch.full((n,), 7.0, dtype=td, device=dev)
    L.call("mmh_prep_weights_stem16_k", ops._ptr(wd), cin, c8, ks, ops._dt(lp), ops._ptr(out), ops._stream())
    ws = torch.zeros(ks, 64, pitch, dtype=td)
    ws[:, :, :ks * c8].reshape(ks, 64, ks, c8)[..., :cin] = want.permute(0, 3, 1, 2)             # [kh][n][kw][c]
    E.assert_bits16(out.reshape(ks, 64, pitch), ws, "mmh_prep_weights_stem16_k")
    kpad = (ks * ks * c8 + 63) // 64 * 64
    outf = torch.full((64, kpad), 7.0, dtype=td, device=dev)
    L.call("mmh_prep_weights_lp16_flat8", ops._ptr(wd), ks * ks, cin, 64, c8, ops._dt(lp), ops._ptr(outf), ops._stream())
    wf = torch.zeros(64, kpad, dtype=td)
    wf[:, :ks * ks * c8].reshape(64, ks * ks, c8)[..., :cin] = want.reshape(ks * ks, cin, 64).permute(2, 0, 1)
    E.assert_bits16(outf, wf, "mmh_prep_weights_lp16_flat8")


@LP
def test_corner_table_act_bwd_lp16(lp, dev):
    """mmh_act_bwd_lp16 with the ReLU mask open (y = 1): the stored value is RNE(g); closed (y = -1): +0"""
    from mmhand_amd import lib as L, ops
    td = ops._wd(lp)
    buf, want, g = _table(td, dev)
    out = ops.raw_act_bwd_lp16(g, torch.ones_like(g), L.ACT_RELU, lp)
    E.assert_bits16(out, want, "mmh_act_bwd_lp16, mask open")
    fin = buf.isfinite()
    out0 = ops.raw_act_bwd_lp16(g, -torch.ones_like(g), L.ACT_RELU, lp)
    assert not bool(out0.cpu()[fin].double().abs().any())


# ============================================================================================ in-kernel conversions of fp32 operands
def _ties(shape, seed, td):
    """odd integers in (cap, 2 cap): each lies half-way between two values of td - RNE sends half of them up and half down"""
    cap = int(E.XMAX[td])
    g = torch.Generator().manual_seed(seed)
    v = 2 * torch.randint(cap // 2, cap - 1, tuple(shape), generator=g) + 1
    sgn = 2 * torch.randint(0, 2, tuple(shape), generator=g) - 1
    t = (v * sgn).to(torch.float32)
    s = E.round_shares(t.double(), td)
    assert s["ties"] == 1.0 and s["ties_up"] > 0.4 and s["ties_down"] > 0.4
    return t


@LP
@pytest.mark.parametrize("case", E.N4_HEAD[1:])
def test_in_kernel_conversion_of_the_n4_head_weight(case, lp, dev, monkeypatch):
    """mmh_conv7_n4_lp16 converts its fp32 w itself: w = ties, x in {-1, 0, 1}; y (fp32, exact) is the oracle's on RNE(w)"""
    from mmhand_amd import ops
    from oracle import ops_ref as R
    B, H, W, refl = case
    td = ops._wd(lp)
    x, bias = E.ints((B, H, W, 64), E.SEED_X), E.ints((4,), E.SEED_B, lo=-2, hi=2)
    w = _ties((7, 7, 64, 4), 31, td) * E.ints((7, 7, 64, 4), E.SEED_W, E.W_DENSITY).abs()
    want = R.conv2d(x, E.rne16(w.double(), td).double(), bias, 1, 3, refl)
    assert float(want.abs().max()) < E.CAP_F32
    ops.bump_weights_epoch()
    calls = _spy(monkeypatch)
    y = ops.raw_conv_fprop(x.to(dev), w.to(dev), bias.to(dev), 1, 3, refl, 0, bf16=lp)
    assert calls["mmh_conv7_n4_lp16"] == 1, calls
    E.assert_exact(y, want, "four-column head fprop on a weight of ties")


@LP
@pytest.mark.parametrize("case", E.HEAD_WGRAD[1:])
def test_in_kernel_conversion_of_the_head_wgrad_dy(case, lp, dev, monkeypatch):
    """mmh_conv7_head_wgrad_lp16 converts its fp32 dy itself: dy = ties, x in {-1, 0, 1}; dw (fp32, exact) is the oracle's on RNE(dy)"""
    from mmhand_amd import ops
    from oracle import ops_ref as R
    B, H, W = case
    td = ops._wd(lp)
    x = E.ints((B, H, W, 64), E.SEED_X)
    dy = _ties((B, H, W, 4), 32, td) * (torch.rand((B, H, W, 4), generator=torch.Generator().manual_seed(33)) < 0.25)
    dy[..., -1] = 0
    w0 = torch.zeros(7, 7, 64, 4)
    want = R.conv2d_grads(x, w0, None, E.rne16(dy.double(), td).double(), 1, 3, True)[2].detach()
    assert float(want.abs().max()) < E.CAP_F32
    x16 = ops.lp16_twin(x.to(dev), lp)
    calls = _spy(monkeypatch)
    dw = ops.raw_head_wgrad16(x16, dy.to(dev), lp)
    assert dict(calls) == {"mmh_conv7_head_wgrad_lp16": 1}, calls
    E.assert_exact(dw, want, "head wgrad on a dy of ties")


@LP
@pytest.mark.parametrize("which", ["dy", "w"])
def test_in_kernel_conversion_of_the_head_dgrad_operands(which, lp, dev, monkeypatch):
    """mmh_conv7_head_dgrad_lp16 converts its fp32 dy (head_dgrad_embed_kernel) and w (head_dgrad_w_kernel) itself: one of them
    ties, the other in {-1, 0, 1}; the result is the documented sequence on the RNE-rounded operand"""
    from types import SimpleNamespace
    from mmhand_amd import ops
    case = E.HEAD_DGRAD[1]
    B, H, W = case
    td = ops._wd(lp)
    x = torch.zeros(B, H, W, 64)
    dy, w = E.ints((B, H, W, 4), E.SEED_DY), E.ints((7, 7, 64, 4), E.SEED_W, E.W_DENSITY)
    thin = lambda t, seed: t * (torch.rand(t.shape, generator=torch.Generator().manual_seed(seed)) < 0.25)     # noqa: E731
    if which == "dy":           # a quarter of the pixels carry a tie: every padded-domain term stays finite in fp16
        dy = thin(_ties((B, H, W, 4), 34, td), 36)
    else:
        w, dy = _ties((7, 7, 64, 4), 35, td) * w.abs(), thin(dy, 37)
    dy[..., -1] = 0; w[..., -1] = 0
    P = SimpleNamespace(x=x, dy=dy, w=w, td=td)
    R_ = SimpleNamespace(x=x, dy=E.rne16(dy.double(), td).float(), w=E.rne16(w.double(), td).float(), td=td)
    got = _head_dgrad(ops, P, case, lp, dev, monkeypatch, "head dgrad")
    assert float(E.head_dgrad_sequence(R_, td, False).abs().max()) < (E.CAP_F32 if lp is True else E.FP16_MAX)
    E.assert_exact(got[False], E.head_dgrad_sequence(R_, td, False), f"head dgrad, fp32 dx, {which} of ties")
    E.assert_bits16(got[True], E.head_dgrad_sequence(R_, td, True), f"head dgrad, 16-bit dx, {which} of ties")
