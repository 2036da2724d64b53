"""Integer-exact checks of the kernel VARIANTS and work PARTITIONS that the smallest ragged shapes of
tests/test_conv_exact_gpu.py never reach: templates picked above a size threshold, the XCD tile remap, split-K ranges with one
pixel or none and the unrolled slab reducers behind them, persistent kernels whose workgroups walk to a second work item, and
every mmh_set_option knob that selects a separately compiled template or another partition.

Same method as tests/test_conv_exact_gpu.py (tests/_exact.py): inputs in {-1, 0, 1}, a correct direct kernel equals the float64
oracle bit for bit (assert_exact), fp32 Winograd rounds to it (assert_rounds).  Each case is in tests/_exact.py with the branch it
is there for and the arithmetic that selects it; where a host-only query shows the branch, the test asserts it was reached
(tests/test_conv_exact_cpu.py asserts the same queries without a GPU, so a moved threshold fails there first).
Knobs are set through E.option(), which puts back the value the key HAD and asserts that it did."""
import ctypes

import pytest
import torch

from tests import _exact as E
from tests.test_conv_exact_gpu import LP, _dev, _relu, _spy, _twins

pytestmark = pytest.mark.gpu

KNOBS_OFF = {}      # the library's defaults


def _ids(kv):
    return ",".join(f"{k}={v}" for k, v in kv.items()) or "default"


def _no_wino(monkeypatch):
    from mmhand_amd import ops
    monkeypatch.setattr(ops, "USE_WINOGRAD", False)
    return ops


def _wgrad_split_count(ops, case, k=3, s=1, p=1, refl=True):
    """mmh_conv2d_wgrad_ws_bytes / (Mrows * Cout * 4): the split count the launcher will use (host-only)"""
    from mmhand_amd import lib
    B, H, W, Cin, Cout = case
    d = ops.conv_desc(B, H, W, Cin, Cout, k, s, p, refl)
    nbytes = lib.load().mmh_conv2d_wgrad_ws_bytes(ctypes.byref(d))
    assert nbytes % (k * k * Cin * Cout * 4) == 0
    return nbytes // (k * k * Cin * Cout * 4)


# ============================================================================================ fp32 implicit GEMM
@pytest.mark.parametrize("knobs", [KNOBS_OFF, dict(conv_dbuf=1)], ids=_ids)
def test_exact_igemm_bn128_template(knobs, dev, monkeypatch):
    """conv_igemm_kernel<128,2,2,...>: the default for 64 < N, N % 256 != 0; fprop (B in [k][n] order), the folded dgrad's main
    piece and the wgrad of the same N"""
    ops = _no_wino(monkeypatch)
    case = E.IGEMM_BN128[0]
    B, H, W, Cin, Cout = case
    P = E.case_problem("igemm_bn128", case)
    x, w, bias, dy = _dev(P, dev)
    calls = _spy(monkeypatch)
    with E.options(**knobs):
        y = ops.raw_conv_fprop(x, w, bias, 1, 1, True, 0)
        yr = ops.raw_conv_fprop(x, w, bias, 1, 1, True, 1)
        dx = ops.raw_conv_dgrad(dy, w, x.shape, 1, 1, True)
        dw = ops.raw_conv_wgrad(x, dy, 3, 1, 1, True)
    assert calls["mmh_conv2d_fprop"] == 2 and calls["mmh_conv2d_dgrad_folded"] == 1 and calls["mmh_conv2d_wgrad"] == 1, calls
    E.assert_exact(y, P.y, "fprop"); E.assert_exact(yr, _relu(P.y), "fprop + relu")
    E.assert_exact(dx, P.dx, "dgrad"); E.assert_exact(dw, P.dw, "wgrad")


@pytest.mark.parametrize("knobs", [KNOBS_OFF, dict(conv_bn256=0), dict(conv_bn256=0, conv_dbuf=1)], ids=_ids)
def test_exact_igemm_n256_on_both_templates(knobs, dev, monkeypatch):
    """N = 256: the 256-wide template by default, the 128-wide one with two column tiles under conv_bn256 = 0"""
    ops = _no_wino(monkeypatch)
    case = E.IGEMM_BN128[1]
    P = E.case_problem("igemm_bn128", case)
    x, w, bias, dy = _dev(P, dev)
    with E.options(**knobs):
        y = ops.raw_conv_fprop(x, w, bias, 1, 1, True, 1)
        dx = ops.raw_conv_dgrad(dy, w, x.shape, 1, 1, True)
    E.assert_exact(y, _relu(P.y), "fprop + relu"); E.assert_exact(dx, P.dx, "dgrad")


def _xcd_cases():
    """every remap case with the remap on and off; conv_xcd1 where it decides (one column tile), conv_bn256 where it does"""
    out = []
    for case in E.IGEMM_XCD:
        out += [(case, KNOBS_OFF), (case, dict(conv_xcd=0))]
        if case[4] <= 64:
            out.append((case, dict(conv_xcd1=0)))
        if case[4] % 256 == 0:
            out.append((case, dict(conv_bn256=0)))
    return out


@pytest.mark.parametrize("case,knobs", _xcd_cases(), ids=lambda v: _ids(v) if isinstance(v, dict) else "x".join(map(str, v)))
def test_exact_igemm_xcd_remap(case, knobs, dev, monkeypatch):
    """the XCD tile remap with a ragged band (gy = 10: eight row tiles remapped, two on their own ids), with gy = 8 exactly,
    at gx = 2 (128- and 256-wide tiles) and at gx = 1 (conv_xcd1); each also with the remap off - the same integers"""
    ops = _no_wino(monkeypatch)
    B, H, W, Cin, Cout = case
    assert (B * H * W + 127) // 128 >= 8                            # gy >= 8: what the launcher asks of the row tiles
    P = E.case_problem("igemm_xcd", case)
    x, w, bias, dy = _dev(P, dev)
    calls = _spy(monkeypatch)
    with E.options(**knobs):
        y = ops.raw_conv_fprop(x, w, bias, 1, 1, True, 0)
        dx = ops.raw_conv_dgrad(dy, w, x.shape, 1, 1, True)
    assert calls["mmh_conv2d_fprop"] == 1 and calls["mmh_conv2d_dgrad_folded"] == 1, calls
    E.assert_exact(y, P.y, f"fprop {case} {_ids(knobs)}")
    E.assert_exact(dx, P.dx, f"dgrad {case} {_ids(knobs)}")


@pytest.mark.parametrize("case,cw", [(E.IGEMM_CW[0], 1), (E.IGEMM_CW[0], 2), (E.IGEMM_CW[0], 4), (E.IGEMM_CW[1], 0), (E.IGEMM_CW[1], 3)])
def test_exact_igemm_chunks_per_tap_visit(case, cw, dev, monkeypatch):
    """conv_cw: how many 32-channel chunks a tap visit covers (k order of the chunk-major gather)"""
    ops = _no_wino(monkeypatch)
    B, H, W, Cin, Cout = case
    assert Cin % 32 == 0 and (cw == 0 or (Cin // 32) % cw == 0)     # else the launcher falls back to the automatic value
    P = E.case_problem("igemm_cw", case)
    x, w, bias, dy = _dev(P, dev)
    with E.option("conv_cw", cw):
        y = ops.raw_conv_fprop(x, w, bias, 1, 1, True, 1)
        dx = ops.raw_conv_dgrad(dy, w, x.shape, 1, 1, True)
    E.assert_exact(y, _relu(P.y), f"fprop + relu, conv_cw={cw}"); E.assert_exact(dx, P.dx, f"dgrad, conv_cw={cw}")


@pytest.mark.parametrize("knobs", [dict(conv_tall=2), dict(conv_tall=2, conv_xcd1=0), KNOBS_OFF], ids=_ids)
def test_exact_igemm_tall_tiles_fprop(knobs, dev, monkeypatch):
    """conv_igemm_tall_kernel<64,4,1> (256-row tiles) on a plain fprop: conv_tall = 2, 32 < N <= 64, M >= 256 * 512, ragged
    over 256; by default the same problem runs on the 128-row kernel"""
    ops = _no_wino(monkeypatch)
    case = E.IGEMM_TALL[0]
    B, H, W, Cin, Cout = case
    assert 32 < Cout <= 64 and B * H * W >= 256 * 512 and (B * H * W) % 256 != 0
    P = E.case_problem("igemm_tall", case)
    x, w, bias, _ = _dev(P, dev)
    calls = _spy(monkeypatch)
    with E.options(**knobs):
        y = ops.raw_conv_fprop(x, w, bias, 1, 1, False, 0)
    assert dict(calls) == {"mmh_conv2d_fprop": 1}, calls
    E.assert_exact(y, P.y, f"fprop {_ids(knobs)}")


@pytest.mark.parametrize("knobs", [KNOBS_OFF, dict(conv_tall=0)], ids=_ids)
def test_exact_dgrad_s2_tall_multi_piece(knobs, dev, monkeypatch):
    """the stride-2 dgrad's four parity classes in ONE launch of 256-row tiles (conv_tall = 1, the default: 32 < Cin <= 64 and
    >= 256 * 128 rows per class) and of 128-row tiles (conv_tall = 0), at a shape the halo kernel declines"""
    from mmhand_amd import lib, ops
    case = E.DGRAD_S2_TALL[0]
    B, H, W, Cin, Cout = case
    assert 32 < Cin <= 64 and B * (H // 2) * (W // 2) >= 256 * 128
    assert lib.load().mmh_dgrad_s2_halo_supported(ctypes.byref(ops.conv_desc(B, H, W, Cin, Cout, 3, 2, 1, False)), Cin) == 0
    P = E.case_problem("dgrad_s2_tall", case)
    _, w, _, dy = _dev(P, dev)
    calls = _spy(monkeypatch)
    with E.options(**knobs):
        dx = ops.raw_conv_dgrad(dy, w, (B, H, W, Cin), 2, 1, False)
    assert dict(calls) == {"mmh_conv2d_dgrad_folded": 1}, calls
    E.assert_exact(dx, P.dx, f"stride-2 dgrad {_ids(knobs)}")


def test_exact_dgrad_s2_four_launches(dev, monkeypatch):
    """dgrad_s2_multi = 0: one launch per parity class (the stride-2 conv of the igemm list with the halo kernel off, and both
    ConvTranspose2d forwards, which ARE that dgrad)"""
    ops = _no_wino(monkeypatch)
    B, H, W, Cin, Cout, k, s, p, refl = case = E.IGEMM[2]
    P = E.case_problem("igemm", case)
    _, w, _, dy = _dev(P, dev)
    with E.options(dgrad_s2_multi=0, dgrad_s2_halo=0):
        dx = ops.raw_conv_dgrad(dy, w, (B, H, W, Cin), s, p, refl)
    E.assert_exact(dx, P.dx, "stride-2 dgrad, four launches")
    for ct in E.CONVT:
        Pt = E.case_problem("convT", ct)
        xt, wt, bt, dyt = _dev(Pt, dev)
        with E.options(dgrad_s2_multi=0, dgrad_s2_halo=0):
            y = ops.raw_convT_fprop(xt, wt, bt)
        E.assert_exact(y, Pt.y, f"convT fprop, four launches {ct}")


@LP
@pytest.mark.parametrize("case", E.FOLD_DGRAD)
def test_exact_lp16_border_launch_on_wide_tiles(case, lp, dev, monkeypatch):
    """border_bn64 = 0: the eight border GEMMs behind the 16-bit mode-1 dgrad (mmh_conv2d_dgrad_border) on 128-wide tiles"""
    from mmhand_amd import ops
    B, H, W, Cin, Cout = case
    P = E.case_problem("fold_dgrad", case)
    _, w, _, dy = _dev(P, dev)
    ops.bump_weights_epoch()
    dy16 = _twins(ops, lp, dy)
    monkeypatch.setattr(ops, "USE_LP16_FOLD", False)                # every shape of the list through mode 1 + border
    calls = _spy(monkeypatch)
    with E.option("border_bn64", 0):
        dx = ops.raw_conv_dgrad(None, w, (B, H, W, Cin), 1, 1, True, bf16=lp, dy16=dy16)
    assert calls["mmh_conv3x3_lp16"] == 1 and calls["mmh_conv2d_dgrad_border"] == 1, calls
    E.assert_exact(dx, P.dx, "reflect dgrad, 128-wide border tiles")


@pytest.mark.parametrize("knobs", [dict(border_bn64=0), dict(conv_bn256=2)], ids=_ids)
@pytest.mark.parametrize("tile", [2, 4])
def test_rounds_winograd_dgrad_border_variants(tile, knobs, dev, monkeypatch):
    """the fp32 border launch behind a Winograd dgrad on 128- and 256-wide tiles (the border terms are direct products; the
    Winograd main term keeps the whole under `rounds`)"""
    from mmhand_amd import ops
    case = E.WINO24[0]
    B, H, W, Cin, Cout, refl = case
    assert refl and Cin % 256 == 0
    P = E.case_problem("wino24", case)
    _, w, _, dy = _dev(P, dev)
    ops.bump_weights_epoch()
    calls = _spy(monkeypatch)
    with E.options(**knobs):
        dx = ops.raw_conv_dgrad_wino(dy, w, (B, H, W, Cin), refl, tile)
    assert calls["mmh_conv2d_dgrad_border"] == 1, calls
    E.assert_rounds(dx, P.dx, f"F({tile}x{tile}) dgrad + border {_ids(knobs)}")


# ============================================================================================ fp32 wgrad: split-K and the slab sum
@pytest.mark.parametrize("par", [1, 0], ids=["slab_par", "slab_seq"])
@pytest.mark.parametrize("case", E.WGRAD_SPLITS)
def test_exact_wgrad_split_ranges_and_slab_reducers(case, par, dev, monkeypatch):
    """split ranges with a single pixel and with none, summed by slab_reduce_par_kernel<4> (8 <= splits < 32, with its remainder
    loop), <8> (splits >= 32) and the sequential kernel; overwriting and accumulating"""
    ops = _no_wino(monkeypatch)
    B, H, W, Cin, Cout = case
    Pn = B * H * W
    assert _wgrad_split_count(ops, case) == E.WGRAD_SPLITS_N[Pn]
    P = E.case_problem("wgrad_splits", case)
    x, _, _, dy = _dev(P, dev)
    acc = E.ints((3, 3, Cin, Cout), E.SEED_ADD, lo=-8, hi=8)
    calls = _spy(monkeypatch)
    with E.option("slab_reduce_par", par):
        dw = ops.raw_conv_wgrad(x, dy, 3, 1, 1, True)
        dwa = ops.raw_conv_wgrad(x, dy, 3, 1, 1, True, out=acc.to(dev))
    assert dict(calls) == {"mmh_conv2d_wgrad": 2}, calls
    E.assert_exact(dw, P.dw, f"wgrad, {E.WGRAD_SPLITS_N[Pn]} splits")
    E.assert_exact(dwa, P.dw + acc.double(), f"wgrad accumulating, {E.WGRAD_SPLITS_N[Pn]} splits")


def test_exact_wgrad_slots_change_the_partition(dev, monkeypatch):
    """wgrad_slots: the split count follows the number of resident workgroups it is told"""
    ops = _no_wino(monkeypatch)
    case = E.WGRAD_SPLITS[0]
    slots, want = E.WGRAD_SLOTS
    P = E.case_problem("wgrad_splits", case)
    x, _, _, dy = _dev(P, dev)
    before = _wgrad_split_count(ops, case)
    with E.option("wgrad_slots", slots):
        assert _wgrad_split_count(ops, case) == want != before
        dw = ops.raw_conv_wgrad(x, dy, 3, 1, 1, True)
    assert _wgrad_split_count(ops, case) == before
    E.assert_exact(dw, P.dw, f"wgrad, wgrad_slots={slots}")


@pytest.mark.parametrize("case,knobs", [(E.WGRAD_TEMPLATES[0], KNOBS_OFF), (E.WGRAD_TEMPLATES[0], dict(wgrad_dbuf=1)),
                                        (E.WGRAD_TEMPLATES[1], KNOBS_OFF), (E.WGRAD_TEMPLATES[1], dict(wgrad_bn256=0)),
                                        (E.WGRAD_TEMPLATES[1], dict(wgrad_bn256=0, wgrad_dbuf=1)),
                                        (E.WGRAD_TEMPLATES[2], KNOBS_OFF), (E.WGRAD_TEMPLATES[3], KNOBS_OFF)],
                         ids=lambda v: _ids(v) if isinstance(v, dict) else f"N{v[4]}")
def test_exact_wgrad_templates(case, knobs, dev, monkeypatch):
    """conv_wgrad_kernel<256|128|64|32> and the double-buffered <128>, each with Mrows = 108 ragged over the 128-row tile"""
    ops = _no_wino(monkeypatch)
    B, H, W, Cin, Cout = case
    assert (9 * Cin) % 128 != 0
    P = E.case_problem("wgrad_templates", case)
    x, _, _, dy = _dev(P, dev)
    acc = E.ints((3, 3, Cin, Cout), E.SEED_ADD, lo=-8, hi=8)
    calls = _spy(monkeypatch)
    with E.options(**knobs):
        dw = ops.raw_conv_wgrad(x, dy, 3, 1, 1, True)
        dwa = ops.raw_conv_wgrad(x, dy, 3, 1, 1, True, out=acc.to(dev))
    assert dict(calls) == {"mmh_conv2d_wgrad": 2}, calls
    E.assert_exact(dw, P.dw, f"wgrad N={Cout} {_ids(knobs)}")
    E.assert_exact(dwa, P.dw + acc.double(), f"wgrad accumulating N={Cout} {_ids(knobs)}")


# ============================================================================================ fp32 Winograd
def _wino6(monkeypatch):
    from mmhand_amd import ops
    monkeypatch.setattr(ops, "WINOGRAD_TILE", 6)
    monkeypatch.setattr(ops, "WINO6_MIN", 0)
    return ops


WINO_GEMM_KNOBS = [dict(wino_gemm_occ=1), dict(wino_gemm_occ=1, wino_gemm_bn=64), dict(wino_gemm_occ=1, wino_gemm_levels=1),
                   dict(wino_gemm_v2=0, wino_bn256=0), dict(wino_gemm_v2=0, wino_bn256=1), KNOBS_OFF]


@pytest.mark.parametrize("knobs", WINO_GEMM_KNOBS, ids=_ids)
def test_rounds_winograd_persistent_gemm_second_item(knobs, dev, monkeypatch):
    """wino_gemm_kernel<128|64, 2|1> with a grid of 8 * 32 workgroups for 384 (768 at 64-wide tiles) work items: every
    workgroup walks to a second item; and the generic batched kernel on 128- and 256-wide tiles"""
    ops = _wino6(monkeypatch)
    case = E.WINO_PERSIST[0]
    B, H, W, Cin, Cout, refl = case
    tiles = B * -(-H // 6) * -(-W // 6)
    bn = 64 if knobs.get("wino_gemm_bn") == 64 else 128
    work = 64 * -(-tiles // 128) * -(-Cout // bn)
    assert -(-work // 8) > 32 * 1 and Cin % 32 == 0 and Cin > 32          # more items than the occ = 1 grid; two k blocks
    assert ops._wino_tile(B, H, W, Cin, Cout, 3, 1, 1, False) == 6
    P = E.case_problem("wino_persist", case)
    x, w, bias, _ = _dev(P, dev)
    ops.bump_weights_epoch()
    calls = _spy(monkeypatch)
    with E.options(**knobs):
        y = ops.raw_conv_fprop(x, w, bias, 1, 1, refl, 1)
    assert calls["mmh_wino_gemm"] == 1 and calls["mmh_conv2d_fprop"] == 0, calls
    E.assert_rounds(y, _relu(P.y), f"F(6x6) fprop + relu {_ids(knobs)}")


def test_winograd_input_transform_remap_is_bit_identical(dev, monkeypatch):
    """nblk = 288 tiles * 64 channels / 256 = 72 (a multiple of 8, >= 64): wino_xcd only permutes which workgroup transforms which
    tile - V is bit-identical with it on and off, and the conv behind either rounds to the oracle"""
    from mmhand_amd import lib
    ops = _wino6(monkeypatch)
    case = E.WINO_PERSIST[0]
    B, H, W, Cin, Cout, refl = case
    tiles = B * -(-H // 6) * -(-W // 6)
    nblk = (tiles * Cin + 255) // 256
    assert nblk % 8 == 0 and nblk >= 64
    P = E.case_problem("wino_persist", case)
    x, w, bias, _ = _dev(P, dev)
    ops.bump_weights_epoch()
    V = {}
    for on in (1, 0):
        with E.option("wino_xcd", on):
            V[on] = torch.full((64, tiles, Cin), float("nan"), device=dev)
            lib.call("mmh_wino_input", x.data_ptr(), B, H, W, Cin, int(refl), 6, lib.F32, V[on].data_ptr(),
                     torch.cuda.current_stream().cuda_stream)
            y = ops.raw_conv_fprop(x, w, bias, 1, 1, refl, 0)
        E.assert_rounds(y, P.y, f"F(6x6) fprop, wino_xcd={on}")
    assert not torch.isnan(V[1]).any()
    assert torch.equal(V[1], V[0]), "the remapped input transform wrote another V"


@pytest.mark.parametrize("vec", [7, 1, 2, 4])
@pytest.mark.parametrize("case", E.WINO6_FUSED, ids=["128x128", "32x32"])
def test_rounds_winograd_f6x6_two_channels_per_thread(case, vec, dev, monkeypatch):
    """wino6_vec bit 0 / 1 / 2: the input / output / dy transform on two channels per thread; all three passes"""
    ops = _wino6(monkeypatch)
    B, H, W, Cin, Cout, refl = case
    P = E.case_problem("wino6", case)
    x, w, bias, dy = _dev(P, dev)
    ops.bump_weights_epoch()
    with E.option("wino6_vec", vec):
        y = ops.raw_conv_fprop(x, w, bias, 1, 1, refl, 1)
        dx = ops.raw_conv_dgrad(dy, w, x.shape, 1, 1, refl)
        dw = ops.raw_conv_wgrad(x, dy, 3, 1, 1, refl)
    E.assert_rounds(y, _relu(P.y), f"F(6x6) fprop + relu {case} wino6_vec={vec}")
    E.assert_rounds(dx, P.dx, f"F(6x6) dgrad {case} wino6_vec={vec}")
    E.assert_rounds(dw, P.dw, f"F(6x6) wgrad {case} wino6_vec={vec}")


_stage = {}


def _wino_wgrad_operands():
    """integer V, Yh and the float64 dU = V^T Yh of E.WINO_WGRAD_PERSIST, computed once"""
    if "wgrad" not in _stage:
        P_, T, Cin, Cout = E.WINO_WGRAD_PERSIST
        V, Y = E.ints((P_, T, Cin), 21), E.ints((P_, T, Cout), 22, E.W_DENSITY)
        want = torch.bmm(V.double().transpose(1, 2), Y.double())
        assert float(want.abs().max()) <= T < E.CAP_F32
        _stage["wgrad"] = (V, Y, want)
    return _stage["wgrad"]


def _wino_wgrad_splits(L_, T, Cin, Cout, P_):
    nbytes = L_.mmh_wino_wgrad_gemm_ws_bytes(T, Cin, Cout, P_)
    assert nbytes % (P_ * Cin * Cout * 4) == 0
    return nbytes // (P_ * Cin * Cout * 4)


WINO_WGRAD_KNOBS = [KNOBS_OFF, dict(wino_wgrad_occ=4), dict(wino_wgrad_bn256=1), dict(wino_wgrad_slots=256),
                    dict(wino_wgrad_v2=0), dict(wino_wgrad_v2=0, wgrad_xcd=0), dict(wino_wgrad_v2=0, wino_wgrad_bn256=1)]


@pytest.mark.parametrize("knobs", WINO_WGRAD_KNOBS, ids=_ids)
def test_exact_wino_wgrad_gemm_variants(knobs, dev):
    """mmh_wino_wgrad_gemm at the stage level (dU[p] = V[p]^T Yh[p]: a plain GEMM, exact on integers, as
    test_exact_wino_wgrad_dma_gemm holds it): the persistent kernel at 3 and 4 workgroups per CU with 1152 items for at most
    8 * 128 workgroups (a second item each), another split count (wino_wgrad_slots), and the generic kernel with and without
    its XCD order and on 256-wide tiles; nine splits, the last with 99 of 288 tiles"""
    from mmhand_amd import lib
    P_, T, Cin, Cout = E.WINO_WGRAD_PERSIST
    V, Y, want = _wino_wgrad_operands()
    Vd, Yd = V.to(dev), Y.to(dev)           # held to the end of the test: the launch below takes raw addresses
    L_ = lib.load()
    assert L_.mmh_wino_wgrad_gemm_ws_bytes(T, Cin, Cout, P_) == P_ * 9 * Cin * Cout * 4           # not the DMA kernel's
    with E.options(**knobs):
        splits = _wino_wgrad_splits(L_, T, Cin, Cout, P_)
        assert splits == (2 if "wino_wgrad_slots" in knobs else 9)
        if knobs.get("wino_wgrad_v2", 1):
            tps = -(-(-(-T // splits)) // 32) * 32
            items = P_ * -(-T // tps) * (Cin // 128) * (Cout // 128)
            if splits == 9:
                assert -(-items // 8) > 32 * 4                          # more work items than the largest persistent grid
        nws = L_.mmh_wino_wgrad_gemm_ws_bytes(T, Cin, Cout, P_)
        ws = torch.full((nws // 4 + 4,), float("nan"), device=dev)
        dU = torch.full((P_, Cin, Cout), 7.0, device=dev)
        lib.call("mmh_wino_wgrad_gemm", Vd.data_ptr(), Yd.data_ptr(), T, Cin, Cout, P_, lib.F32, ws.data_ptr(), nws,
                 dU.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    E.assert_exact(dU, want, f"Winograd-domain wgrad GEMM {_ids(knobs)}")


@pytest.mark.parametrize("knobs", [dict(wino_bf16_occ=1), dict(wino_bf16_bk=128), KNOBS_OFF], ids=_ids)
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_exact_wino_bf16_gemm_variants(dt, knobs, dev):
    """the 16-bit F(2x2,3x3) GEMM M[p] = V[p] U[p]^T at the stage level, on integers whose products sum below 256 (exact in
    fp32 and in the 16-bit result): the 128-deep k-step, and a grid sized for one workgroup per CU (576 items: a second each)"""
    from mmhand_amd import lib
    P_, T, K, N = E.WINO_BF16_PERSIST
    assert K % 128 == 0 and -(-(P_ * -(-T // 128) * -(-N // 128)) // 8) > 64
    if "bf16" not in _stage:
        V, U = E.ints((P_, T, K), 23), E.ints((P_, N, K), 24, E.W_DENSITY)
        want = torch.bmm(V.double(), U.double().transpose(1, 2))
        assert float(want.abs().max()) <= E.CAP_BF16
        _stage["bf16"] = (V, U, want)
    V, U, want = _stage["bf16"]
    wd = torch.bfloat16 if dt == "bf16" else torch.float16
    Vd, Ud = V.to(dev).to(wd), U.to(dev).to(wd)
    out = torch.full((P_, T, N), 7.0, dtype=wd, device=dev)
    with E.options(**knobs):
        lib.call("mmh_wino_gemm", Vd.data_ptr(), Ud.data_ptr(), out.data_ptr(), T, K, N, P_, lib.BF16 if dt == "bf16" else lib.FP16,
                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    E.assert_exact(out, want, f"16-bit Winograd-domain GEMM {dt} {_ids(knobs)}")


# ============================================================================================ 16-bit direct kernels
@LP
@pytest.mark.parametrize("case", E.HALO_FPROP)
def test_exact_conv3x3_lp16_row_tiles_tap_inner(case, lp, dev):
    """lp16_tap_inner = 1 on the row-tile kernel (lp16_shape 17, the kernel that reads it): the k loop walks the nine taps
    inside a 64-channel chunk instead of the chunks inside a tap"""
    from mmhand_amd import ops
    B, H, W, Cin, Cout, refl = case
    P = E.case_problem("halo_fprop", case)
    x, w, bias, _ = _dev(P, dev)
    with E.options(lp16_shape=17, lp16_tap_inner=1):
        ops.bump_weights_epoch()
        x16 = _twins(ops, lp, x)
        y = ops.raw_conv3x3_lp16(x16, w, bias, refl, 1, lp, 0)
        y16 = ops.raw_conv3x3_lp16(x16, w, bias, refl, 0, lp, 0, out16=True)
    E.assert_exact(y, _relu(P.y), "fprop + relu, fp32 out, tap-inner")
    E.assert_exact(y16, P.y, "fprop, 16-bit out, tap-inner")


def _halo_tiles(B, H, W, N):
    return B * -(-H // E.HALO_TILE) * -(-W // E.HALO_TILE) * (N // E.HALO_TBN)


def _persistent_grid(dev):
    """8 * (CUs / 8): the workgroups the halo launcher starts when there are more tiles than that (as it reads the CU count)"""
    return 8 * (torch.cuda.get_device_properties(dev).multi_processor_count // 8)


@LP
@pytest.mark.parametrize("persist", [1, 0, 2])
def test_exact_conv3x3_lp16_halo_walks_a_second_tile_fprop(persist, lp, dev):
    """288 tiles for 256 persistent workgroups: the halo kernel's loop to a second tile (lp16_persist 1 and 2), and one
    workgroup per tile (0)"""
    from mmhand_amd import ops
    case = E.HALO_PERSIST_FPROP[0]
    B, H, W, Cin, Cout, refl = case
    assert _halo_tiles(B, H, W, Cout) > _persistent_grid(dev)
    P = E.case_problem("halo_persist_fprop", case)
    x, w, bias, _ = _dev(P, dev)
    ops.bump_weights_epoch()
    x16 = _twins(ops, lp, x)
    with E.option("lp16_persist", persist):
        y16 = ops.raw_conv3x3_lp16(x16, w, bias, refl, 1, lp, 0, out16=True)
    E.assert_exact(y16, _relu(P.y), f"fprop + relu, 16-bit out, lp16_persist={persist}")


@LP
@pytest.mark.parametrize("fold", [False, True], ids=["mode1_border", "mode2_fold"])
@pytest.mark.parametrize("persist", [1, 0, 2])
def test_exact_conv3x3_lp16_halo_walks_a_second_tile_dgrad(persist, fold, lp, dev, monkeypatch):
    """the same for the dgrad of a reflect-padded conv: mode 1 (+ border call) and the in-kernel fold (mode 2, which
    lp16_persist = 2 launches one workgroup per tile)"""
    from mmhand_amd import ops
    case = E.HALO_PERSIST_DGRAD[0]
    B, H, W, Cin, Cout = case
    assert _halo_tiles(B, H, W, Cin) > _persistent_grid(dev)
    P = E.case_problem("halo_persist_dgrad", case)
    _, w, _, dy = _dev(P, dev)
    ops.bump_weights_epoch()
    dy16 = _twins(ops, lp, dy)
    monkeypatch.setattr(ops, "USE_LP16_FOLD", fold)
    calls = _spy(monkeypatch)
    with E.option("lp16_persist", persist):
        dx = ops.raw_conv_dgrad(None, w, (B, H, W, Cin), 1, 1, True, bf16=lp, dy16=dy16, out16=True)
    assert calls["mmh_conv3x3_lp16"] == 1 and ("mmh_conv2d_dgrad_border" not in calls) == fold, calls
    E.assert_exact(dx, P.dx, f"reflect dgrad, 16-bit out, fold={fold}, lp16_persist={persist}")
