"""The round-once problems of tests/_exact.py without a GPU: (a) every (family, case, type, edge) that
tests/test_conv_round16_gpu.py uses meets the conditions on the oracle alone (shares of inexact results, ties both ways,
negative inexact results under ReLU - printed under -s), and so do the fp16-overflow and NaN / inf problems; (b) the reference
rounding rne16 equals an independent integer-arithmetic rounding of the fp32 bit pattern, on the corner table and on 2^20
seeded bit patterns; (c) the gap these families close, written down as a test: an epilogue that truncates, one that rounds half
away from zero and one that rounds twice around the bias each pass the capped (_B16) problems of the exact suite bit for bit,
and each fails a round-once problem."""
import numpy as np
import pytest
import torch

from tests import _exact as E

TDS = [torch.bfloat16, torch.float16]


def _id(v):
    return "-".join(str(p) for p in v) if isinstance(v, tuple) else str(v)


# ------------------------------------------------------------------------------------------------ (a) the conditions
@pytest.mark.parametrize("fam,case,lp,edge", E.round_cases(), ids=_id)
def test_round_once_conditions_hold(fam, case, lp, edge):
    P = E.round_problem(fam, case, lp, edge)            # asserts the conditions
    assert P.shares and set(P.shares) == set(P.spec[-1])
    for out, s in P.shares.items():
        print(f"\n[shares] {fam} {case} {lp} {edge or 'main'} {out}: xm = {P.xm} " + " ".join(f"{k} = {v:.3f}" for k, v in s.items()))
        assert s["inexact"] >= E.MIN_INEXACT and s["ties"] >= E.MIN_TIES and s["ties_up"] >= E.MIN_TIES_UP and s["ties_down"] >= E.MIN_TIES_DOWN
        if out == "y":
            assert s["neg_inexact"] >= E.MIN_NEG_INEXACT
    assert P.y.dtype == torch.float64 and P.dx.dtype == torch.float64


def test_round_cases_cover_every_family_in_both_types():
    seen = {(f, lp, e) for f, _, lp, e in E.round_cases()}
    for fam in E.ROUND_FAMILIES:
        for lp in ("bf16", "fp16"):
            assert (fam, lp, None) in seen
            assert ((fam, lp, "scaled") in seen) == ("persist" not in fam)


@pytest.mark.parametrize("fam", sorted(E.OVERFLOW_CASES))
def test_overflow_problems_straddle_the_fp16_threshold(fam):
    P = E.overflow_problem(fam, E.OVERFLOW_CASES[fam])      # asserts: the steered values are met exactly, nothing else overflows
    for out, ts in P.targets.items():
        res = P.y if out == "y" else P.dx
        r = E.rne16(res, torch.float16)
        assert len({t[1] for t in ts}) == 1                 # one output row
        n_inf = int(r.isinf().sum())
        n_edge = int(((res.abs() > E.FP16_MAX) & r.isfinite()).sum())
        print(f"\n[overflow] {fam} {out}: {n_edge} elements in (65504, 65520) -> +-65504, {n_inf} elements >= 65520 -> +-inf")
        assert n_inf >= E.MIN_EACH_SIDE and n_edge >= E.MIN_EACH_SIDE
        assert bool((r[(res.abs() > E.FP16_MAX) & r.isfinite()].abs() == E.FP16_MAX).all())
        assert float(r[tuple(ts[6])]) == float("inf")       # 65520 itself: the tie goes to even, which is 2^16


@pytest.mark.parametrize("lp", ["bf16", "fp16"])
@pytest.mark.parametrize("fam", [f for f in E.ROUND_FAMILIES if "persist" not in f])
def test_special_value_problems_mark_the_receptive_field(fam, lp):
    P = E.special_problem(fam, E.ROUND_FAMILIES[fam][0][0], lp)      # asserts: non-finite set == receptive field
    for out in P.spec[-1]:
        res = P.y if out == "y" else P.dx
        assert bool(res.isnan().any()) and bool(res.isfinite().any())


def test_a_condition_that_does_not_hold_is_refused():
    v = torch.arange(-200.0, 200.0, dtype=torch.float64)             # all exact in bf16
    with pytest.raises(AssertionError, match="share of inexact"):
        E.check_round_conditions(v, torch.bfloat16, "small integers")
    with pytest.raises(AssertionError, match="not finite"):
        E.check_round_conditions(torch.tensor([70000.0], dtype=torch.float64), torch.float16, "too large")
    with pytest.raises(AssertionError, match="not exactly representable in fp32"):
        E.rne16(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64), torch.bfloat16)


# ------------------------------------------------------------------------------------------------ (b) the reference rounding
def _rne_bits(u, td):
    """RNE of fp32 bit patterns (uint32 numpy) to bf16 / fp16 bit patterns, in integer arithmetic only; NaN -> a quiet NaN"""
    u = u.astype(np.uint64)
    sign, a = (u >> 16) & 0x8000, u & 0x7FFFFFFF
    nan = a > 0x7F800000
    if td is torch.bfloat16:
        out = (u + 0x7FFF + ((u >> 16) & 1)) >> 16                  # add half minus one, plus the kept lsb: ties go to even
        return np.where(nan, sign | 0x7FC0, out & 0xFFFF).astype(np.uint16)
    m = a - (112 << 23)                                              # normal results: rebias the exponent (127 -> 15)
    normal = (m + 0xFFF + ((m >> 13) & 1)) >> 13
    e, frac = a >> 23, a & 0x7FFFFF
    mant = np.where(e > 0, frac | 0x800000, frac)                    # value = mant 2^(max(e, 1) - 150); in units of 2^-24: >> s
    s = np.minimum(126 - np.maximum(e, 1), 40)
    q, rem, half = mant >> s, mant & ((np.uint64(1) << s) - 1), np.uint64(1) << (s - 1)
    sub = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    out = np.where(a >= 0x477FF000, 0x7C00, np.where(a >= 0x38800000, normal, sub))       # 65520 and above: inf
    return np.where(nan, sign | 0x7E00, sign | out).astype(np.uint16)


def _check_rne16(f32, td):
    want = _rne_bits(f32.numpy().view(np.uint32), td)
    got = E.rne16(f32.double(), td)
    gb = got.view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(f32.numpy())
    assert bool(got.isnan().numpy()[nan].all())
    bad = (gb != want) & ~nan
    assert not bad.any(), (td, int(bad.sum()), hex(int(f32.numpy().view(np.uint32)[bad][0])), hex(int(gb[bad][0])), hex(int(want[bad][0])))


@pytest.mark.parametrize("td", TDS, ids=["bf16", "fp16"])
def test_rne16_equals_integer_rounding_of_the_bit_pattern(td):
    table = E.corner_table(td)
    assert len(table) % 8 == 6 and bool(table.isnan().any()) and bool(table.isinf().any())
    _check_rne16(table, td)
    rng = np.random.default_rng(20)
    u = rng.integers(0, 2 ** 32, size=2 ** 20, dtype=np.uint64).astype(np.uint32)
    if td is torch.float16:                                          # half of them where fp16 has its range: exponents 2^-27 .. 2^17
        u[::2] = (u[::2] & 0x807FFFFF) | (rng.integers(100, 145, size=2 ** 19, dtype=np.uint64).astype(np.uint32) << 23)
    _check_rne16(torch.from_numpy(u.view(np.float32).copy()), td)


@pytest.mark.parametrize("td", TDS, ids=["bf16", "fp16"])
def test_corner_table_holds_what_it_says(td):
    t = E.corner_table(td).double()
    fin = t[t.isfinite()]
    s = E.round_shares(fin, td)
    assert s["ties_up"] > 0.1 and s["ties_down"] > 0.1 and s["inexact"] > 0.6
    r = E.rne16(t, td)
    assert bool((r.isinf() & t.isfinite()).any())                    # a finite value that must overflow
    sub = 2.0 ** (-126 if td is torch.bfloat16 else -14)
    assert bool(((r.double().abs() < sub) & (r != 0)).any()) and bool(((r == 0) & (t != 0)).any())      # subnormal results; a tie to zero
    trip = E.round_shares(t[:3], td)
    assert trip["ties"] == pytest.approx(1 / 3) and E.round_shares(torch.cat([t, t[:2]])[-1:], td)["ties"] == 1.0


@pytest.mark.parametrize("td", TDS, ids=["bf16", "fp16"])
def test_round_shares_agree_with_the_cast(td):
    """the shares are computed on the value's own grid in float64; the cast knows nothing of that: inexact <=> the cast moves it"""
    P = E.round_problem("halo_fprop", E.HALO_FPROP[0], "bf16" if td is torch.bfloat16 else "fp16")
    moved = float((E.rne16(P.y, td).double() != P.y).double().mean())
    assert moved == P.shares["y"]["inexact"]


# ------------------------------------------------------------------------------------------------ (c) the gap
def _step(t16, towards_larger):
    """the neighbour of a finite 16-bit value, one unit away in magnitude (sign-magnitude bit patterns)"""
    b = t16.view(torch.int16).to(torch.int32) & 0xFFFF
    b = b + (1 if towards_larger else -1)
    return ((b + 0x8000) % 0x10000 - 0x8000).to(torch.int16).view(t16.dtype)


def _truncate(v, bias, td):
    r = E.rne16(v, td)
    return torch.where(r.double().abs() > v.abs(), _step(r, False), r)


def _half_away(v, bias, td):
    lo = _truncate(v, bias, td)
    hi = _step(lo, True)
    tie = (lo.double() != v) & ((v.abs() - lo.double().abs()) == (hi.double().abs() - v.abs()))
    return torch.where(tie, hi, E.rne16(v, td))


def _twice_around_bias(v, bias, td):
    return E.rne16(E.rne16(v - bias.double(), td).double() + bias.double(), td)


WRONG = [_truncate, _half_away, _twice_around_bias]


@pytest.mark.parametrize("td", TDS, ids=["bf16", "fp16"])
@pytest.mark.parametrize("wrong", WRONG, ids=lambda f: f.__name__.strip("_"))
def test_wrong_epilogues_pass_the_capped_problems_and_fail_the_round_once_ones(wrong, td):
    lp = "bf16" if td is torch.bfloat16 else "fp16"
    for fam, case in (("halo_fprop", E.HALO_FPROP[0]), ("stem16", E.STEM16[0]), ("s2_lp16", E.S2_LP16[0])):
        old = E.case_problem(fam, case)                              # results within the exact range of the type: nothing rounds
        for act in (lambda t: t, lambda t: t.clamp_min(0.0)):
            E.assert_rounded_once(wrong(act(old.y), old.bias, td), act(old.y), td, f"capped {fam}")
            E.assert_exact(wrong(act(old.y), old.bias, td), act(old.y), f"capped {fam}")
        new = E.round_problem(fam, case, lp)
        with pytest.raises(AssertionError, match="differ bit for bit; first at index"):
            E.assert_rounded_once(wrong(new.y, new.bias, td), new.y, td, f"round-once {fam}")
        E.assert_rounded_once(E.rne16(new.y, td), new.y, td, f"round-once {fam}")


def test_relu_after_the_rounding_is_not_seen_here_but_the_order_is_fixed():
    """RNE commutes with ReLU (it is monotone and keeps zero), so 'ReLU after the rounding' stores the same bits - except the sign
    of a zero that a negative value rounds to, which assert_bits16 compares: -2^-26 rounds to -0 in fp16, relu(-2^-26) is +0"""
    v = torch.tensor([-2.0 ** -26, 3.0, -5.0], dtype=torch.float64)
    after = E.rne16(v, torch.float16).clamp_min(0.0)
    after = torch.where(E.rne16(v, torch.float16) == 0, E.rne16(v, torch.float16), after)       # a relu that lets -0 through
    with pytest.raises(AssertionError, match="first at index \\(0,\\)"):
        E.assert_rounded_once(after, v.clamp_min(0.0), torch.float16, "relu after the rounding")


def test_assert_rounded_once_compares_zero_signs_and_nan_by_nan_ness():
    td = torch.float16
    v = torch.tensor([0.0, -0.0, float("nan"), 1.0], dtype=torch.float64)
    E.assert_rounded_once(torch.tensor([0.0, -0.0, float("nan"), 1.0], dtype=td), v, td, "same")
    other_nan = torch.tensor([0x0000, 0x8000 - 0x10000, 0xFE01 - 0x10000, 0x3C00], dtype=torch.int16).view(td)
    assert bool(other_nan[2].isnan())
    E.assert_rounded_once(other_nan, v, td, "another NaN payload")
    with pytest.raises(AssertionError, match="1 of 4 elements differ bit for bit; first at index \\(1,\\)"):
        E.assert_rounded_once(torch.tensor([0.0, 0.0, float("nan"), 1.0], dtype=td), v, td, "+0 for -0")
    with pytest.raises(AssertionError):
        E.assert_rounded_once(torch.tensor([0.0, -0.0, 1.0, 1.0], dtype=td), v, td, "a number for NaN")
    with pytest.raises(AssertionError):
        E.assert_rounded_once(torch.zeros(4, dtype=torch.bfloat16), v, td, "another type")


@pytest.mark.parametrize("lp", ["bf16", "fp16"])
def test_the_two_rounding_sequences_differ_from_one_rounding(lp):
    """the documented two-rounding paths (border_add on a 16-bit dx, the head dgrad's 16-bit padded domain) are NOT the rounding
    of the fp32 result: their GPU tests must hold them to the sequence, and these problems can tell the two apart"""
    td = E.TD[lp]
    for case in E.FOLD_DGRAD:
        P = E.round_problem("fold_dgrad", case, lp)
        twice, share = E.border_sequence(P, td)
        ring = torch.zeros(P.dx.shape, dtype=torch.bool)
        ring[:, [1, -2], :, :] = True; ring[:, :, [1, -2], :] = True
        differs = E._bits16(twice) != E._bits16(E.rne16(P.dx, td))
        assert share > 0 and not bool((differs & ~ring).any())       # only the ring pixels are rounded twice
    for case in E.HEAD_DGRAD:
        P = E.round_problem("head_dgrad", case, lp)
        assert not torch.equal(E.head_dgrad_sequence(P, td, False), P.dx)
        assert bool((E._bits16(E.head_dgrad_sequence(P, td, True)) != E._bits16(E.rne16(P.dx, td))).any())
