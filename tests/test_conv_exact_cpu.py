"""The integer-exact method of tests/_exact.py has teeth - shown on the CPU with PyTorch's own fp32 convolution as the stand-in
kernel: (a) it equals the float64 oracle bit for bit on integer inputs, (b) the caps hold for every case the GPU file
(tests/test_conv_exact_gpu.py) uses, (c) one tap dropped at one output element fails assert_exact - which names the element -
while the whole-tensor relative L1 of the same pair stays under the 2e-5 the kernel tests allow."""
import pytest
import torch

from oracle import ops_ref as R
from tests import _exact as E

# (B, H, W, Cin, Cout, k, pad): reflect padding, stride 1
SHAPES = [(1, 16, 16, 512, 512, 3, 1), (2, 9, 11, 256, 256, 3, 1), (2, 16, 16, 44, 64, 7, 3), (2, 16, 16, 64, 4, 7, 3)]


def _standin(P, k, pad, act=0):
    """PyTorch's fp32 convolution and its autograd: the 'kernel' under test here"""
    # clones: at fp32 the oracle's .to(dtype) is no copy, and it marks its operands as requiring a gradient
    return R.conv2d_grads(P.x.clone(), P.w.clone(), P.bias.clone(), P.dy, 1, pad, True, act, dtype=torch.float32)


@pytest.mark.parametrize("shape", SHAPES)
def test_fp32_conv_equals_the_fp64_oracle_on_integers(shape):
    B, H, W, Cin, Cout, k, pad = shape
    P = E.problem(B, H, W, Cin, Cout, k, 1, pad, True)
    y, dx, dw, db = _standin(P, k, pad)
    assert y.dtype == torch.float32
    E.assert_exact(y, P.y, "y"); E.assert_exact(dx, P.dx, "dx"); E.assert_exact(dw, P.dw, "dw"); E.assert_exact(db, P.db, "db")
    # the premise: far below the 256 that bf16 still represents exactly (a factor of 2 left at K = 4608)
    assert max(float(t.abs().max()) for t in (P.y, P.dx, P.dw)) <= 128


@pytest.mark.parametrize("family", sorted(E.FAMILIES))
def test_caps_hold_for_every_gpu_case(family):
    """problem() checks on the oracle's result alone that it is integer-valued and within the cap of its storage type"""
    cases, spec = E.FAMILIES[family]
    assert cases
    for case in cases:
        P = E.problem(*spec(case))
        assert P.y.dtype == torch.float64 and P.dx.dtype == torch.float64


def test_caps_of_the_stand_alone_sums():
    rows, cols = E.COLSUM
    assert float(E.ints((rows, cols), 1).double().sum(0).abs().max()) <= rows < E.CAP_F32
    P_, T, Cin, Cout = E.WINO_WGRAD_DMA
    assert T < E.CAP_F32          # |sum over T tiles of products of values in {-1, 0, 1}| <= T


def test_a_cap_that_does_not_hold_is_refused():
    x, w, dy = E.ints((1, 8, 8, 256), 1), E.ints((3, 3, 256, 64), 2), E.ints((1, 8, 8, 64), 4)       # dense weights
    with pytest.raises(AssertionError, match="exceeds the cap"):
        E.exact_conv(x, w, None, dy, 1, 1, True, cap_y=16.0)
    with pytest.raises(AssertionError, match="not integer-valued"):
        E.exact_conv(x * 0.5, w, None, dy, 1, 1, True)


def test_ints_is_seeded_integer_valued_and_masked():
    a, b = E.ints((64, 64), 5, 1.0 / 3.0), E.ints((64, 64), 5, 1.0 / 3.0)
    assert torch.equal(a, b) and not torch.equal(a, E.ints((64, 64), 6, 1.0 / 3.0))
    assert a.dtype == torch.float32 and torch.equal(a, a.round()) and float(a.abs().max()) == 1.0
    dense = E.ints((64, 64), 5)
    assert 0.55 < float((dense != 0).float().mean()) < 0.78             # {-1, 0, 1} uniformly: two thirds non-zero
    assert 0.15 < float((a != 0).float().mean()) < 0.30                 # ... of which the mask keeps a third
    t = E.ints((1000,), 7, lo=-8, hi=8)
    assert float(t.min()) == -8.0 and float(t.max()) == 8.0


def test_one_dropped_tap_fails_exact_and_passes_rel_l1():
    """The gap: one tap's contribution missing from ONE output element of a 1 x 16 x 16 x 512 tensor"""
    B, H, W, Cin, Cout, k, pad = SHAPES[0]
    P = E.problem(B, H, W, Cin, Cout, k, 1, pad, True)
    y = _standin(P, k, pad)[0]
    b, h, w_, c = 0, 9, 5, 137                                      # an interior pixel: no reflection in its taps
    taps = [(i, j, float((P.x[b, h + i - 1, w_ + j - 1, :] * P.w[i, j, :, c]).sum())) for i in range(3) for j in range(3)]
    i, j, contrib = next(t for t in taps if t[2] != 0.0)
    bad = y.clone()
    bad[b, h, w_, c] -= contrib
    with pytest.raises(AssertionError) as err:
        E.assert_exact(bad, P.y, "mutated y")
    msg = str(err.value)
    assert "1 of %d elements differ" % P.y.numel() in msg and f"(b, h, w, c) = ({b}, {h}, {w_}, {c})" in msg, msg
    assert f"largest |got - want| = {abs(contrib)}" in msg, msg
    rel = R.rel_l1(bad, P.y)
    assert 0.0 < rel < 2e-5, rel                                    # the kernel tests' whole-tensor bound does not notice
    with pytest.raises(AssertionError, match="do not round to the oracle"):
        E.assert_rounds(bad, P.y, "mutated y")                      # the Winograd form of the check does
    E.assert_exact(y, P.y, "y")
