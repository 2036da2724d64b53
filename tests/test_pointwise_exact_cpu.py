"""The premises of tests/test_pointwise_exact_gpu.py, checked without a GPU on the references of tests/_pointwise_oracle.py alone:
(a) for every case the conditions that make "exact" true hold - each reference value is finite and exactly representable in
every type it is stored in, each sum is an integer below 2^24; (b) the sizes lie where the comments say: on either side of a
block and past the grid caps; (c) each point of the BCE grid falls on the side of the series threshold its comment claims;
(d) the hand-written references equal torch's CPU implementations (max_pool2d and its backward on tied inputs, float64
binary_cross_entropy_with_logits, autograd through the gate, torch.optim.Adam); (e) one wrong element in four million fails
assert_exact while the whole-tensor relative L1 the older tests use stays under their 2e-5."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import ops_ref as R
from tests import _exact as E
from tests import _pointwise_oracle as PO

ALL = ("f32", "bf16", "fp16")
LP = ("bf16", "fp16")


@pytest.fixture(scope="module", autouse=True)
def _drop_the_cached_cases():
    yield
    PO.clear_caches()       # the large cases and their float64 references: about 1 GB of host memory


def test_sizes_lie_on_either_side_of_a_block_and_past_the_caps():
    for sizes, vec, cap in ((PO.N_F4, 4, 4096), (PO.N_8, 8, 4096), (PO.N_ADAM, 1, 8192)):
        lanes = [n // vec for n in sizes]
        assert lanes == [1, 255, 257, cap * PO.TPB + 257] and all(n % vec == 0 for n in sizes)
        second = lanes[3] - cap * PO.TPB                # lanes of the second turn: one block and one lane, so it ends mid-block
        assert 0 < second and second % PO.TPB == 1
    assert PO.POOL_ELEMS // 4 - 256 * PO.TPB == 257 and PO.POOL_ELEMS % 4 == 0
    B, H, W, C = PO.MAXPOOL[-1]
    assert B * (H // 2) * (W // 2) * (C // 4) > 4096 * PO.TPB
    assert all(h % 2 == 0 and w % 2 == 0 and c % 4 == 0 for _, h, w, c in PO.MAXPOOL)


@pytest.mark.parametrize("n", sorted(set(PO.N_F4 + PO.N_8)))
def test_act_bwd_references_are_exact_in_every_type(n):
    P = PO.act_bwd_case(n)
    for t in (P.g, P.y):
        PO.check_exact(t.double(), ALL, "input")
    for act in (PO.ACT_RELU, PO.ACT_TANH):
        PO.check_exact(P.want[act], ALL, f"act_bwd[{act}]")
    if n >= 1020:
        y = P.y
        assert bool((y == 0).any()) and bool((y == 1).any()) and bool((y == -1).any())
        assert float(P.want[PO.ACT_TANH].abs().max()) == 3.0 and bool((P.want[PO.ACT_TANH] != P.want[PO.ACT_RELU]).any())


@pytest.mark.parametrize("shape", PO.MAXPOOL, ids=str)
def test_maxpool_reference_is_torchs_on_tied_inputs(shape):
    P = PO.maxpool_case(shape)
    PO.check_exact(P.y, ("f32",), "y"); PO.check_exact(P.dx, ("f32",), "dx")
    B, H, W, C = shape
    win = P.dx.reshape(B, H // 2, 2, W // 2, 2, C)
    assert torch.equal(win.sum((2, 4)), P.g.double())                               # the whole gradient, once
    assert torch.equal((win != 0).sum((2, 4)), torch.ones(B, H // 2, W // 2, C, dtype=torch.int64))     # to ONE place (g >= 1)
    xw = P.x.reshape(B, H // 2, 2, W // 2, 2, C)
    tied = ((xw == xw.amax((2, 4), keepdim=True)).sum((2, 4)) > 1).double().mean()
    assert float(tied) > 0.5 or P.x.numel() <= 16, float(tied)                      # most windows tie
    if P.x.numel() <= 1 << 20:
        xn = P.x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        yn = F.max_pool2d(xn, 2, 2)
        yn.backward(P.g.double().permute(0, 3, 1, 2))
        assert torch.equal(yn.detach().permute(0, 2, 3, 1), P.y) and torch.equal(xn.grad.permute(0, 2, 3, 1), P.dx)


@pytest.mark.parametrize("n", sorted(set(PO.N_F4 + PO.N_8)))
def test_loss_sums_are_integers_below_2_24_and_gradients_exact(n):
    P = PO.loss_case(n)
    PO.check_sum(P.l1, "sum |a - b|"); PO.check_sum(P.mse, "sum (a - b)^2")
    assert P.mse <= 4 * n and P.l1 <= 2 * n
    for t in (P.a, P.b):
        PO.check_exact(t.double(), ALL, "input")
    PO.check_exact(P.l1_bwd, ("f32",), "l1_bwd"); PO.check_exact(P.mse_bwd, ("f32",), "mse_bwd")
    PO.check_exact(P.l1_relu_bwd, LP, "l1_relu_bwd")
    if n >= 1020:
        assert 0 < P.n_equal < n and bool((P.l1_relu_bwd == 0).any()) and bool((P.l1_relu_bwd != 0).any())
    for w in PO.LOSS_WEIGHTED:
        assert math.isfinite(PO.weighted(P.l1, w, n)) and PO.weighted(P.l1, 1.0, 1) == P.l1


def _row_geom(groups, rows, C, row_chunks):
    """csrc/pointwise.hip::row_geom restated"""
    c8 = C // 8
    step = (PO.TPB // c8) * 4
    chunks = min(max(1, row_chunks // max(groups, 1)), max(1, rows // (2 * step)))
    rpc = -(-(-(-rows // chunks)) // step) * step
    return PO.TPB // c8, step, -(-rows // rpc), rpc


def test_scale_shift_act_geometries_take_the_branches_their_comments_claim():
    v2 = lambda C: C % 8 == 0 and 1 <= C // 8 <= 256 and (C // 8) & (C // 8 - 1) == 0
    assert [v2(g[2]) for g in PO.SSA_GEOMS] == [True, True, True, False, False]
    assert _row_geom(2, 1073, 64, 4096) == (32, 128, 3, 384) and 1073 - 2 * 384 == 305 and 305 - 2 * 128 == 49
    assert _row_geom(2, 1073, 64, 5) == (32, 128, 2, 640) and _row_geom(2, 1073, 64, 1) == (32, 128, 1, 1152)
    assert all(_row_geom(1, 1500, 8, rc) == (256, 1024, 1, 2048) for rc in (1, 5, 4096)) and 1500 - 1024 == 476
    assert _row_geom(3, 37, 2048, 4096) == (1, 4, 4, 12) and 37 - 3 * 12 == 1 and _row_geom(3, 37, 2048, 5) == (1, 4, 1, 40)
    assert 2 * 36 * 24 // 4 == 432 and 6561 * 96 // 4 == 157464 == 615 * 256 + 24
    assert sorted(set(PO.SSA_OPTIONS)) == [(v, rc) for v in (0, 1) for rc in (1, 5, 4096)]


@pytest.mark.parametrize("geom", PO.SSA_GEOMS, ids=str)
def test_scale_shift_act_references_are_exact_in_every_type(geom):
    P = PO.ssa_case(geom)
    for t in (P.x, P.scale, P.shift, P.residual):
        PO.check_exact(t.double(), ALL, "input")
    assert set(P.scale.unique().tolist()) == {0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0} and set(P.mask.unique().tolist()) == {0, 1}
    for mode in PO.SSA_MODES:
        out, bits = PO.ssa_ref(geom, mode)
        PO.check_exact(out, ALL, f"out{mode}")
        assert float(out.abs().max()) <= 48.0 and torch.equal(out * 2, (out * 2).round())
        assert bits.dtype == torch.uint8 and int(bits.max()) <= 15 and tuple(bits.shape) == (geom[0], geom[1], geom[2] // 4)
        if mode[2] and not mode[0]:
            assert bool(((out > 0).reshape(-1, 4)[:, 0] != ((bits.reshape(-1) & 1) != 0)).any())     # the bits are NOT out > 0


@pytest.mark.parametrize("shape", PO.GATE_SHAPES, ids=str)
def test_gate_routing_references_are_exact_and_autograds(shape):
    P = PO.gate_exact_case(shape)
    assert bool((P.s2c != 0).all()) and bool((P.s3c != 0).all()) and bool((P.s2c != P.s3c).all())
    for t in (P.x1, P.s1f, P.s1b, P.s2c, P.s3c, P.g_out, P.g_x2n, P.g_x3n):
        PO.check_exact(t.double(), ALL, "input")
    for t in P.fwd_a + P.fwd_b:
        PO.check_exact(t, ALL, "forward")
    for has in [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]:
        for t in PO.gate_exact_bwd(P, *has):
            PO.check_exact(t, ALL, f"backward{has}")
    # autograd through the oracle's gate, in float64, at s2 = s3 = 0 (sigmoid(0) = 0.5 exactly)
    ts = [t.double().requires_grad_(True) for t in (P.x1, P.s1b, P.zero, P.zero)]
    outs = R.gate(*ts)
    torch.autograd.backward(outs, [P.g_out.double(), P.g_x2n.double(), P.g_x3n.double()])
    for got, want in zip([t.grad for t in ts], PO.gate_exact_bwd(P, 1, 1, 1)):
        assert torch.equal(got, want)
    for got, want in zip(R.gate(P.x1.double(), P.s1f.double(), P.zero.double(), P.zero.double()), P.fwd_a):
        assert torch.equal(got, want)
    for got, want in zip(R.gate(P.x1.double(), P.zero.double(), P.s2c.double(), P.s3c.double()), P.fwd_b):
        assert torch.equal(got, want)


def test_pool_exchange_reference():
    P = PO.pool_case()
    assert torch.equal(P.out[0], P.pool[2].double()) and not torch.equal(P.after[2], P.pool[2].double())       # the OLD content comes out
    assert torch.equal(P.after[2], P.images[0].double()) and torch.equal(P.after[3], P.images[2].double())
    assert torch.equal(P.after[:2], P.pool[:2].double()) and torch.equal(P.out[1], P.images[1].double())
    assert -1 in PO.POOL_DST and any(s < 0 for s in PO.POOL_SRC) and any(s >= 0 and s in PO.POOL_DST for s in PO.POOL_SRC)


def test_nonfinite_positions_lie_where_their_names_say():
    for r in range(4):
        n = PO.NONFINITE_N + r
        pos = PO.nonfinite_positions(r)
        assert len(pos) == 3 + r == len(set(pos)) and all(0 <= p < n for p in pos)
        assert pos[1] // 4 == PO.CAP - 1 and pos[2] // 4 == PO.CAP and PO.CAP < n // 4            # both are whole vectors
        assert [p for p in pos if p >= 4 * (n // 4)] == list(range(4 * (n // 4), n))               # each tail element, and no other


def test_bce_points_fall_on_the_side_of_the_threshold_their_comments_claim():
    assert sorted(PO.BCE_LOG_SIDE + PO.BCE_SERIES_SIDE) == sorted(PO.BCE_POINTS)
    for p in PO.BCE_POINTS:
        t = math.exp(-abs(float(torch.tensor(p, dtype=torch.float32))))         # of the fp32 value the kernel is given
        margin = PO.BCE_MARGIN.get(p, 0.02)
        if p in PO.BCE_LOG_SIDE:
            assert t >= PO.BCE_THRESHOLD * (1 + margin), (p, t / PO.BCE_THRESHOLD)
        else:
            assert t <= PO.BCE_THRESHOLD * (1 - margin), (p, t / PO.BCE_THRESHOLD)
    # the two nearest points stay at a distance __expf cannot bridge: its error is a few ulp (1e-7 relative) plus the rounding
    # of x * log2(e) at magnitude 10 (1e-6 in the exponent), four orders of magnitude below 0.8 %
    assert min(PO.BCE_MARGIN.values()) >= 0.008
    assert len(PO.BCE_GRID) == 2 * len(PO.BCE_POINTS) - 1 and all(len(g) == 4 for g in PO.BCE_GROUPS)
    assert sorted({p for g in PO.BCE_GROUPS[:len(PO.BCE_GROUPS) - len(PO.BCE_GRID)] for p in g}) == PO.BCE_GRID


@pytest.mark.parametrize("target", [0.0, 1.0])
def test_bce_reference_is_torchs_float64(target):
    x = PO.f32(PO.BCE_GRID).requires_grad_(True)
    want = F.binary_cross_entropy_with_logits(x, torch.full_like(x, target), reduction="none")
    want.sum().backward()
    got, S = PO.bce_terms(x.detach(), target)
    dgot, dS = PO.bce_bwd(x.detach(), target, 1.0)
    for t in (got, S, dgot, dS):
        assert bool(torch.isfinite(t).all())
    # torch forms (1 - t) * x - logsigmoid(x): exact to an ulp of |x|, where this reference keeps the tiny softplus itself
    assert bool(((got - want.detach()).abs() <= 2.0 ** -51 * (x.detach().abs() + 1)).all())
    assert bool(((dgot - x.grad).abs() <= 1e-15 * dS).all())
    assert bool((S >= got.abs()).all()) and bool((dS >= dgot.abs()).all())
    if target == 0.0:       # what makes the series branch visible: at negative x, S is the softplus alone
        neg = x.detach() < 0
        assert torch.equal(S[neg], got[neg])
    big = PO.bce_large()
    assert big.numel() == PO.N_F4[3] and torch.equal(big[:len(PO.BCE_GRID)].double(), x.detach())
    assert math.isfinite(float(PO.bce_terms(big.double(), target)[0].sum()))


def test_gate_reference_is_autograd_through_the_oracles_gate():
    P = PO.gate_real_case()
    assert sorted(set(P.s2[:, 0].tolist())) == PO.GATE_S == sorted(set(P.s3[:, 0].tolist()))
    assert len({(a, b) for a, b in zip(P.s2[:, 0].tolist(), P.s3[:, 0].tolist())}) == len(PO.GATE_S) ** 2      # every pair
    for t in (P.s2, P.s3):
        PO.check_exact(t.double(), ALL, "gate grid")
    ts = [t.double().requires_grad_(True) for t in (P.x1, P.s1, P.s2, P.s3)]
    outs = R.gate(*ts)
    torch.autograd.backward(outs, [P.g_out.double(), P.g_x2n.double(), P.g_x3n.double()])
    for got, want in zip(outs, P.fwd):
        assert bool(torch.isfinite(want).all()) and bool(((got.detach() - want).abs() <= 1e-14 * (1 + want.abs())).all())
    for t, want, S in zip(ts, P.bwd, P.bwd_S):      # autograd forms 1 - sigmoid by subtraction: absolute, relative to S
        assert bool(torch.isfinite(want).all()) and bool(((t.grad - want).abs() <= 1e-14 * S).all())
        assert bool((S >= want.abs() * (1 - 1e-12)).all())


def test_adam_reference_is_torch_optim_adam_in_float64():
    n = 257
    P = PO.adam_case(n)
    cfg = PO.ADAM
    b1, b2, eps = (float(torch.tensor(cfg[k], dtype=torch.float32)) for k in ("beta1", "beta2", "eps"))
    par = torch.nn.Parameter(P.p0.double().clone())
    opt = torch.optim.Adam([par], lr=cfg["lr"], betas=(b1, b2), eps=eps)
    p, m, v = P.p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for i, g in enumerate(P.grads):
        gr = g.double() * (cfg["grad_scale"] / cfg["loss_scale"])
        assert torch.equal(gr.float().double(), gr)                 # the two scalings are exact
        par.grad = gr.clone()
        opt.step()
        (p, m, v), (Sm, Sv) = PO.adam_ref(p, g, m, v, i + 1)
        for t in (p, m, v, Sm, Sv):
            assert bool(torch.isfinite(t).all())
        st = opt.state[par]
        assert torch.allclose(m, st["exp_avg"], rtol=1e-13, atol=0) and torch.allclose(v, st["exp_avg_sq"], rtol=1e-13, atol=0)
        # the reference rounds lr and the two coefficients to float as the host does: 2^-24 relative each on an update of lr * O(1)
        step_size, isb2 = PO.adam_coef(i + 1)
        assert abs(step_size - cfg["lr"] / (1 - b1 ** (i + 1))) <= 2.0 ** -23 * step_size
        assert abs(isb2 - 1 / math.sqrt(1 - b2 ** (i + 1))) <= 2.0 ** -24 * isb2
        assert float((p - par.detach()).abs().max()) <= 3 * 2.0 ** -24 * (i + 1) * step_size * 1.01
    assert float((p - P.p0.double()).abs().max()) > 1e-4


def test_one_wrong_element_in_four_million_fails_exact_and_passes_rel_l1():
    P = PO.act_bwd_case(PO.N_F4[3])
    want = P.want[PO.ACT_TANH]
    got = want.float().clone()
    i = 4 * PO.CAP + 5          # an element of the second turn
    got[i] += 1.0
    assert R.rel_l1(got, want) < 2e-5
    with pytest.raises(AssertionError, match=rf"1 of {want.numel()} elements differ; first at index \(b, h, w, c\) = \({i},\)"):
        E.assert_exact(got, want, "act_bwd")
