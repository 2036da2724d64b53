"""The HBM-bound kernels of csrc/pointwise.hip against the float64 references of tests/_pointwise_oracle.py, ELEMENT BY ELEMENT,
through the C-ABI: the activation backward, MaxPool2d(2, 2), the L1 / MSE / BCE losses, scale-shift-activation, the PATBlock
gate, the image pool exchange, the non-finite flag and Adam - at one vector, on either side of a block and past the grid cap,
where a lane takes the second turn of its grid-stride loop.  Families 1 to 8 are exact (integer or dyadic inputs: bit for bit);
the families with transcendentals are held per element to |got - want| <= TOL * S + 2^-126 and print their worst
|got - want| / S.  tests/test_pointwise_exact_cpu.py checks the premises of every case here without a GPU.  Every output starts
from NaN: an element the kernel does not write fails the comparison."""
import itertools
from types import SimpleNamespace

import pytest
import torch

from tests import _exact as E
from tests import _pointwise_oracle as PO
from tests.test_pointwise_gpu import TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _drop_the_cached_cases():
    yield
    PO.clear_caches()       # the large cases and their float64 references: about 1 GB of host memory

ALL = ("f32", "bf16", "fp16")
LP = ("bf16", "fp16")
CODE = {"f32": 0, "bf16": 1, "fp16": 2}        # MMH_F32 | MMH_BF16 | MMH_FP16


def _nan(shape, dev, dtype="f32"):
    return torch.full(tuple(shape), float("nan"), dtype=PO.DTYPES[dtype], device=dev)


def _to(t, dev, dtype="f32"):
    return t.to(PO.DTYPES[dtype]).to(dev).contiguous()


def _same(got, want64, what):
    """bit for bit; compared on the device, E.assert_exact names the element when they differ"""
    if tuple(got.shape) == tuple(want64.shape) and torch.equal(got.double(), want64.to(got.device)):
        return
    E.assert_exact(got, want64, what)


def _abi():
    from mmhand_amd import lib as L
    from mmhand_amd import ops
    return L, ops._ptr, ops._stream


# ------------------------------------------------------------------------------------------------ 1. activation backward
@pytest.mark.parametrize("act", [PO.ACT_RELU, PO.ACT_TANH], ids=["relu", "tanh"])
@pytest.mark.parametrize("n", PO.N_F4)
def test_act_bwd_exact(n, act, dev):
    L, ptr, stream = _abi()
    P = PO.act_bwd_case(n)
    g, y, dx = _to(P.g, dev), _to(P.y, dev), _nan((n,), dev)
    L.call("mmh_act_bwd", ptr(g), ptr(y), ptr(dx), n, act, stream())
    _same(dx, P.want[act], f"mmh_act_bwd n={n} act={act}")


@pytest.mark.parametrize("lp", LP)
@pytest.mark.parametrize("act", [PO.ACT_RELU, PO.ACT_TANH], ids=["relu", "tanh"])
@pytest.mark.parametrize("n", PO.N_8)
def test_act_bwd_lp16_and_io_exact(n, act, lp, dev):
    """mmh_act_bwd_lp16 and the four (g 16-bit, y 16-bit) forms of mmh_act_bwd_lp16_io"""
    L, ptr, stream = _abi()
    P = PO.act_bwd_case(n)
    g = {False: _to(P.g, dev), True: _to(P.g, dev, lp)}
    y = {False: _to(P.y, dev), True: _to(P.y, dev, lp)}
    out = _nan((n,), dev, lp)
    L.call("mmh_act_bwd_lp16", ptr(g[False]), ptr(y[False]), n, act, CODE[lp], ptr(out), stream())
    _same(out, P.want[act], f"mmh_act_bwd_lp16 n={n} act={act} {lp}")
    for g16, y16 in itertools.product((False, True), repeat=2):
        out = _nan((n,), dev, lp)
        L.call("mmh_act_bwd_lp16_io", ptr(g[g16]), int(g16), ptr(y[y16]), int(y16), n, act, CODE[lp], ptr(out), stream())
        _same(out, P.want[act], f"mmh_act_bwd_lp16_io n={n} act={act} {lp} g16={g16} y16={y16}")


# ------------------------------------------------------------------------------------------------ 2. MaxPool2d(2, 2)
@pytest.mark.parametrize("shape", PO.MAXPOOL, ids=str)
def test_maxpool_exact_on_tied_inputs(shape, dev):
    L, ptr, stream = _abi()
    P = PO.maxpool_case(shape)
    B, H, W, C = shape
    x, g = _to(P.x, dev), _to(P.g, dev)
    y, dx = _nan(P.y.shape, dev), _nan(shape, dev)
    L.call("mmh_maxpool2x2_fwd", ptr(x), B, H, W, C, ptr(y), stream())
    L.call("mmh_maxpool2x2_bwd", ptr(x), ptr(g), B, H, W, C, ptr(dx), stream())
    _same(y, P.y, f"mmh_maxpool2x2_fwd {shape}")
    _same(dx, P.dx, f"mmh_maxpool2x2_bwd {shape}")


# ------------------------------------------------------------------------------------------------ 3. L1 / MSE forward
def _reduce(dev, n, vec, launch):
    """one loss forward with the workspace at exactly mmh_reduce_ws_bytes(n), NaN before the call: afterwards the partial sums the
    final pass reads are all written, and nothing is behind them - up to a guard past the workspace's end"""
    L, ptr, stream = _abi()
    nbytes = int(L.load().mmh_reduce_ws_bytes(n))
    slots, used = nbytes // 4, min(-(-(n // vec) // PO.TPB), 4096)
    assert 1 <= used <= slots
    ws, out = _nan((slots + 64,), dev), _nan((), dev)
    launch(L, ptr, stream, out, ws, nbytes)
    host = ws.cpu()
    assert not bool(torch.isnan(host[:used]).any()), "a partial sum that the final pass reads was not written"
    assert bool(torch.isnan(host[used:]).all()), "a slot behind the last partial sum was written"
    return float(out)


@pytest.mark.parametrize("kind", ["l1", "mse"])
@pytest.mark.parametrize("n", PO.N_F4)
def test_l1_mse_forward_is_the_integer_sum(n, kind, dev):
    P = PO.loss_case(n)
    a, b = _to(P.a, dev), _to(P.b, dev)
    total = P.l1 if kind == "l1" else P.mse
    for weight, denom, want in [(1.0, 1.0, total)] + [(w, float(n), PO.weighted(total, w, n)) for w in PO.LOSS_WEIGHTED]:
        got = _reduce(dev, n, 4, lambda L, ptr, stream, out, ws, nb: L.call(
            f"mmh_{kind}_fwd", ptr(a), ptr(b), n, weight, denom, ptr(out), ptr(ws), nb, stream()))
        assert got == want, (kind, n, weight, got, want, got - want)


@pytest.mark.parametrize("lp", LP)
@pytest.mark.parametrize("n", PO.N_8)
def test_l1_forward_lp16_is_the_integer_sum(n, lp, dev):
    P = PO.loss_case(n)
    a, b = _to(P.a, dev, lp), _to(P.b, dev, lp)
    for weight, denom, want in [(1.0, 1.0, P.l1)] + [(w, float(n), PO.weighted(P.l1, w, n)) for w in PO.LOSS_WEIGHTED]:
        got = _reduce(dev, n, 8, lambda L, ptr, stream, out, ws, nb: L.call(
            "mmh_l1_fwd_lp16", ptr(a), ptr(b), n, weight, denom, CODE[lp], ptr(out), ptr(ws), nb, stream()))
        assert got == want, (n, lp, weight, got, want, got - want)


# ------------------------------------------------------------------------------------------------ 4. L1 / MSE backward
@pytest.mark.parametrize("kind", ["l1", "mse"])
@pytest.mark.parametrize("n", PO.N_F4)
def test_l1_mse_backward_exact(n, kind, dev):
    L, ptr, stream = _abi()
    P = PO.loss_case(n)
    a, b, da = _to(P.a, dev), _to(P.b, dev), _nan((n,), dev)
    gs = torch.tensor(PO.BWD_GS, dtype=torch.float32, device=dev)
    L.call(f"mmh_{kind}_bwd", ptr(a), ptr(b), n, PO.BWD_WEIGHT, PO.BWD_DENOM, ptr(gs), ptr(da), stream())
    _same(da, P.l1_bwd if kind == "l1" else P.mse_bwd, f"mmh_{kind}_bwd n={n}")


@pytest.mark.parametrize("lp", LP)
@pytest.mark.parametrize("n", PO.N_8)
def test_l1_relu_backward_lp16_exact(n, lp, dev):
    L, ptr, stream = _abi()
    P = PO.loss_case(n)
    a, b, out = _to(P.a, dev, lp), _to(P.b, dev, lp), _nan((n,), dev, lp)
    gs = torch.tensor(PO.BWD_GS, dtype=torch.float32, device=dev)
    L.call("mmh_l1_relu_bwd_lp16", ptr(a), ptr(b), n, PO.BWD_WEIGHT, PO.BWD_DENOM, ptr(gs), CODE[lp], ptr(out), stream())
    _same(out, P.l1_relu_bwd, f"mmh_l1_relu_bwd_lp16 n={n} {lp}")


# ------------------------------------------------------------------------------------------------ 5. scale, shift, activation
@pytest.mark.parametrize("opt", PO.SSA_OPTIONS, ids=lambda o: f"pw_v2={o[0]}-row_chunks={o[1]}")
@pytest.mark.parametrize("geom", PO.SSA_GEOMS, ids=str)
def test_scale_shift_act_exact_in_every_type(geom, opt, dev):
    """x dtype x out dtype x twin {none, bf16, fp16} x {ReLU, dropout mask, residual}: out, the twin and the keep bits"""
    L, ptr, stream = _abi()
    groups, rows, C = geom
    v2, rc = opt
    P = PO.ssa_case(geom)
    x = {d: _to(P.x, dev, d) for d in ALL}
    scale, shift, residual, mask = _to(P.scale, dev), _to(P.shift, dev), _to(P.residual, dev), P.mask.to(dev)
    c8 = C // 8
    twin_ok = bool(v2) and C % 8 == 0 and c8 <= 256 and c8 & (c8 - 1) == 0
    runs = 0
    with E.options(pw_v2=v2, row_chunks=rc):
        for mode in PO.SSA_MODES:
            relu, drop, res = mode
            want, bits = PO.ssa_ref(geom, mode)
            want_d, bits_d = want.to(dev), bits.to(dev)
            for xd, od, td in itertools.product(ALL, ALL, (None,) + LP if twin_ok else (None,)):
                what = f"mmh_scale_shift_act {geom} {opt} relu={relu} drop={drop} res={res} x={xd} out={od} twin={td}"
                out = _nan((groups, rows, C), dev, od)
                kb = torch.full(tuple(bits.shape), 0xA5, dtype=torch.uint8, device=dev)
                args = (ptr(x[xd]), ptr(scale), ptr(shift), ptr(residual) if res else None, ptr(out), groups, rows, C, int(relu),
                        0.5 if drop else 0.0, 0, ptr(mask) if drop else None, ptr(kb), CODE[xd], CODE[od])
                if td is None:
                    L.call("mmh_scale_shift_act", *args, stream())
                else:
                    twin = _nan((groups, rows, C), dev, td)
                    L.call("mmh_scale_shift_act_twin", *args, ptr(twin), CODE[td], stream())
                    if not torch.equal(twin.double(), want_d):
                        E.assert_exact(twin, want, what + ": twin")
                if not torch.equal(out.double(), want_d):
                    E.assert_exact(out, want, what)
                if not torch.equal(kb, bits_d):
                    E.assert_exact(kb, bits.double(), what + ": keep bits")
                runs += 1
        if not twin_ok:         # no kernel writes a twin here: the launcher says so, it does not quietly leave the twin out
            out, twin = _nan((groups, rows, C), dev), _nan((groups, rows, C), dev, "bf16")
            rc_ = L.load().mmh_scale_shift_act_twin(ptr(x["f32"]), ptr(scale), ptr(shift), None, ptr(out), groups, rows, C, 0, 0.0, 0, None,
                                                    None, CODE["f32"], CODE["f32"], ptr(twin), CODE["bf16"], stream())
            assert rc_ != 0 and bool(torch.isnan(twin.float()).all())
    assert runs == len(PO.SSA_MODES) * 9 * (3 if twin_ok else 1)


# ------------------------------------------------------------------------------------------------ 6. PATBlock gate, routing
@pytest.mark.parametrize("shape", PO.GATE_SHAPES, ids=str)
def test_gate_forward_routing_exact(shape, dev):
    """call A (s2 = s3 = 0): out = x1 + s1 / 4 and the `out` halves of the cats; call B (s1 = 0): where s3 and s2 are copied to"""
    L, ptr, stream = _abi()
    rows, C = shape
    P = PO.gate_exact_case(shape)
    x1 = _to(P.x1, dev)
    for cat, sd in itertools.product(ALL, ALL):
        for name, s1, s2, s3, want in (("A", P.s1f, P.zero, P.zero, P.fwd_a), ("B", P.zero, P.s2c, P.s3c, P.fwd_b)):
            s1d, s2d, s3d = _to(s1, dev), _to(s2, dev, sd), _to(s3, dev, sd)
            out, x2n, x3n = _nan(shape, dev), _nan((rows, 2 * C), dev, cat), _nan((rows, 2 * C), dev, cat)
            L.call("mmh_patblock_gate_fwd", ptr(x1), ptr(s1d), ptr(s2d), ptr(s3d), ptr(out), ptr(x2n), ptr(x3n), rows, C, CODE[cat],
                   CODE[sd], stream())
            for got, w, part in zip((out, x2n, x3n), want, ("out", "x2n = cat(s3, out)", "x3n = cat(s2, out)")):
                _same(got, w, f"mmh_patblock_gate_fwd {shape} call {name} cat={cat} s23={sd}: {part}")
            if cat == "f32":        # without the cats
                out = _nan(shape, dev)
                L.call("mmh_patblock_gate_fwd", ptr(x1), ptr(s1d), ptr(s2d), ptr(s3d), ptr(out), None, None, rows, C, CODE[cat], CODE[sd],
                       stream())
                _same(out, want[0], f"mmh_patblock_gate_fwd {shape} call {name} no cats s23={sd}")
    z, out, x2n = _to(P.zero, dev), _nan(shape, dev), _nan((rows, 2 * C), dev)
    assert L.load().mmh_patblock_gate_fwd(ptr(x1), ptr(z), ptr(z), ptr(z), ptr(out), ptr(x2n), None, rows, C, 0, 0, stream()) != 0
    assert bool(torch.isnan(out).all())         # one cat without the other is refused, nothing ran


@pytest.mark.parametrize("shape", PO.GATE_SHAPES, ids=str)
def test_gate_backward_routing_exact(shape, dev):
    """s2 = s3 = 0: g_x1 = G, g_s1 = G / 4, g_s2 = G s1 / 8 + g_x3n[.., :C], g_s3 = G s1 / 8 + g_x2n[.., :C] - every combination of the
    gradient dtypes with all three incoming gradients, and every subset of them present in fp32 and in bf16"""
    L, ptr, stream = _abi()
    rows, C = shape
    P = PO.gate_exact_case(shape)
    s1 = _to(P.s1b, dev)
    combos = [(gc, sd, gd, (1, 1, 1)) for gc, sd, gd in itertools.product(ALL, ALL, ALL)]
    combos += [(d, d, d, has) for d in ("f32", "bf16") for has in itertools.product((0, 1), repeat=3) if has != (1, 1, 1)]
    for gc, sd, gd, has in combos:
        g_out = _to(P.g_out, dev) if has[0] else None
        g2 = _to(P.g_x2n, dev, gc) if has[1] else None
        g3 = _to(P.g_x3n, dev, gc) if has[2] else None
        s2, s3 = _to(P.zero, dev, sd), _to(P.zero, dev, sd)
        outs = (_nan(shape, dev), _nan(shape, dev), _nan(shape, dev, gd), _nan(shape, dev, gd))
        L.call("mmh_patblock_gate_bwd", ptr(g_out), ptr(g2), ptr(g3), ptr(s1), ptr(s2), ptr(s3), *[ptr(o) for o in outs], rows, C,
               CODE[gc], CODE[sd], CODE[gd], stream())
        for got, want, part in zip(outs, PO.gate_exact_bwd(P, *has), ("g_x1", "g_s1", "g_s2", "g_s3")):
            _same(got, want, f"mmh_patblock_gate_bwd {shape} gcat={gc} s23={sd} gs23={gd} present={has}: {part}")


# ------------------------------------------------------------------------------------------------ 7. image pool exchange
def test_pool_exchange_exact_past_the_block_cap(dev):
    L, ptr, stream = _abi()
    P = PO.pool_case()
    pool, images, out = _to(P.pool, dev), _to(P.images, dev), _nan((PO.POOL_B, PO.POOL_ELEMS), dev)
    src = torch.tensor(PO.POOL_SRC, dtype=torch.int32, device=dev)
    dst = torch.tensor(PO.POOL_DST, dtype=torch.int32, device=dev)
    L.call("mmh_pool_exchange", ptr(pool), ptr(images), ptr(out), ptr(src), ptr(dst), PO.POOL_B, PO.POOL_ELEMS, stream())
    _same(out, P.out, "mmh_pool_exchange: out")
    _same(pool, P.after, "mmh_pool_exchange: pool")


# ------------------------------------------------------------------------------------------------ 8. non-finite gradient flag
def test_grad_nonfinite_sees_every_position(dev):
    from mmhand_amd import ops
    buf = torch.ones(PO.NONFINITE_N + 4, device=dev)
    flag, own = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    one, zero = torch.ones(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)

    def run(n, flag_in=None, with_own=False):
        flag.fill_(7); own.fill_(7)
        ops.grad_nonfinite(buf[:n], flag, flag_in, own if with_own else None)
        return int(flag), int(own)

    for r in range(4):
        n = PO.NONFINITE_N + r
        buf[n] = float("inf")                       # the element behind the last one is not the gradient's
        assert run(n) == (0, 7), r
        assert run(n, zero, True) == (0, 0) and run(n, one, True) == (1, 0), r       # a carried flag survives; own_out is this call's alone
        for pos in PO.nonfinite_positions(r):
            for bad in (float("inf"), float("-inf"), float("nan")):
                buf[pos] = bad
                assert run(n) == (1, 7), (r, pos, bad)
                buf[pos] = 1.0
        pos = PO.nonfinite_positions(r)[-1]
        buf[pos] = float("nan")
        assert run(n, zero, True) == (1, 1) and run(n, one, True) == (1, 1), r
        buf[pos] = 1.0
        buf[n] = 1.0
    assert run(PO.NONFINITE_N) == (0, 7)


# ------------------------------------------------------------------------------------------------ 9. BCE with logits
@pytest.mark.parametrize("target", [0.0, 1.0])
def test_bce_forward_points_around_the_series_threshold(target, dev):
    """n = 4, weight = denom = 1: the sum of one group of four points (the groups of PO.BCE_GROUPS: four neighbours of the sorted
    grid, and every point on its own).  At target 0 and negative x, S is the softplus alone: what holds both of its branches."""
    worst = 0.0
    for grp in PO.BCE_GROUPS:
        x = torch.tensor(grp, dtype=torch.float32, device=dev)
        got = _reduce(dev, 4, 4, lambda L, ptr, stream, out, ws, nb: L.call(
            "mmh_bce_logits_fwd", ptr(x), 4, target, 1.0, 1.0, ptr(out), ptr(ws), nb, stream()))
        want, S = PO.bce_terms(PO.f32(grp), target)
        worst = max(worst, PO.within(torch.tensor([got], dtype=torch.float64), want.sum().reshape(1), S.sum().reshape(1), TOL,
                                     f"mmh_bce_logits_fwd target={target} x={grp}"))
    print(f"\n[worst] bce forward, target {target}: |got - want| / S = {worst:.3e}")


@pytest.mark.parametrize("target", [0.0, 1.0])
def test_bce_backward_points(target, dev):
    L, ptr, stream = _abi()
    pts = PO.BCE_GRID + [0.0] * (-len(PO.BCE_GRID) % 4)
    x, dx = torch.tensor(pts, dtype=torch.float32, device=dev), _nan((len(pts),), dev)
    gs = torch.tensor(PO.BCE_GS, dtype=torch.float32, device=dev)
    L.call("mmh_bce_logits_bwd", ptr(x), len(pts), target, 1.0, 1.0 / PO.BCE_K, ptr(gs), ptr(dx), stream())
    want, S = PO.bce_bwd(PO.f32(pts), target, PO.BCE_K * PO.BCE_GS)
    worst = PO.within(dx, want, S, TOL, f"mmh_bce_logits_bwd target={target}")
    print(f"\n[worst] bce backward, target {target}: |got - want| / S = {worst:.3e}")


@pytest.mark.parametrize("target", [0.0, 1.0])
def test_bce_past_the_grid_cap(target, dev):
    """the same grid tiled to n = 4 195 332: the two-level reduction at 4096 partials against the float64 sum, bound TOL * sum(S);
    the backward element by element"""
    L, ptr, stream = _abi()
    xc = PO.bce_large()
    n = xc.numel()
    x = xc.to(dev)
    got = _reduce(dev, n, 4, lambda L, ptr, stream, out, ws, nb: L.call(
        "mmh_bce_logits_fwd", ptr(x), n, target, 1.0, 1.0, ptr(out), ptr(ws), nb, stream()))
    want, S = PO.bce_terms(xc.double(), target)
    worst = PO.within(torch.tensor([got], dtype=torch.float64), want.sum().reshape(1), S.sum().reshape(1), TOL,
                      f"mmh_bce_logits_fwd target={target} n={n}")
    dx, gs = _nan((n,), dev), torch.tensor(PO.BCE_GS, dtype=torch.float32, device=dev)
    L.call("mmh_bce_logits_bwd", ptr(x), n, target, 1.0, 1.0 / PO.BCE_K, ptr(gs), ptr(dx), stream())
    wantb, Sb = PO.bce_bwd(xc.double(), target, PO.BCE_K * PO.BCE_GS)
    worstb = PO.within(dx, wantb, Sb, TOL, f"mmh_bce_logits_bwd target={target} n={n}")
    print(f"\n[worst] bce at n = {n}, target {target}: forward {worst:.3e}, backward {worstb:.3e}")


def test_bce_halves_is_two_const_calls(monkeypatch, dev):
    """BCEWithLogitsHalvesFn == BCEWithLogitsConstFn(x[:B], 1) and (x[B:], 0) on contiguous copies: both losses and both halves of dx
    bit for bit, also with one of the two losses unused.  The Function does not switch gradient materialisation off, so autograd
    hands its backward a zero tensor for an unused loss and never None; the `g is None` branch is therefore reached by calling
    backward directly, with dx starting from NaN: the half without a gradient must come out +0.0, the other half untouched by it."""
    from mmhand_amd import ops
    x = (PO.mk((4, 5, 7, 8), 91) * 3.0).to(dev)
    xa, xb = x[:2].clone().requires_grad_(True), x[2:].clone().requires_grad_(True)
    ra, fb = ops.BCEWithLogitsConstFn.apply(xa, 1.0, 2.0), ops.BCEWithLogitsConstFn.apply(xb, 0.0, 2.0)
    (ra * 3.0).backward(); (fb * 0.5).backward()
    xh = x.clone().requires_grad_(True)
    real, fake = ops.BCEWithLogitsHalvesFn.apply(xh, 2.0)
    assert torch.equal(real, ra) and torch.equal(fake, fb) and float(real.detach()) != float(fake.detach())
    (real * 3.0 + fake * 0.5).backward()
    assert torch.equal(xh.grad[:2], xa.grad) and torch.equal(xh.grad[2:], xb.grad)
    for use_real in (True, False):      # through autograd: a materialised zero gradient, the kernel runs with k = 0
        xo = x.clone().requires_grad_(True)
        real, fake = ops.BCEWithLogitsHalvesFn.apply(xo, 2.0)
        (real * 3.0 if use_real else fake * 0.5).backward()
        used, unused = (xo.grad[:2], xo.grad[2:]) if use_real else (xo.grad[2:], xo.grad[:2])
        assert torch.equal(used, xa.grad if use_real else xb.grad)
        assert float(unused.abs().max()) == 0.0 and float(used.abs().max()) > 0.0
    # the None branch, by a direct call: backward allocates dx with torch.empty_like - here it starts from NaN
    ctx = SimpleNamespace(saved_tensors=(x,), weight=2.0)
    g3, g05 = torch.tensor(3.0, device=dev), torch.tensor(0.5, device=dev)
    monkeypatch.setattr(torch, "empty_like", lambda t, **kw: torch.full_like(t, float("nan"), **kw))
    dx_real, none = ops.BCEWithLogitsHalvesFn.backward(ctx, g3, None)
    dx_fake, _ = ops.BCEWithLogitsHalvesFn.backward(ctx, None, g05)
    monkeypatch.undo()
    assert none is None and tuple(dx_real.shape) == tuple(x.shape) == tuple(dx_fake.shape)
    assert torch.equal(dx_real[:2], xa.grad) and int(dx_real[2:].contiguous().view(torch.int32).abs().max()) == 0
    assert torch.equal(dx_fake[2:], xb.grad) and int(dx_fake[:2].contiguous().view(torch.int32).abs().max()) == 0


# ------------------------------------------------------------------------------------------------ 10. gate with real sigmoids
@pytest.mark.parametrize("dt", ALL)
def test_gate_with_real_sigmoids_per_element(dt, dev):
    """s2, s3 on {0, +-0.25, +-1, +-4, +-12, +-30, +-90}^2: forward and the four backward outputs; dt is the type of the cats, of s2 / s3
    and of every gradient that may be 16-bit (the references take the rounded inputs)"""
    L, ptr, stream = _abi()
    rows, C = PO.GATE_REAL_SHAPE
    P = PO.gate_real_case()
    rnd = lambda t: t.to(PO.DTYPES[dt]).float()
    fwd, fwd_S, bwd, bwd_S = PO.gate_real_ref(P.x1, P.s1, rnd(P.s2), rnd(P.s3), P.g_out, rnd(P.g_x2n), rnd(P.g_x3n))
    x1, s1, s2, s3 = _to(P.x1, dev), _to(P.s1, dev), _to(P.s2, dev, dt), _to(P.s3, dev, dt)
    out, x2n, x3n = _nan((rows, C), dev), _nan((rows, 2 * C), dev, dt), _nan((rows, 2 * C), dev, dt)
    L.call("mmh_patblock_gate_fwd", ptr(x1), ptr(s1), ptr(s2), ptr(s3), ptr(out), ptr(x2n), ptr(x3n), rows, C, CODE[dt], CODE[dt], stream())
    worst = {"out": PO.within(out, fwd[0], fwd_S, TOL, f"gate forward {dt}: out")}
    for got, want, part in ((x2n, fwd[1], "x2n"), (x3n, fwd[2], "x3n")):
        _same(got[:, :C], want[:, :C].contiguous(), f"gate forward {dt}: the copied half of {part}")
        worst[part] = PO.within(got[:, C:], want[:, C:], fwd_S, TOL, f"gate forward {dt}: the out half of {part}", dtype=dt)
    g_out, g2, g3 = _to(P.g_out, dev), _to(P.g_x2n, dev, dt), _to(P.g_x3n, dev, dt)
    outs = (_nan((rows, C), dev), _nan((rows, C), dev), _nan((rows, C), dev, dt), _nan((rows, C), dev, dt))
    L.call("mmh_patblock_gate_bwd", ptr(g_out), ptr(g2), ptr(g3), ptr(s1), ptr(s2), ptr(s3), *[ptr(o) for o in outs], rows, C, CODE[dt],
           CODE[dt], CODE[dt], stream())
    for got, want, S, part, d in zip(outs, bwd, bwd_S, ("g_x1", "g_s1", "g_s2", "g_s3"), ("f32", "f32", dt, dt)):
        worst[part] = PO.within(got, want, S, TOL, f"gate backward {dt}: {part}", dtype=d)
    print(f"\n[worst] gate {dt}: |got - want| / S = " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------ 11. Adam
@pytest.mark.parametrize("n", PO.N_ADAM)
def test_adam_three_steps_per_element(n, dev):
    """mmh_adam_step against float64 on the same fp32 state, step by step, with grad_scale 0.5 and a loss scale of 1024; a skipped
    step moves nothing and does not count; mmh_adam_step_dev leaves the same m and v bit for bit"""
    L, ptr, stream = _abi()
    from mmhand_amd import ops
    cfg = PO.ADAM
    P = PO.adam_case(n)
    p, pd = P.p0.to(dev), P.p0.to(dev)
    m, v, md, vd = (torch.zeros(n, device=dev) for _ in range(4))
    step, coef = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(2, device=dev)
    lr, ls = torch.full((1,), cfg["lr"], device=dev), torch.full((1,), cfg["loss_scale"], device=dev)
    skip = torch.zeros(1, dtype=torch.int32, device=dev)

    def both(g, t):
        ops.adam_step(p, g, m, v, cfg["lr"], cfg["beta1"], cfg["beta2"], cfg["eps"], t, cfg["grad_scale"], skip, ls)
        L.call("mmh_adam_step_dev", ptr(pd), ptr(g), ptr(md), ptr(vd), n, ptr(lr), cfg["beta1"], cfg["beta2"], cfg["eps"], ptr(step),
               cfg["grad_scale"], ptr(skip), ptr(ls), ptr(coef), stream())

    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for i, gc in enumerate(P.grads):
        g = gc.to(dev)
        before = [t.clone() for t in (p, m, v, pd, md, vd)]
        if i == 1:              # an overflow step in between
            skip.fill_(1)
            both(g, i + 1)
            skip.fill_(0)
            assert all(torch.equal(a, b) for a, b in zip(before, (p, m, v, pd, md, vd))) and int(step) == i
        both(g, i + 1)
        assert int(step) == i + 1
        (pw, mw, vw), (Sm, Sv) = PO.adam_ref(before[0].cpu(), gc, before[1].cpu(), before[2].cpu(), i + 1)
        worst["m"] = max(worst["m"], PO.within(m, mw, Sm, TOL, f"adam n={n} step {i + 1}: m"))
        worst["v"] = max(worst["v"], PO.within(v, vw, Sv, TOL, f"adam n={n} step {i + 1}: v"))
        err = (p.double().cpu() - pw).abs()
        allow = PO.ADAM_P_ATOL + PO.ADAM_P_RTOL * pw.abs()
        assert bool((err <= allow).all()), (n, i, int((err > allow).sum()), float(err.max()))
        worst["p"] = max(worst["p"], float((err / allow).max()))
        assert torch.equal(m, md) and torch.equal(v, vd)
        assert torch.allclose(p, pd, rtol=0, atol=1e-9)
    assert float((p.cpu() - P.p0).abs().max()) > 1e-4
    print(f"\n[worst] adam n={n}: |got - want| / S: m {worst['m']:.3e}, v {worst['v']:.3e}; p: {worst['p']:.3e} of its allowance")
