"""The pointwise reductions under every work partition their knobs select: pw_v2 (second- / first-generation kernels),
col_chunks (how many chunks of rows a column reduction is cut into) and row_chunks (the same for the row-parallel apply passes).
rows_per_chunk = ceil(rows / chunks) leaves the last chunk short or EMPTY (B = 1, 81 x 81, C = 96: 82 chunks of 81 rows, chunk 81
has none; 5000 x 256: 156 chunks of 33 rows, the last four have none) - the kernels guard n == 0, and these tests pin it.

Sums of integers are exact whatever the partition: the column sums and s1 = sum dz of the norm backward (integer g, keep bits,
drop_p 0.5 or 0 - a scale of 2 or 1) are held to float64 element by element (tests/_exact.py).  Everything else keeps the
tolerances of tests/test_pointwise_gpu.py (imported, not copied).  Knobs go through E.option(), which restores what the key had.

tests/test_norm_exact_gpu.py holds s2 and every element of dx EXACTLY on dyadic inputs (tests/_norm_oracle.py) at the default
partition; the tolerance tests here stay: they are the ones with realistic values, count = rows and every partition."""
import itertools

import pytest
import torch

from oracle import ops_ref as R
from tests import _exact as E
from tests._norm_oracle import drop_bytes as _drop_bytes, keep_bytes as _keep_bytes      # the keep-mask layouts, shared with the exact tests
from tests.test_pointwise_gpu import GRAD_TOL, TOL, _mk

pytestmark = pytest.mark.gpu

COMBOS = list(itertools.product((0, 1), (1, 3, 2048), (1, 5, 4096)))      # pw_v2, col_chunks, row_chunks
# (B, H, W, C): the empty-chunk geometry (C / 8 = 12 is no power of two: first-generation kernels whatever pw_v2 says); a short
# last chunk on the second-generation path (1073 rows: neither a multiple of its 32-row step nor of 8 chunks); rows below one chunk
GEOMETRIES = [(1, 81, 81, 96), (2, 37, 29, 64), (3, 6, 6, 24)]


def _knobs(combo):
    return E.options(pw_v2=combo[0], col_chunks=combo[1], row_chunks=combo[2])


def _finite(t, what):
    assert bool(torch.isfinite(t).all()), f"{what}: {int((~torch.isfinite(t)).sum())} of {t.numel()} values are NaN or inf"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def test_exact_colsum_in_every_partition(dev):
    """raw_colsum of E.COLSUM's integers: fp32, bf16 and fp16 input, overwriting and accumulating, in all 18 combinations"""
    from mmhand_amd import ops
    rows, cols = E.COLSUM
    t = E.ints((rows, cols), 11)
    want = t.double().sum(0)
    acc = E.ints((cols,), 12, lo=-8, hi=8)
    td = t.to(dev)
    t16 = {lp: td.to(ops._wd(lp)) for lp in (True, 2)}
    for combo in COMBOS:
        with _knobs(combo):
            E.assert_exact(ops.raw_colsum(rows, cols, td), want, f"colsum fp32 {combo}")
            for lp in (True, 2):
                E.assert_exact(ops.raw_colsum(rows, cols, t16[lp]), want, f"colsum {ops._wd(lp)} {combo}")
            E.assert_exact(ops.raw_colsum(rows, cols, td, out=acc.to(dev)), want + acc.double(), f"colsum accumulating {combo}")
            E.assert_exact(ops.raw_colsum(rows, cols, t16[True], out=acc.to(dev)), want + acc.double(), f"colsum bf16 accumulating {combo}")


def test_exact_colsum_of_a_strided_matrix(dev):
    """cs > C: the columns [0, C) of a wider matrix (the first-generation kernel takes the stride)"""
    from mmhand_amd import lib
    rows, C, cs = 1073, 64, 96
    wide = E.ints((rows, cs), 13)
    want = wide[:, :C].double().sum(0)
    wd = wide.to(dev)
    for combo in COMBOS:
        with _knobs(combo):
            nws = lib.load().mmh_colsum_ws_bytes(rows, C)
            ws = torch.full((nws // 4 + 4,), float("nan"), device=dev)
            out = torch.full((C,), 7.0, device=dev)
            lib.call("mmh_colsum", wd.data_ptr(), rows, C, cs, out.data_ptr(), ws.data_ptr(), nws, 0, lib.F32, _stream())
            E.assert_exact(out, want, f"strided colsum {combo}")


def _bwd_reference(g, keep, dsc, x, mean, invstd, rows):
    """float64 dz, s1, s2, dx of the norm backward from the same fp32 mean / invstd the kernels read (gamma = 1)"""
    dz = g.double() * keep.double() * dsc
    xhat = (x.double() - mean.double()[:, None, None, :]) * invstd.double()[:, None, None, :]
    s1 = dz.sum((1, 2))
    s2 = (dz * xhat).sum((1, 2))
    dx = invstd.double()[:, None, None, :] * (dz - s1[:, None, None, :] / rows - xhat * s2[:, None, None, :] / rows)
    return s1, s2, dx


@pytest.mark.parametrize("g16", [False, True], ids=["g32", "g_bf16"])
@pytest.mark.parametrize("masked,drop_p", [(2, 0.5), (2, 0.0), (0, 0.0)], ids=["keep_p0.5", "keep_p0", "unmasked"])
@pytest.mark.parametrize("shape", GEOMETRIES, ids=lambda s: "x".join(map(str, s)))
def test_exact_norm_bwd_sums_in_every_partition(shape, masked, drop_p, g16, dev):
    """mmh_norm_bwd_reduce: s1 = sum dz exact; s2 and the dx of mmh_norm_bwd_apply within the gradient tolerance"""
    from mmhand_amd import lib
    B, H, W, C = shape
    rows = H * W
    g = E.ints(shape, 31, lo=-3, hi=3)
    x = _mk(shape, 32, "cpu", 2.0, 3.0)
    keep = torch.rand(shape, generator=torch.Generator().manual_seed(33)) < 0.6 if masked else torch.ones(shape, dtype=torch.bool)
    mean = x.mean((1, 2))
    invstd = (x.var((1, 2), unbiased=False) + 1e-5).rsqrt()
    dsc = 1.0 / (1.0 - drop_p)
    s1w, s2w, dxw = _bwd_reference(g, keep, dsc, x, mean, invstd, rows)
    assert float(s1w.abs().max()) < E.CAP_F32 and torch.equal(s1w, s1w.round())
    gd = g.to(dev).to(torch.bfloat16) if g16 else g.to(dev)
    gdt = lib.BF16 if g16 else lib.F32
    xd, md, isd = x.to(dev), mean.to(dev), invstd.to(dev)
    kb = _keep_bytes(keep).to(dev) if masked else None
    kbp = kb.data_ptr() if masked else None
    for combo in COMBOS:
        with _knobs(combo):
            nws = lib.load().mmh_norm_bwd_ws_bytes(B, rows, C)
            ws = torch.full((nws // 4 + 4,), float("nan"), device=dev)
            s1 = torch.full((B, C), 7.0, device=dev); s2 = torch.full((B, C), 7.0, device=dev)
            lib.call("mmh_norm_bwd_reduce", gd.data_ptr(), kbp, xd.data_ptr(), md.data_ptr(), isd.data_ptr(), B, rows, C, masked,
                     drop_p, s1.data_ptr(), s2.data_ptr(), ws.data_ptr(), nws, gdt, lib.F32, _stream())
            dx = torch.full(shape, float("nan"), device=dev)
            lib.call("mmh_norm_bwd_apply", gd.data_ptr(), kbp, xd.data_ptr(), md.data_ptr(), isd.data_ptr(), None, s1.data_ptr(),
                     s2.data_ptr(), float(rows), B, rows, C, masked, drop_p, dx.data_ptr(), gdt, lib.F32, lib.F32, _stream())
        _finite(s1, f"s1 {combo}"); _finite(s2, f"s2 {combo}"); _finite(dx, f"dx {combo}")
        E.assert_exact(s1, s1w, f"s1 = sum dz {shape} {combo}")
        assert R.rel_l1(s2, s2w) < GRAD_TOL, (combo, R.rel_l1(s2, s2w))
        assert R.rel_l1(dx, dxw) < GRAD_TOL, (combo, R.rel_l1(dx, dxw))


@pytest.mark.parametrize("relu,drop_p", [(1, 0.5), (1, 0.0), (0, 0.0)], ids=["relu_p0.5", "relu_p0", "plain"])
@pytest.mark.parametrize("shape", [(2, 37, 29, 64), (3, 6, 6, 16)], ids=lambda s: "x".join(map(str, s)))
def test_exact_norm_bwd_rc_sums_in_every_partition(shape, relu, drop_p, dev):
    """mmh_norm_bwd_reduce_rc decides the keep again from the dropout bit and fma(x, scale, shift) > 0: with integer x, scale 1
    and shift 0.5 that expression is exact, so s1 is; s2 and the dx of mmh_norm_bwd_apply_rc within the gradient tolerance"""
    from mmhand_amd import lib
    B, H, W, C = shape
    rows = H * W
    g = E.ints(shape, 41, lo=-3, hi=3)
    x = E.ints(shape, 42, lo=-3, hi=3)
    bit = torch.rand(shape, generator=torch.Generator().manual_seed(43)) < 0.5 if drop_p > 0 else torch.ones(shape, dtype=torch.bool)
    keep = bit & ((x + 0.5 > 0) if relu else torch.ones(shape, dtype=torch.bool))
    mean = x.mean((1, 2))
    invstd = (x.var((1, 2), unbiased=False) + 1e-5).rsqrt()
    dsc = 1.0 / (1.0 - drop_p)
    s1w, s2w, dxw = _bwd_reference(g, keep, dsc, x, mean, invstd, rows)
    assert torch.equal(s1w, s1w.round())
    gd, xd, md, isd = g.to(dev), x.to(dev), mean.to(dev), invstd.to(dev)
    scale, shift = torch.ones((B, C), device=dev), torch.full((B, C), 0.5, device=dev)
    db = _drop_bytes(bit).to(dev) if drop_p > 0 else None
    dbp = db.data_ptr() if db is not None else None
    for combo in COMBOS:
        with _knobs(combo):
            nws = lib.load().mmh_norm_bwd_ws_bytes(B, rows, C)
            ws = torch.full((nws // 4 + 4,), float("nan"), device=dev)
            s1 = torch.full((B, C), 7.0, device=dev); s2 = torch.full((B, C), 7.0, device=dev)
            lib.call("mmh_norm_bwd_reduce_rc", gd.data_ptr(), xd.data_ptr(), md.data_ptr(), isd.data_ptr(), scale.data_ptr(),
                     shift.data_ptr(), dbp, B, rows, C, relu, drop_p, s1.data_ptr(), s2.data_ptr(), ws.data_ptr(), nws, _stream())
            dx = torch.full(shape, float("nan"), device=dev)
            lib.call("mmh_norm_bwd_apply_rc", gd.data_ptr(), xd.data_ptr(), md.data_ptr(), isd.data_ptr(), None, s1.data_ptr(),
                     s2.data_ptr(), scale.data_ptr(), shift.data_ptr(), dbp, float(rows), B, rows, C, relu, drop_p, dx.data_ptr(),
                     _stream())
        _finite(s1, f"s1 {combo}"); _finite(s2, f"s2 {combo}"); _finite(dx, f"dx {combo}")
        E.assert_exact(s1, s1w, f"s1 = sum dz (recomputed keep) {shape} {combo}")
        assert R.rel_l1(s2, s2w) < GRAD_TOL, (combo, R.rel_l1(s2, s2w))
        assert R.rel_l1(dx, dxw) < GRAD_TOL, (combo, R.rel_l1(dx, dxw))


@pytest.mark.parametrize("mode", ["batch", "instance"])
@pytest.mark.parametrize("relu,drop", [(False, False), (True, True)], ids=["plain", "relu_drop"])
@pytest.mark.parametrize("shape", GEOMETRIES, ids=lambda s: "x".join(map(str, s)))
def test_norm_act_fwd_bwd_in_every_partition(shape, relu, drop, mode, dev):
    """mmh_norm_stats, then NormActFn forward and backward against R.norm_act (one oracle per case, shared by the 18
    combinations), as tests/test_pointwise_gpu.py::test_norm_act_fwd_bwd holds the default partition"""
    from mmhand_amd import ops
    B, H, W, C = shape
    x0 = _mk(shape, 1, dev, 2.0, 3.0)
    g0 = _mk((C,), 2, dev, 0.1, 1.0) if mode == "batch" else None
    b0 = _mk((C,), 3, dev, 0.1) if mode == "batch" else None
    mask = (torch.rand(shape, generator=torch.Generator().manual_seed(5)) >= 0.5).to(torch.uint8).to(dev) if drop else None
    dy = _mk(shape, 4, dev)
    xc = x0.cpu().double().requires_grad_(True)
    gc = g0.cpu().double().requires_grad_(True) if g0 is not None else None
    bc = b0.cpu().double().requires_grad_(True) if b0 is not None else None
    ref = R.norm_act(xc, gc, bc, mode, relu, None if mask is None else mask.cpu(), 0.5)
    ref.backward(dy.cpu().double())
    groups = B if mode == "instance" else 1
    xg = xc.detach().reshape(groups, -1, C)
    mean_w, m2_w = xg.mean(1), ((xg - xg.mean(1, keepdim=True)) ** 2).sum(1)
    for combo in COMBOS:
        with _knobs(combo):
            mean, m2, rows = ops.raw_norm_stats(x0, groups)
            x = x0.clone().requires_grad_(True)
            gamma = g0.clone().requires_grad_(True) if g0 is not None else None
            beta = b0.clone().requires_grad_(True) if b0 is not None else None
            rm = torch.zeros(C, device=dev) if mode == "batch" else None
            rv = torch.ones(C, device=dev) if mode == "batch" else None
            out = ops.NormActFn.apply(x, gamma, beta, None, rm, rv, mode, relu, 0.5 if drop else 0.0, 0, mask, None)
            out.backward(dy)
        assert rows == xg.shape[1]
        for t, what in ((mean, "mean"), (m2, "M2"), (out, "out"), (x.grad, "dx")):
            _finite(t, f"{what} {shape} {combo}")
        assert R.rel_l1(mean, mean_w) < TOL and R.rel_l1(m2, m2_w) < TOL, (combo, R.rel_l1(mean, mean_w), R.rel_l1(m2, m2_w))
        assert R.rel_l1(out, ref) < TOL, (combo, R.rel_l1(out, ref))
        assert R.rel_l1(x.grad, xc.grad) < GRAD_TOL, (combo, R.rel_l1(x.grad, xc.grad))
        if mode == "batch":
            gtol = 5e-4 if relu else GRAD_TOL       # as in test_norm_act_fwd_bwd: a ReLU mask bit within fp32 rounding of 0 may flip
            _finite(gamma.grad, f"dgamma {combo}"); _finite(beta.grad, f"dbeta {combo}")
            assert R.rel_l1(gamma.grad, gc.grad) < gtol and R.rel_l1(beta.grad, bc.grad) < gtol, combo
