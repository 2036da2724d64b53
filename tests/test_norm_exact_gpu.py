"""The normalisation kernels of csrc/pointwise.hip against the float64 references of tests/_norm_oracle.py, ELEMENT BY ELEMENT,
through the C-ABI: the two-pass norm backward (mmh_norm_bwd_reduce + _apply, both generations, every storage type), the
recomputed-keep pair (_reduce_rc / _apply_rc), the one-pass plane kernel (mmh_norm_bwd_fused) in each of its geometries,
mmh_norm_bwd_sums_final on both sides of its kernel switch, the PATBlock gate with the norm inside, the sums a dgrad takes
in its epilogue, and the partial statistics the conv epilogues leave.  On the dyadic inputs of the oracle module all of
these are exact - bit for bit, whatever the order of summation.  The statistics (mmh_norm_stats) and the merge kernels
cannot be; they are held per (group, channel) to a bound derived in the oracle module, far below what one dropped row does.
tests/test_norm_exact_cpu.py checks the premises of every case here without a GPU.  Every output starts from NaN: an element
a kernel does not write fails the comparison."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _exact as E
from tests import _norm_oracle as NO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _drop_the_cached_cases():
    yield
    NO.clear_caches()


def _id(s):
    return "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def _abi():
    from mmhand_amd import lib as L
    from mmhand_amd import ops
    return L, ops._ptr, ops._stream


def _nan(shape, dev, dtype="f32"):
    return torch.full(tuple(shape), float("nan"), dtype=NO.DTYPES[dtype], device=dev)


def _to(t, dev, dtype="f32"):
    return t.to(NO.DTYPES[dtype]).to(dev).contiguous()


def _same(got, want64, what):
    """bit for bit; compared on the device, E.assert_exact names the element when they differ"""
    if tuple(got.shape) == tuple(want64.shape) and torch.equal(got.double(), want64.to(got.device)):
        return
    E.assert_exact(got, want64.cpu(), what)


def _bits(t):
    """the bit pattern of every element, with -0 normalised to +0"""
    v = t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    return torch.where(t == 0, torch.zeros_like(v), v)


def _ws(L, groups, rows, C, dev):
    nws = L.load().mmh_norm_bwd_ws_bytes(groups, rows, C)
    return torch.full((nws // 4 + 4,), float("nan"), device=dev), nws


class _Dev:
    """the operands of one dyadic case on the device, in every storage type a test asks for (made once per case)"""

    def __init__(self, P, dev):
        self.P, self.dev, self._t = P, dev, {}
        self.mean, self.invstd, self.gamma = _to(P.mean, dev), _to(P.invstd, dev), _to(P.gamma, dev)
        self.s1w, self.s2w = P.s1.to(dev), P.s2.to(dev)
        self.keep = {0: None, 1: _to(P.out, dev), 2: P.kb.to(dev).contiguous()} if hasattr(P, "out") else None

    def t(self, name, dtype):
        if (name, dtype) not in self._t:
            self._t[name, dtype] = _to(getattr(self.P, name), self.dev, dtype)
        return self._t[name, dtype]

    def want(self, affine, dtype):
        key = ("dx" if affine else "dx_plain", "want", dtype)
        if key not in self._t:
            self._t[key] = NO.stored(getattr(self.P, key[0]), dtype).to(self.dev)
        return self._t[key]


def _two_pass(L, D, masked, types, affine, what):
    """mmh_norm_bwd_reduce + mmh_norm_bwd_apply on the case D holds -> (s1, s2, dx), each checked against float64"""
    _, ptr, stream = _abi()
    P, dev = D.P, D.dev
    gt, xt, dt = types
    g, x = D.t("g", gt), D.t("x", xt)
    keep = D.keep[masked]
    ws, nws = _ws(L, P.groups, P.rows, P.C, dev)
    s1, s2 = _nan((P.groups, P.C), dev), _nan((P.groups, P.C), dev)
    L.call("mmh_norm_bwd_reduce", ptr(g), ptr(keep), ptr(x), ptr(D.mean), ptr(D.invstd), P.groups, P.rows, P.C, masked, P.drop_p,
           ptr(s1), ptr(s2), ptr(ws), nws, NO.CODE[gt], NO.CODE[xt], stream())
    _same(s1, D.s1w, f"s1 = sum dz {what}")
    _same(s2, D.s2w, f"s2 = sum dz xhat {what}")
    dx = _nan(P.g.shape, dev, dt)
    L.call("mmh_norm_bwd_apply", ptr(g), ptr(keep), ptr(x), ptr(D.mean), ptr(D.invstd), ptr(D.gamma if affine else None), ptr(s1),
           ptr(s2), P.count, P.groups, P.rows, P.C, masked, P.drop_p, ptr(dx), NO.CODE[gt], NO.CODE[xt], NO.CODE[dt], stream())
    _same(dx, D.want(affine, dt), f"dx {what}")
    return s1, s2, dx


# ------------------------------------------------------------------------------------------------ two-pass reduce and apply
CASES_2P = [(s, False) for s in NO.TWO_PASS] + [(s, True) for s in NO.TWO_PASS_BATCH]


@pytest.mark.parametrize("masked,drop_p", NO.MASKS, ids=["unmasked", "out_p0.5", "out_p0", "bits_p0.5", "bits_p0"])
@pytest.mark.parametrize("shape,batch", CASES_2P, ids=[_id(s) + ("-batch" if b else "") for s, b in CASES_2P])
def test_two_pass_norm_backward_exact(shape, batch, masked, drop_p, dev):
    """s1, s2 and every element of dx in every storage type, gamma NULL and given, first- and second-generation kernels
    (masked = 1, the fp32 output as the mask, always takes the first generation; so does C / 8 = 12 or 3)"""
    L, _, _ = _abi()
    D = _Dev(NO.two_pass_case(shape, masked, drop_p, batch), dev)
    for v2 in (0, 1):
        with E.option("pw_v2", v2):
            for types in NO.TYPES:
                for affine in (False, True):
                    _two_pass(L, D, masked, types, affine, f"{shape} batch={batch} masked={masked} p={drop_p} pw_v2={v2} {types} gamma={affine}")


# ------------------------------------------------------------------------------------------------ recomputed keep
@pytest.mark.parametrize("relu,drop_p", NO.RC_MODES, ids=["relu_p0.5", "relu_p0", "plain"])
@pytest.mark.parametrize("shape", NO.RC_SHAPES, ids=_id)
def test_recomputed_keep_norm_backward_exact(shape, relu, drop_p, dev):
    """mmh_norm_bwd_reduce_rc / _apply_rc: the keep decided again from the dropout bit array and fma(x, scale, shift) > 0"""
    L, ptr, stream = _abi()
    P = NO.rc_case(shape, relu, drop_p)
    D = _Dev(P, dev)
    g, x, scale, shift = D.t("g", "f32"), D.t("x", "f32"), _to(P.scale, dev), _to(P.shift, dev)
    db = P.db.to(dev).contiguous() if drop_p > 0 else None
    ws, nws = _ws(L, P.groups, P.rows, P.C, dev)
    s1, s2 = _nan((P.groups, P.C), dev), _nan((P.groups, P.C), dev)
    L.call("mmh_norm_bwd_reduce_rc", ptr(g), ptr(x), ptr(D.mean), ptr(D.invstd), ptr(scale), ptr(shift), ptr(db), P.groups, P.rows,
           P.C, relu, drop_p, ptr(s1), ptr(s2), ptr(ws), nws, stream())
    _same(s1, D.s1w, f"rc s1 {shape}")
    _same(s2, D.s2w, f"rc s2 {shape}")
    for affine in (False, True):
        dx = _nan(P.g.shape, dev)
        L.call("mmh_norm_bwd_apply_rc", ptr(g), ptr(x), ptr(D.mean), ptr(D.invstd), ptr(D.gamma if affine else None), ptr(s1), ptr(s2),
               ptr(scale), ptr(shift), ptr(db), P.count, P.groups, P.rows, P.C, relu, drop_p, ptr(dx), stream())
        _same(dx, D.want(affine, "f32"), f"rc dx {shape} gamma={affine}")


# ------------------------------------------------------------------------------------------------ one pass
@pytest.mark.parametrize("lp", ["bf16", "fp16"])
@pytest.mark.parametrize("case", NO.PLANE, ids=lambda c: _id(c[0]) + "-" + c[1])
def test_one_pass_norm_backward_exact(case, lp, dev):
    """mmh_norm_bwd_fused in the geometry the case list names (tests/test_norm_exact_cpu.py asserts each lpr_log2 and tail):
    s1, s2 and dx exact, for dx32 / dx16, masked or not, gamma NULL and given - and element for element the two-pass result,
    bit for bit up to the sign of an exact zero, which on these inputs is exact too (tests/test_norm_bwd_plane_gpu.py holds realistic values to rounding)"""
    L, ptr, stream = _abi()
    shape, gk, _, _ = case
    gt = "f32" if gk == "f32" else lp
    for dx16, masked in NO.PLANE_VARIANTS:
        P = NO.plane_case(shape, masked)
        D = _Dev(P, dev)
        mk, dt = (2 if masked else 0), (lp if dx16 else "f32")
        assert L.load().mmh_norm_bwd_fused_supported(P.groups, P.rows, P.C, mk, NO.CODE[gt], NO.CODE[lp]) == 1
        g, x, keep = D.t("g", gt), D.t("x", lp), D.keep[mk]
        for affine in (False, True):
            what = f"{shape} g={gt} x={lp} dx={dt} masked={masked} gamma={affine}"
            f1, f2 = _nan((P.groups, P.C), dev), _nan((P.groups, P.C), dev)
            dx = _nan(P.g.shape, dev, dt)
            L.call("mmh_norm_bwd_fused", ptr(g), ptr(keep), ptr(x), ptr(D.mean), ptr(D.invstd), ptr(D.gamma if affine else None),
                   P.count, P.groups, P.rows, P.C, mk, P.drop_p, ptr(f1), ptr(f2), ptr(dx), NO.CODE[gt], NO.CODE[lp], NO.CODE[dt],
                   stream())
            _same(f1, D.s1w, f"fused s1 {what}")
            _same(f2, D.s2w, f"fused s2 {what}")
            _same(dx, D.want(affine, dt), f"fused dx {what}")
            s1, s2, dx2 = _two_pass(L, D, mk, (gt, lp, dt), affine, "two-pass " + what)
            # the two kernels agree bit for bit once -0 is read as +0: an exact zero may carry either sign - fma(k0, 0, -0)
            # against fma(k0, 0, fma(-0, x, 0)) - which is the one difference two exact results can have
            for a, b in ((f1, s1), (f2, s2), (dx, dx2)):
                assert torch.equal(_bits(a), _bits(b)), what


# ------------------------------------------------------------------------------------------------ production count
@pytest.mark.parametrize("shape", NO.PROD, ids=_id)
def test_norm_backward_with_count_equal_rows_within_eight_roundings(shape, dev, capsys):
    """count = rows, as the training step passes it: (float)(1.0 / rows) is inexact and so is dx.  The sums stay exact; dx per
    element within 8 u (|k0 dz| + |k0 k1| + |(x - mu) k2|) plus half an ulp of the storage type (tests/_norm_oracle.py:
    prod_bound gives the count of the eight roundings) for both generations of the two-pass kernels, whose arithmetic
    (norm_bwd_elem, norm_bwd_apply_kernel) that count describes.

    The one-pass kernel regroups dx = fma(k0, dz, fma(-k2, x, c)) with c = fma(mu, k2, -(k0 k1)) rounded once per channel: an
    error of u |mu k2| that does not shrink where x is close to the mean.  Measured against the 8 u bound alone it is
    26.5 x (1073 x 64) and 30.8 x (2025 x 32) over it, at elements with dz = 0 and x = mu, where that bound is a few u |k0 k1|.
    Its own count: k0 dz 1 rounding, k0 k1 6 (inv_count, s1 inv_count, the product, c, the inner and the outer fma),
    (x - mu) k2 5 (three for k2, both fmas) - all within the 8 - plus ONE of size u |mu k2| (1 + 4 u) for c.  The one-pass
    result is held to the 8 u bound plus that term; the ratio to the 8 u bound alone is printed."""
    L, ptr, stream = _abi()
    worst = {}
    for masked in (False, True):
        P = NO.prod_case(shape, masked)
        D = _Dev(P, dev)
        mk = 2 if masked else 0
        for gt, xt, dt in (("f32", "bf16", "f32"), ("bf16", "bf16", "bf16"), ("fp16", "fp16", "fp16"), ("f32", "f32", "f32")):
            g, x, keep = D.t("g", gt), D.t("x", xt), D.keep[mk]
            for affine in (False, True):
                want, allow = NO.prod_bound(P, P.gamma if affine else None, dt)
                want, allow = want.to(dev), allow.to(dev)
                gm = ptr(D.gamma if affine else None)

                muk2 = NO.U32 * (1 + 4 * NO.U32) * NO.prod_mu_k2(P, P.gamma if affine else None).to(dev)

                def check(dx, kernel, extra=None):
                    kernel += " dx32" if dt == "f32" else " dx16"
                    err = (dx.double() - want).abs()
                    pos = allow > 0
                    if extra is not None:
                        worst[kernel + " (against 8 u alone)"] = max(worst.get(kernel + " (against 8 u alone)", 0.0), float((err[pos] / allow[pos]).max()))
                    allow_ = allow if extra is None else allow + extra
                    r = float((err[pos] / allow_[pos]).max())
                    worst[kernel] = max(worst.get(kernel, 0.0), r)
                    bad = ~(err <= allow_)
                    assert not bool(bad.any()), (f"{kernel} {shape} masked={masked} {gt, xt, dt} gamma={affine}: {int(bad.sum())} elements out of "
                                                 f"bound, worst |got - want| / bound = {r:.3f}, first at {tuple(int(i) for i in bad.nonzero()[0])}")
                for v2 in (0, 1):
                    with E.option("pw_v2", v2):
                        ws, nws = _ws(L, P.groups, P.rows, P.C, dev)
                        s1, s2 = _nan((P.groups, P.C), dev), _nan((P.groups, P.C), dev)
                        L.call("mmh_norm_bwd_reduce", ptr(g), ptr(keep), ptr(x), ptr(D.mean), ptr(D.invstd), P.groups, P.rows, P.C, mk,
                               P.drop_p, ptr(s1), ptr(s2), ptr(ws), nws, NO.CODE[gt], NO.CODE[xt], stream())
                        _same(s1, D.s1w, "s1"); _same(s2, D.s2w, "s2")
                        dx = _nan(P.g.shape, dev, dt)
                        L.call("mmh_norm_bwd_apply", ptr(g), ptr(keep), ptr(x), ptr(D.mean), ptr(D.invstd), gm, ptr(s1), ptr(s2), P.count,
                               P.groups, P.rows, P.C, mk, P.drop_p, ptr(dx), NO.CODE[gt], NO.CODE[xt], NO.CODE[dt], stream())
                        check(dx, f"two-pass pw_v2={v2}")
                if xt != "f32" and L.load().mmh_norm_bwd_fused_supported(P.groups, P.rows, P.C, mk, NO.CODE[gt], NO.CODE[xt]) == 1:
                    f1, f2 = _nan((P.groups, P.C), dev), _nan((P.groups, P.C), dev)
                    dx = _nan(P.g.shape, dev, dt)
                    L.call("mmh_norm_bwd_fused", ptr(g), ptr(keep), ptr(x), ptr(D.mean), ptr(D.invstd), gm, P.count, P.groups, P.rows,
                           P.C, mk, P.drop_p, ptr(f1), ptr(f2), ptr(dx), NO.CODE[gt], NO.CODE[xt], NO.CODE[dt], stream())
                    _same(f1, D.s1w, "fused s1"); _same(f2, D.s2w, "fused s2")
                    check(dx, "one-pass", muk2)
    with capsys.disabled():
        print(f"\n[count = rows] {shape}: worst |got - want| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


# ------------------------------------------------------------------------------------------------ mmh_norm_bwd_sums_final
@pytest.mark.parametrize("chunks", NO.SUMS_FINAL_CHUNKS)
def test_sums_final_exact(chunks, dev):
    """col_reduce_final<8> below 256 chunks and <32> from there, on both sides of each kernel's 4-way unrolled loop; 40 channels:
    the last work-group of 32 is part-filled"""
    L, ptr, stream = _abi()
    P = NO.sums_final_case(chunks)
    part = _to(P.part, dev)
    s1, s2 = _nan((NO.SUMS_FINAL_GROUPS, NO.SUMS_FINAL_C), dev), _nan((NO.SUMS_FINAL_GROUPS, NO.SUMS_FINAL_C), dev)
    L.call("mmh_norm_bwd_sums_final", ptr(part), NO.SUMS_FINAL_GROUPS, NO.SUMS_FINAL_C, chunks, ptr(s1), ptr(s2), stream())
    _same(s1, P.s1, f"sums_final s1 chunks={chunks}")
    _same(s2, P.s2, f"sums_final s2 chunks={chunks}")


# ------------------------------------------------------------------------------------------------ the gate with the norm inside
@pytest.mark.parametrize("types", NO.GATE_TYPES, ids=lambda t: "-".join(t))
@pytest.mark.parametrize("shape", NO.GATE, ids=_id)
def test_gate_norm_exact(shape, types, dev):
    """mmh_patblock_gate_norm_fwd: out, x2n, x3n; mmh_patblock_gate_norm_bwd: g_x1, g_s1, g_s2, g_s3, sum1, sum2 with each of
    g_out / g_x2n / g_x3n NULL in turn; and sum1, sum2 bit for bit what mmh_norm_bwd_reduce gives for that g_s1 and y2"""
    L, ptr, stream = _abi()
    yt, st, ct = types
    P = NO.gate_case(shape)
    G, rows, C = P.groups, P.rows, P.C
    assert L.load().mmh_patblock_gate_norm_supported(G, rows, C) == 1
    x1, y2, scale, shift = _to(P.x1, dev), _to(P.y2, dev, yt), _to(P.scale, dev), _to(P.shift, dev)
    zero = _to(P.zero, dev, st)
    mean, invstd = _to(P.mean, dev), _to(P.invstd, dev)

    def fwd(y2_, shift_, s2_, s3_):
        out, x2n, x3n = _nan((G, rows, C), dev), _nan((G, rows, 2 * C), dev, ct), _nan((G, rows, 2 * C), dev, ct)
        L.call("mmh_patblock_gate_norm_fwd", ptr(x1), ptr(y2_), ptr(scale), ptr(shift_), ptr(s2_), ptr(s3_), ptr(out), ptr(x2n), ptr(x3n),
               G, rows, C, NO.CODE[yt], NO.CODE[ct], NO.CODE[st], stream())
        return out, x2n, x3n
    out, x2n, x3n = fwd(y2, shift, zero, zero)
    _same(out, P.out, f"gate_norm_fwd out {shape} {types}")
    _same(x2n, NO.stored(P.cat, ct), f"gate_norm_fwd x2n {shape} {types}")
    _same(x3n, NO.stored(P.cat, ct), f"gate_norm_fwd x3n {shape} {types}")
    # where s2 and s3 are COPIED: y2 = 0 and shift = 0 make s1 = 0 and out = x1 whatever the gates are
    out, x2n, x3n = fwd(torch.zeros_like(y2), torch.zeros_like(shift), _to(P.s2r, dev, st), _to(P.s3r, dev, st))
    _same(out, P.x1.double(), f"gate_norm_fwd routing out {shape} {types}")
    _same(x2n, NO.stored(torch.cat([P.s3r.double(), P.x1.double()], -1), ct), f"gate_norm_fwd x2n = cat(s3, out) {shape} {types}")
    _same(x3n, NO.stored(torch.cat([P.s2r.double(), P.x1.double()], -1), ct), f"gate_norm_fwd x3n = cat(s2, out) {shape} {types}")
    out_only = _nan((G, rows, C), dev)
    L.call("mmh_patblock_gate_norm_fwd", ptr(x1), ptr(y2), ptr(scale), ptr(shift), ptr(zero), ptr(zero), ptr(out_only), None, None,
           G, rows, C, NO.CODE[yt], NO.CODE[ct], NO.CODE[st], stream())
    _same(out_only, P.out, f"gate_norm_fwd out alone {shape} {types}")

    g_out, g_x2n, g_x3n = _to(P.g_out, dev), _to(P.g_x2n, dev, ct), _to(P.g_x3n, dev, ct)
    for has in NO.GATE_ABSENT:
        Rf = NO.gate_bwd_ref(P, *has)
        what = f"{shape} {types} present={has}"
        g_x1, g_s1 = _nan((G, rows, C), dev), _nan((G, rows, C), dev)
        g_s2, g_s3 = _nan((G, rows, C), dev, st), _nan((G, rows, C), dev, st)
        sum1, sum2 = _nan((G, C), dev), _nan((G, C), dev)
        ws, nws = _ws(L, G, rows, C, dev)
        L.call("mmh_patblock_gate_norm_bwd", ptr(g_out if has[0] else None), ptr(g_x2n if has[1] else None),
               ptr(g_x3n if has[2] else None), ptr(y2), ptr(scale), ptr(shift), ptr(mean), ptr(invstd), ptr(zero), ptr(zero), ptr(g_x1),
               ptr(g_s1), ptr(g_s2), ptr(g_s3), ptr(sum1), ptr(sum2), ptr(ws), nws, G, rows, C, NO.CODE[yt], NO.CODE[ct], NO.CODE[st],
               stream())
        _same(g_x1, Rf.g_x1, f"gate_norm_bwd g_x1 {what}")
        _same(g_s1, Rf.g_s1, f"gate_norm_bwd g_s1 {what}")
        _same(g_s2, NO.stored(Rf.g_s2, st), f"gate_norm_bwd g_s2 {what}")
        _same(g_s3, NO.stored(Rf.g_s3, st), f"gate_norm_bwd g_s3 {what}")
        _same(sum1, Rf.sum1, f"gate_norm_bwd sum1 {what}")
        _same(sum2, Rf.sum2, f"gate_norm_bwd sum2 {what}")
        r1, r2 = _nan((G, C), dev), _nan((G, C), dev)
        ws, nws = _ws(L, G, rows, C, dev)
        L.call("mmh_norm_bwd_reduce", ptr(g_s1), None, ptr(y2), ptr(mean), ptr(invstd), G, rows, C, 0, 0.0, ptr(r1), ptr(r2), ptr(ws), nws,
               NO.CODE["f32"], NO.CODE[yt], stream())
        assert torch.equal(sum1, r1) and torch.equal(sum2, r2), what


# ------------------------------------------------------------------------------------------------ statistics
def _stats_call(L, x, groups, rows, C, cs, dtype, dev):
    _, ptr, stream = _abi()
    nws = L.load().mmh_norm_stats_ws_bytes(groups, rows, C)
    ws = torch.full((nws // 4 + 4,), float("nan"), device=dev)
    mean, m2 = _nan((groups, C), dev), _nan((groups, C), dev)
    L.call("mmh_norm_stats", ptr(x), groups, rows, C, cs, ptr(mean), ptr(m2), ptr(ws), nws, NO.CODE[dtype], stream())
    return mean, m2


@pytest.mark.parametrize("dtype", ["f32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", NO.STATS_SHAPES, ids=_id)
def test_norm_stats_within_the_derived_bound(shape, dtype, dev, capsys):
    """mmh_norm_stats (norm_stats_partial and _v2): mean and M2 per (group, channel) against float64, under the bound derived in
    tests/_norm_oracle.py (section 4) - at most 1/8 of what dropping the first or the last row of the group would do"""
    L, _, _ = _abi()
    B, H, W, C = shape
    rows = H * W
    P = NO.stats_case(B, rows, C, dtype)
    x = P.x.to(dev).contiguous()
    worst = []
    for v2 in (0, 1):
        with E.option("pw_v2", v2):
            mean, m2 = _stats_call(L, x, B, rows, C, C, dtype, dev)
        rm, rq = NO.stats_ratio(mean, m2, P, NO.stats_merges(rows, C, bool(v2) and NO.row_geom_ok(C)))
        worst.append((v2, rm, rq))
        assert rm <= NO.STATS_FINDING and rq <= NO.STATS_FINDING, (shape, dtype, v2, rm, rq)
    with capsys.disabled():
        print(f"\n[stats bound] {shape} {dtype}: got / bound " + ", ".join(f"pw_v2={v} mean {a:.4f} M2 {b:.4f}" for v, a, b in worst))


def test_norm_stats_of_a_strided_matrix_within_the_derived_bound(dev, capsys):
    """cs = 96 > C = 64: the first-generation kernel takes the stride; the 32 columns it must not read hold NaN"""
    L, _, _ = _abi()
    rows, C, cs = NO.STATS_STRIDED
    P = NO.stats_case(1, rows, C)
    wide = torch.full((rows, cs), float("nan"))
    wide[:, :C] = P.x[0]
    for v2 in (0, 1):
        with E.option("pw_v2", v2):
            mean, m2 = _stats_call(L, wide.to(dev), 1, rows, C, cs, "f32", dev)
        rm, rq = NO.stats_ratio(mean, m2, P, NO.stats_merges(rows, C, False))
        with capsys.disabled():
            print(f"\n[stats bound] strided {NO.STATS_STRIDED} pw_v2={v2}: got / bound mean {rm:.4f} M2 {rq:.4f}")
        assert rm <= NO.STATS_FINDING and rq <= NO.STATS_FINDING, (v2, rm, rq)


# ------------------------------------------------------------------------------------------------ the merge kernels
MERGE2_SUB = {1: 1, 3: 3, 9: 3, 57: 19, 64: 8, 65: 5}


def _within_ulps(got, want64, n, what):
    u = NO.ulps(got, want64)
    assert bool(torch.isfinite(got).all()) and float(u.max()) <= n, f"{what}: {float(u.max()):.2f} ulps (allowed {n})"


@pytest.mark.parametrize("chunks", NO.MERGE_CHUNKS)
def test_merge_kernels_with_empty_partials(chunks, dev):
    """mmh_norm_stats_merge, _merge2, _merge_finalize and mmh_syncbn_merge_finalize with fewer partials than chunk lanes, an empty
    FIRST partial and a chunk lane whose partials are all empty: mean / M2 within 2 fp32 ulps of float64 (the merge runs in
    double), scale / shift / invstd and the running statistics within 4 ulps of the float64 formula on the RETURNED mean / M2"""
    L, ptr, stream = _abi()
    P = NO.merge_case(chunks)
    G, C = NO.MERGE_GROUPS, NO.MERGE_C
    part = P.part.to(dev)
    eps = NO.MERGE_EPS
    mean, m2 = _nan((G, C), dev), _nan((G, C), dev)
    L.call("mmh_norm_stats_merge", ptr(part), G, chunks, C, ptr(mean), ptr(m2), stream())
    _within_ulps(mean, P.mean, 2, f"merge mean chunks={chunks}")
    _within_ulps(m2, P.m2, 2, f"merge M2 chunks={chunks}")

    sub = MERGE2_SUB[chunks]
    one = part[0].contiguous()
    ws = torch.full((L.load().mmh_norm_stats_merge2_ws_bytes(sub, C) // 4,), float("nan"), device=dev)
    mean2, m22 = _nan((1, C), dev), _nan((1, C), dev)
    L.call("mmh_norm_stats_merge2", ptr(one), chunks, C, sub, ptr(ws), ws.numel() * 4, ptr(mean2), ptr(m22), stream())
    _within_ulps(mean2[0], P.mean[0], 2, f"merge2 mean chunks={chunks} sub={sub}")
    _within_ulps(m22[0], P.m2[0], 2, f"merge2 M2 chunks={chunks} sub={sub}")

    outs = [_nan((G, C), dev) for _ in range(5)]
    L.call("mmh_norm_stats_merge_finalize", ptr(part), G, chunks, C, P.count, eps, *[ptr(o) for o in outs], stream())
    mean, m2, scale, shift, invstd = outs
    _within_ulps(mean, P.mean, 2, f"merge_finalize mean chunks={chunks}")
    _within_ulps(m2, P.m2, 2, f"merge_finalize M2 chunks={chunks}")
    sc_w, sh_w, is_w = NO.finalize_ref(mean.cpu(), m2.cpu(), P.count, eps)
    _within_ulps(invstd, is_w, 4, f"merge_finalize invstd chunks={chunks}")
    _within_ulps(scale, sc_w, 4, f"merge_finalize scale chunks={chunks}")
    _within_ulps(shift, sh_w, 4, f"merge_finalize shift chunks={chunks}")

    # SyncBN: one group, the ranks' triples at a column offset of wider rows; gamma > 0 and beta < 0 (mean > 0: no cancellation
    # in shift = beta - mean scale, whose error in ulps would otherwise have no bound)
    off, other = 3 * 8, 3 * 16
    stride = off + 3 * C + other
    buf = torch.full((chunks, stride), float("nan"))
    buf[:, off:off + 3 * C] = P.part[0].reshape(chunks, 3 * C)
    buf = buf.to(dev)
    gen = torch.Generator().manual_seed(chunks)
    gamma, beta = 0.5 + torch.rand(C, generator=gen), -0.1 - torch.rand(C, generator=gen)
    rm0, rv0 = 0.5 + torch.rand(C, generator=gen), 1.0 + torch.rand(C, generator=gen)
    rm, rv, gamma_d, beta_d = rm0.to(dev), rv0.to(dev), gamma.to(dev), beta.to(dev)
    outs = [_nan((1, C), dev) for _ in range(5)]
    L.call("mmh_syncbn_merge_finalize", ctypes.c_void_p(buf.data_ptr() + 4 * off), chunks, stride, C, P.count, eps, ptr(gamma_d),
           ptr(beta_d), *[ptr(o) for o in outs], ptr(rm), ptr(rv), NO.MERGE_MOMENTUM, stream())
    mean, m2, scale, shift, invstd = [o[0] for o in outs]
    _within_ulps(mean, P.mean[0], 2, f"syncbn mean ranks={chunks}")
    _within_ulps(m2, P.m2[0], 2, f"syncbn M2 ranks={chunks}")
    sc_w, sh_w, is_w = NO.finalize_ref(mean.cpu(), m2.cpu(), P.count, eps, gamma, beta)
    _within_ulps(invstd, is_w, 4, f"syncbn invstd ranks={chunks}")
    _within_ulps(scale, sc_w, 4, f"syncbn scale ranks={chunks}")
    _within_ulps(shift, sh_w, 4, f"syncbn shift ranks={chunks}")
    mom = float(np.float32(NO.MERGE_MOMENTUM))
    unb = m2.cpu().double() / (P.count - 1.0)
    _within_ulps(rm, (1.0 - mom) * rm0.double() + mom * mean.cpu().double(), 4, f"syncbn running mean ranks={chunks}")
    _within_ulps(rv, (1.0 - mom) * rv0.double() + mom * unb, 4, f"syncbn running var ranks={chunks}")


# ------------------------------------------------------------------------------------------------ conv epilogues
LPARG = {"bf16": True, "fp16": 2}       # the `bf16` argument of the ops wrappers


@pytest.mark.parametrize("lp", ["bf16", "fp16"])
@pytest.mark.parametrize("case", NO.NBR, ids=lambda c: _id(c[0]) + ("-reflect" if c[1] else "-zero") + ("-batch" if c[2] else ""))
def test_dgrad_epilogue_sums_exact(case, lp, dev):
    """mmh_conv3x3_lp16_dgrad_nbr on an integer problem: dx bit-identical to the plain dgrad (and to the oracle), s1 and s2 of
    the norm whose output gradient dx is exact against float64 of the stored dx - and the same sums again through
    mmh_norm_bwd_sums_final from the raw workspace the epilogue wrote"""
    from mmhand_amd import ops
    L, ptr, stream = _abi()
    (B, H, W, Cin, Cout), reflect, batch, masked, drop_p = case
    P = NO.nbr_case(case)
    mode = 2 if reflect else 1
    d = ops.conv_desc(B, H, W, Cin, Cout, 3, 1, 1, reflect)
    d.dtype = NO.CODE[lp]
    cpi = L.load().mmh_conv3x3_lp16_dgrad_nbr_chunks(ctypes.byref(d), mode)
    assert cpi > 0, "the epilogue form is not available for this shape"
    w = P.conv.w.to(dev)
    dy16 = _to(P.conv.dy, dev, lp)
    ops.bump_weights_epoch()
    plain = ops.raw_conv3x3_lp16(dy16, w, None, reflect, L.ACT_NONE, LPARG[lp], mode, out16=True)
    E.assert_exact(plain, P.conv.dx, "plain dgrad")
    wp, _ = ops.bf16_weights(w, LPARG[lp])
    xn = _to(P.x.reshape(B, H, W, Cin), dev, lp)
    bits = P.kb.reshape(B, H, W, Cin // 4).to(dev).contiguous() if masked else None
    mean, invstd = _to(P.mean, dev), _to(P.invstd, dev)
    s1, s2 = _nan((P.groups, Cin), dev), _nan((P.groups, Cin), dev)
    ws = _nan((B * cpi * 2 * Cin + 4,), dev)
    dx = _nan((B, H, W, Cin), dev, lp)
    L.call("mmh_conv3x3_lp16_dgrad_nbr", ctypes.byref(d), mode, ptr(dy16), ptr(wp), ptr(dx), ptr(xn), ptr(bits), ptr(mean), ptr(invstd),
           P.groups, drop_p, ptr(s1), ptr(s2), ptr(ws), B * cpi * 2 * Cin * 4, ptr(ops.zero_page(dx.device)), stream())
    assert torch.equal(dx.view(torch.int16), plain.view(torch.int16))
    _same(s1, P.s1, f"dgrad_nbr s1 {case} {lp}")
    _same(s2, P.s2, f"dgrad_nbr s2 {case} {lp}")
    r1, r2 = _nan((P.groups, Cin), dev), _nan((P.groups, Cin), dev)
    L.call("mmh_norm_bwd_sums_final", ptr(ws), P.groups, Cin, cpi * B // P.groups, ptr(r1), ptr(r2), stream())
    _same(r1, P.s1, f"sums_final of the epilogue's partials, s1 {case} {lp}")
    _same(r2, P.s2, f"sums_final of the epilogue's partials, s2 {case} {lp}")


@pytest.mark.parametrize("lp", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", sorted(NO.EPI_STATS))
def test_epilogue_statistics_partials_exact(kind, lp, dev, monkeypatch):
    """mmh_conv3x3_lp16_fprop_stats (halo), mmh_conv_lp16_fprop_stats (s2), mmh_conv_stem16_stats (stem) on integer problems
    with |y| <= 16: every partial (n, mean, M2) is exact, so per (image, channel), with no knowledge of which pixels a partial
    covers: sum n == rows, sum n mean == sum y, sum (M2 + n mean^2) == sum y^2 - in float64 from the raw partials, with ==.
    The two fp32 epilogues (mmh_conv2d_fprop_stats, mmh_wino_output) are not run here: their partials cover ragged counts
    (1 / n is not dyadic), so they cannot be exact and belong under the statistics bound; tests/test_norm_fusion_gpu.py and
    tests/test_conv_gpu.py hold them to float64 at 2e-6 / 2e-5.  The kernels are reached through the ops wrappers, which own
    the weight layouts and padded inputs each of them wants; the partials are read where the wrappers park them."""
    from mmhand_amd import ops
    L, _, _ = _abi()
    spec, _ = NO.EPI_STATS[kind]
    B, H, W, Cin, Cout, k, stride, pad, refl = spec
    P = NO.epi_problem(kind)
    x, w, bias = P.x.to(dev), P.w.to(dev), P.bias.to(dev)
    monkeypatch.setattr(ops, "FUSE_NORM_STATS", True)
    monkeypatch.setattr(ops, "FUSE_NORM_STATS_NARROW", True)
    ops.bump_weights_epoch()
    calls = {}
    orig = L.call

    def spy(name, *a):
        calls[name] = calls.get(name, 0) + 1
        return orig(name, *a)
    monkeypatch.setattr(L, "call", spy)
    d = ops.conv_desc(B, H, W, Cin, Cout, k, stride, pad, refl)
    if kind == "halo":
        y = ops.raw_conv3x3_lp16(ops.lp16_twin(x, LPARG[lp]), w, bias, refl, 0, LPARG[lp], 0, out16=True, want_stats=True)
        entry = "mmh_conv3x3_lp16_fprop_stats"
    elif kind == "s2":
        y = ops.raw_conv_lp16g(d, 0, ops.lp16_twin(x, LPARG[lp]), w, bias, 0, LPARG[lp], out16=True, want_stats=True)
        entry = "mmh_conv_lp16_fprop_stats"
    else:
        y = ops.raw_conv_lp16_flat(d, x, w, bias, 0, LPARG[lp], out16=True, want_stats=True)
        entry = "mmh_conv_stem16_stats"
    assert calls.get(entry) == 1, calls
    pend = ops._take_stats(y)                   # this test's own entry, nothing else
    assert pend is not None, "the kernel left no partial statistics"
    stats = pend[0].double().cpu()
    E.assert_exact(y, P.y, f"{entry} y")
    assert stats.shape[0] == B and stats.shape[2] == 3 and stats.shape[3] == Cout and bool(torch.isfinite(stats).all())
    n, mean, m2 = stats[:, :, 0], stats[:, :, 1], stats[:, :, 2]
    yd = P.y.reshape(B, -1, Cout)
    rows = yd.shape[1]
    assert torch.equal(n.sum(1), torch.full((B, Cout), float(rows), dtype=torch.float64)), "sum n != rows"
    E.assert_exact((n * mean).sum(1), yd.sum(1), f"{entry}: sum n mean == sum y")
    E.assert_exact((m2 + n * mean * mean).sum(1), (yd * yd).sum(1), f"{entry}: sum (M2 + n mean^2) == sum y^2")
