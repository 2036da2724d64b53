"""Exact problems for the normalisation kernels of csrc/pointwise.hip and their float64 references (plain module, no fixtures).

The dyadic design.  tests/_exact.py makes convolutions exact with small integers; the norm backward also MULTIPLIES by
per-channel coefficients, so everything that multiplies is a power of two here:

    g in -3 .. 3, keep mask of density 0.6, drop_p in {0, 0.5} (dsc = 1 / (1 - drop_p) in {1, 2}), x in -8 .. 8 (exact in bf16
    and fp16), mean[g][c] in -2 .. 2, invstd[g][c] in {1/4, 1/2, 1, 2}, gamma[c] in {-1, 1/2, 1, 2} or NULL, and
    count = the next power of two >= rows (a separate argument of the entry points: SyncBN passes it larger than rows).

The backward kernels take mean / invstd as inputs, so they need not be the statistics of x.  With these inputs dz, xhat,
every term dz * xhat, every partial sum, k0 = gamma invstd, k1 = s1 / count, k2 = k0 invstd s2 / count and all three
forms of dx in the code (norm_bwd_elem; norm_bwd_apply_kernel's gm is (gv - a1 ic - (x - mu) is a2 ic); the plane
kernel's fma(k0, dz, fma(-k2, x, c))) are small dyadic rationals: any summation order, any chunking and any FMA
contraction gives the same fp32 result, and a 16-bit dx is the single round-to-nearest-even of an exact fp32 value -
want = float64 dx -> .float() -> .to(bf16 | fp16) compares bit for bit.

The conditions that make this true are asserted on the reference alone (check_any_order, check_forms;
tests/test_norm_exact_cpu.py runs them over every case list here).  A case that fails gets smaller ranges, never a looser
check.

The statistics (mmh_norm_stats) cannot be exact - 1 / n and Chan's nb / nt are not dyadic for ragged counts: section 4
derives a bound per (group, channel) from the kernels' operation count."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from tests import _exact as E

TPB, UNR = 256, 4
COL_CHUNKS, ROW_CHUNKS = 2048, 4096         # the defaults of mmh_set_option("col_chunks" | "row_chunks")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CODE = {"f32": 0, "bf16": 1, "fp16": 2}     # MMH_F32 | MMH_BF16 | MMH_FP16
MIN_INVSTD = 0.25
_INVSTD = torch.tensor([0.25, 0.5, 1.0, 2.0])
_GAMMA = torch.tensor([-1.0, 0.5, 1.0, 2.0])

_CACHES = []


def _cached(fn):
    """one entry per case, computed once and shared (read-only!) by the tests of a module, which drops them at teardown"""
    fn = functools.lru_cache(maxsize=None)(fn)
    _CACHES.append(fn)
    return fn


def clear_caches():
    for fn in _CACHES:
        fn.cache_clear()


def keep_bytes(keep):
    """bool [.., C] -> uint8 [.., C / 4]: bit e of a byte = lane e of its float4 (the layout mmh_scale_shift_act writes)"""
    k = keep.reshape(*keep.shape[:-1], keep.shape[-1] // 4, 4).to(torch.uint8)
    return k[..., 0] | (k[..., 1] << 1) | (k[..., 2] << 2) | (k[..., 3] << 3)


def drop_bytes(keep):
    """bool [.., C] -> uint8 [.., C / 8]: one bit per element (the layout of mmh_dropout_bits)"""
    k = keep.reshape(*keep.shape[:-1], keep.shape[-1] // 8, 8).to(torch.uint8)
    out = torch.zeros(k.shape[:-1], dtype=torch.uint8)
    for e in range(8):
        out |= k[..., e] << e
    return out


def next_pow2(n):
    return 1 << max(0, int(n) - 1).bit_length()


def is_f32(t64):
    """every value of a float64 tensor equals its own float32 round trip"""
    return bool(torch.equal(t64.float().double(), t64))


def stored(t64, dtype):
    """what a correct kernel leaves in a tensor of `dtype`: the float64 reference (exact in fp32), rounded ONCE"""
    return t64.float().to(DTYPES[dtype]).double()


# ------------------------------------------------------------------------------------------------ 1. the norm backward
def norm_bwd_ref(g, keep, dsc, x, mean, invstd, gamma, count):
    """float64 (dz, s1, s2, dx) of a norm backward; g, keep, x: [groups][rows][C], mean / invstd: [groups][C], gamma [C] | None
    dx = gamma invstd (dz - s1 / count - xhat s2 / count), xhat = (x - mean) invstd"""
    dz = g.double() * keep.double() * dsc
    mu, is_ = mean.double()[:, None, :], invstd.double()[:, None, :]
    xhat = (x.double() - mu) * is_
    s1, s2 = dz.sum(1), (dz * xhat).sum(1)
    gm = gamma.double()[None, None, :] if gamma is not None else 1.0
    dx = gm * is_ * (dz - s1[:, None, :] / count - xhat * s2[:, None, :] / count)
    return dz, s1, s2, dx


def check_any_order(dz, x, mean, invstd, what):
    """per (group, channel): sum |dz * xhat| / min(invstd) and sum |dz| are below 2^24.  Every term is a multiple of
    min(invstd) (dz and x - mean are integers), so every partial sum of any subset in any order is such a multiple below
    2^24 min(invstd): exactly representable in fp32."""
    xhat = (x.double() - mean.double()[:, None, :]) * invstd.double()[:, None, :]
    assert float(invstd.min()) >= MIN_INVSTD and is_f32(dz) and torch.equal(dz, dz.round()) and torch.equal(x.double(), x.double().round())
    t = (dz * xhat).abs().sum(1) / MIN_INVSTD
    assert float(t.max()) < 2 ** 24, f"{what}: sum |dz xhat| / min(invstd) = {float(t.max())} - use smaller ranges"
    assert float(dz.abs().sum(1).max()) < 2 ** 24, f"{what}: sum |dz| = {float(dz.abs().sum(1).max())}"


def check_forms(dz, s1, s2, x, mean, invstd, gamma, count, dx, what):
    """every named intermediate of the three dx forms in the code equals its own float32 round trip, and the three agree"""
    ic = 1.0 / count
    assert count == next_pow2(count), (what, count)
    mu, is_ = mean.double()[:, None, :], invstd.double()[:, None, :]
    gm = gamma.double()[None, None, :] if gamma is not None else torch.ones(1, 1, x.shape[-1], dtype=torch.float64)
    xd = x.double()
    a1, a2 = s1[:, None, :], s2[:, None, :]
    named = {}

    def n(name, v):
        named[name] = v
        return v
    xc = n("x - mu", xd - mu)
    xhat = n("xhat", xc * is_)
    n("dz xhat", dz * xhat); n("s1", a1); n("s2", a2)
    k0 = n("k0", gm * is_)
    k1 = n("k1", a1 * ic)
    k2 = n("k2", n("k0 is", k0 * is_) * n("s2 ic", a2 * ic))
    # norm_bwd_elem (device_prims.h): a = dz - k1; t = (x - mu) k2; o = fma(k0, a, -t)
    a = n("elem a", dz - k1)
    t = n("elem t", xc * k2)
    elem = n("elem o", n("elem k0 a", k0 * a) - t)
    # norm_bwd_apply_kernel: gm is (gv - a1 ic - ((x - mu) is a2) ic)
    u = n("v1 xhat a2 ic", n("v1 xhat a2", xhat * a2) * ic)
    v1 = n("v1 o", k0 * n("v1 diff", n("v1 gv - k1", dz - k1) - u))
    # norm_bwd_plane_kernel: c = fma(mu, k2, -(k0 k1)); o = fma(k0, dz, fma(-k2, x, c))
    c = n("plane c", n("plane mu k2", mu * k2) - n("plane k0 k1", k0 * k1))
    inner = n("plane inner", c - n("plane k2 x", k2 * xd))
    plane = n("plane o", n("plane k0 dz", k0 * dz) + inner)
    for name, v in named.items():
        assert is_f32(v), f"{what}: intermediate '{name}' loses bits in fp32 - use smaller ranges"
    assert torch.equal(elem, dx) and torch.equal(v1, dx) and torch.equal(plane, dx), f"{what}: the three forms of dx disagree"
    return SimpleNamespace(max_s2=float(s2.abs().max()), max_dx=float(dx.abs().max()))


def _dyadic_params(groups, C, seed):
    gen = torch.Generator().manual_seed(seed)
    mean = torch.randint(-2, 3, (groups, C), generator=gen).float()
    # every invstd and every gamma in every group, even at C = 8 (the pick of _pointwise_oracle.ssa_case)
    invstd = _INVSTD[(torch.arange(C)[None, :] + 3 * torch.arange(groups)[:, None] + seed) % 4].contiguous()
    gamma = _GAMMA[(torch.arange(C) // 4 + torch.arange(C) + seed) % 4].contiguous()
    return mean, invstd, gamma


@_cached
def dyadic_case(B, rows, C, masked, drop_p, seed, groups=None, count=None):
    """The dyadic problem of B images of rows x C.  groups = B (instance statistics, the default) or 1 (batch).
    Returns the inputs as [groups][rows per group][C] fp32 tensors, the keep mask in the three layouts the kernels read
    (`out`: fp32, kept where > 0 - masked = 1; `kb`: mmh_scale_shift_act's keep bits - masked = 2; `db`: 1 bit per element -
    the _rc entry points) and float64 s1, s2, dx for gamma given (.dx) and NULL (.dx_plain).  masked = 0: everything kept.
    count: what the entry points get as `count` (default: the next power of two >= rows per group)."""
    assert drop_p in (0.0, 0.5) and (masked or drop_p == 0.0)
    groups = B if groups is None else groups
    assert groups in (1, B)
    R = rows * (B // groups)
    shape = (groups, R, C)
    gen = torch.Generator().manual_seed(seed)
    g = E.ints(shape, seed + 1, lo=-3, hi=3)
    x = E.ints(shape, seed + 2, lo=-8, hi=8)
    keep = torch.rand(shape, generator=gen) < 0.6 if masked else torch.ones(shape, dtype=torch.bool)
    mean, invstd, gamma = _dyadic_params(groups, C, seed)
    count = float(next_pow2(R)) if count is None else float(count)
    dsc = 1.0 / (1.0 - drop_p)
    P = SimpleNamespace(g=g, x=x, keep=keep, mean=mean, invstd=invstd, gamma=gamma, count=count, dsc=dsc, drop_p=drop_p,
                        groups=groups, rows=R, C=C, masked=masked)
    # masked = 1: the fp32 output of the forward; kept where > 0 (0 and -0 are NOT kept)
    pos = torch.tensor([0.5, 1.0, 3.0])[torch.randint(0, 3, shape, generator=gen)]
    neg = torch.tensor([0.0, -0.0, -1.0])[torch.randint(0, 3, shape, generator=gen)]
    P.out = torch.where(keep, pos, neg)
    P.kb, P.db = keep_bytes(keep), drop_bytes(keep)
    P.dz, P.s1, P.s2, P.dx = norm_bwd_ref(g, keep, dsc, x, mean, invstd, gamma, count)
    P.dx_plain = norm_bwd_ref(g, keep, dsc, x, mean, invstd, None, count)[3]
    return P


def check_dyadic(P, what):
    check_any_order(P.dz, P.x, P.mean, P.invstd, what)
    if P.count == next_pow2(P.count):
        check_forms(P.dz, P.s1, P.s2, P.x, P.mean, P.invstd, None, P.count, P.dx_plain, what + " gamma NULL")
        return check_forms(P.dz, P.s1, P.s2, P.x, P.mean, P.invstd, P.gamma, P.count, P.dx, what)
    return None


# (B, H, W, C) of the two-pass tests; rows = H * W per image
TWO_PASS = [(2, 37, 29, 64),     # c8 = 8: second generation, 1073 rows: a short last chunk
            (1, 81, 81, 96),     # C / 8 = 12 is no power of two: first generation; 82 chunks of 81 rows, the last one empty
            (3, 6, 6, 24),       # first generation, fewer rows than one chunk
            (1, 5, 7, 1024),     # c8 = 128: two rows per block iteration
            (2, 3, 3, 8)]        # c8 = 1: 256 row lanes for 9 rows
TWO_PASS_BATCH = [(2, 37, 29, 64), (3, 6, 6, 24)]       # the same images as ONE group (BatchNorm)
MASKS = [(0, 0.0), (1, 0.5), (1, 0.0), (2, 0.5), (2, 0.0)]      # (masked, drop_p)
# (g, x, dx) storage types: all-fp32, all 16-bit, and the two mixed g32 / x16 forms
TYPES = [("f32", "f32", "f32"), ("bf16", "bf16", "bf16"), ("fp16", "fp16", "fp16"), ("f32", "bf16", "f32"), ("f32", "fp16", "fp16")]
SEED_TWO_PASS, SEED_RC, SEED_PLANE, SEED_GATE, SEED_NBR, SEED_PROD = 100, 200, 300, 400, 500, 600


def two_pass_case(shape, masked, drop_p, batch=False):
    B, H, W, C = shape
    return dyadic_case(B, H * W, C, 1 if masked else 0, drop_p, SEED_TWO_PASS, groups=1 if batch else B)


# ------------------------------------------------------------------------------------------------ recomputed keep (_rc)
RC_SHAPES = [(2, 37, 29, 64), (3, 6, 6, 16)]
RC_MODES = [(1, 0.5), (1, 0.0), (0, 0.0)]       # (relu, drop_p)


@_cached
def rc_case(shape, relu, drop_p):
    """mmh_norm_bwd_reduce_rc / _apply_rc decide the keep again: dropout bit AND (not relu OR fma(x, scale, shift) > 0).
    scale[g][c] in {1, 2, 4} (a power of two that keeps x scale an integer) and shift[g][c] a half-integer: x scale + shift is
    exact and never 0."""
    B, H, W, C = shape
    rows = H * W
    gen = torch.Generator().manual_seed(SEED_RC)
    P = SimpleNamespace(groups=B, rows=rows, C=C, drop_p=drop_p, dsc=1.0 / (1.0 - drop_p), relu=relu, count=float(next_pow2(rows)))
    P.g = E.ints((B, rows, C), SEED_RC + 1, lo=-3, hi=3)
    P.x = E.ints((B, rows, C), SEED_RC + 2, lo=-8, hi=8)
    P.scale = torch.tensor([1.0, 2.0, 4.0])[torch.randint(0, 3, (B, C), generator=gen)]
    P.shift = torch.tensor([-2.5, -0.5, 0.5, 1.5])[torch.randint(0, 4, (B, C), generator=gen)]
    P.bit = torch.rand((B, rows, C), generator=gen) < 0.5 if drop_p > 0 else torch.ones((B, rows, C), dtype=torch.bool)
    act = P.x.double() * P.scale.double()[:, None, :] + P.shift.double()[:, None, :]
    assert bool((act != 0).all()) and is_f32(act)
    P.keep = P.bit & ((act > 0) if relu else torch.ones_like(P.bit))
    P.db = drop_bytes(P.bit)
    P.mean, P.invstd, P.gamma = _dyadic_params(B, C, SEED_RC)
    P.dz, P.s1, P.s2, P.dx = norm_bwd_ref(P.g, P.keep, P.dsc, P.x, P.mean, P.invstd, P.gamma, P.count)
    P.dx_plain = norm_bwd_ref(P.g, P.keep, P.dsc, P.x, P.mean, P.invstd, None, P.count)[3]
    return P


# ------------------------------------------------------------------------------------------------ the one-pass plane kernel
FT = 1024


def plane_nr(g):
    return 4 if g == "f32" else 8


def plane_lpr_log2(rows, C, g):
    """pointwise.hip: plane_lpr_log2, transcribed"""
    c8 = C // 8
    if C % 8 or c8 < 1 or c8 > TPB or c8 & (c8 - 1) or rows <= 0 or rows * c8 >= 1 << 30:
        return -1
    cap = FT * plane_nr(g)
    if rows > cap:
        return -1
    l = 0
    while l < 3 and (2 << l) <= c8 and rows * (2 << l) <= cap:
        l += 1
    return l


def plane_has_tail(rows, C, g):
    """some slot of some lane lies past the plane: rows of (NR - 1) * nslots + rs >= rows for the largest rs = nslots - 1"""
    l = plane_lpr_log2(rows, C, g)
    return plane_nr(g) * (FT >> l) > rows


# (B, H, W, C), g type, the expected lpr_log2, tail.  cap = 1024 * NR rows * lanes per row (NR = 8 for a 16-bit g, 4 for fp32);
# l grows while 2^(l+1) <= c8 and rows * 2^(l+1) <= cap, up to 3
PLANE = [((5, 8, 8, 8), "g16", 0, True),        # c8 = 1: l = 0
         ((5, 8, 8, 8), "f32", 0, True),
         ((2, 23, 17, 64), "g16", 3, True),     # rows 391: 391 * 8 = 3128 <= 4096 <= 8192: l = 3 for both g types
         ((2, 23, 17, 64), "f32", 3, True),
         ((1, 64, 64, 16), "g16", 1, False),    # rows 4096, c8 = 2: 4096 * 2 = 8192 <= 8192: l = 1, 512 slots * 8 rows: every slot live
         ((1, 64, 64, 16), "f32", 0, False),    # 4096 * 2 > 4096: l = 0 and rows = 1024 * 4 exactly: every slot live, no tail
         ((1, 45, 45, 32), "g16", 2, True),     # rows 2025, c8 = 4: 2025 * 4 = 8100 <= 8192: l = 2; 256 slots * 8 = 2048 > 2025
         ((1, 45, 45, 32), "f32", 1, True),     # 2025 * 2 = 4050 <= 4096 < 8100: l = 1; 512 * 4 = 2048 > 2025
         ((1, 1, 8191, 8), "g16", 0, True),     # one row short of the cap
         ((1, 1, 8192, 8), "g16", 0, False)]    # the cap: 1024 * 8 rows, no tail
PLANE_VARIANTS = [(dx16, masked) for dx16 in (False, True) for masked in (False, True)]


def plane_case(shape, masked):
    B, H, W, C = shape
    return dyadic_case(B, H * W, C, 1 if masked else 0, 0.5 if masked else 0.0, SEED_PLANE)


# ------------------------------------------------------------------------------------------------ production count
# count = rows: (float)(1.0 / rows) is inexact, so dx is not.  norm_bwd_elem's roundings: inv_count (1), k1 = s1 inv_count (1),
# k2 = k0 is (s2 inv_count) (s2 inv_count, the product with the exact k0 is: 2, plus inv_count's own: 3), t = (x - mu) k2 (1),
# a = dz - k1 (1), the final fma (1): 8 roundings, each at most u = 2^-24 relative to one of the three terms of
# dx = k0 dz - k0 k1 - (x - mu) k2.  Plus half an ulp of the storage type for the store.
PROD = [(2, 37, 29, 64), (1, 45, 45, 32)]
U32 = 2.0 ** -24


def prod_case(shape, masked):
    B, H, W, C = shape
    return dyadic_case(B, H * W, C, 1 if masked else 0, 0.5 if masked else 0.0, SEED_PROD, count=H * W)


def prod_bound(P, gamma, dtype):
    """(want, allowed) float64: 8 u (|k0 dz| + |k0 k1| + |(x - mu) k2|) + half an ulp of `dtype` at want"""
    gm = gamma.double()[None, None, :] if gamma is not None else 1.0
    mu, is_ = P.mean.double()[:, None, :], P.invstd.double()[:, None, :]
    k0 = gm * is_ * torch.ones_like(mu)
    k1 = P.s1[:, None, :] / P.count
    k2 = k0 * is_ * P.s2[:, None, :] / P.count
    xc = P.x.double() - mu
    want = k0 * P.dz - k0 * k1 - xc * k2
    allow = 8 * U32 * ((k0 * P.dz).abs() + (k0 * k1).abs() + (xc * k2).abs())
    if dtype != "f32":
        p = 8 if dtype == "bf16" else 11
        _, ex = torch.frexp(want.abs() + allow)
        allow = allow + 0.5 * torch.ldexp(torch.ones_like(want), ex - p)
    return want, allow


def prod_mu_k2(P, gamma):
    """|mu k2| [groups][1][C] (float64): the magnitude the one-pass kernel rounds its per-channel constant c at"""
    gm = gamma.double()[None, None, :] if gamma is not None else 1.0
    mu, is_ = P.mean.double()[:, None, :], P.invstd.double()[:, None, :]
    return (mu * gm * is_ * is_ * P.s2[:, None, :] / P.count).abs()


# ------------------------------------------------------------------------------------------------ mmh_norm_bwd_sums_final
SUMS_FINAL_CHUNKS = (1, 7, 8, 9, 33, 255, 256, 257, 300)    # KL = 8 below 256 chunks, 32 from there; each kernel's unrolled loop
SUMS_FINAL_GROUPS, SUMS_FINAL_C = 2, 40                     # takes 4 KL chunks per turn; 40 channels: the last work-group part-filled


@_cached
def sums_final_case(chunks):
    part = E.ints((SUMS_FINAL_GROUPS, chunks, 2, SUMS_FINAL_C), 700 + chunks, lo=-100, hi=100)
    want = part.double().sum(1)
    return SimpleNamespace(part=part, s1=want[:, 0], s2=want[:, 1])


# ------------------------------------------------------------------------------------------------ the gate with the norm inside
# s2 = s3 = 0: both sigmoids are exactly 1/2 (section 6 of tests/_pointwise_oracle.py).  y2 in -8 .. 8, scale[g][c] in {1/2, 1, 2},
# shift[g][c] in -2 .. 2: s1 = fma(y2, scale, shift) is a multiple of 1/2 within 18.  Forward: out = x1 + s1 / 4.  Backward:
# g_out and the concat gradients are multiples of 4 within 12, G = g_out + g_x2n[.., C:] + g_x3n[.., C:] within 36;
# g_x1 = G, g_s1 = G / 4 (an integer within 9), g_s2 = G s1 / 8 + g_x3n[.., :C], g_s3 = G s1 / 8 + g_x2n[.., :C]: multiples of
# 1/4 within 93 - exact in fp32, rounded once where they are stored in 16 bits.  sum1 = sum g_s1, sum2 = sum g_s1 xhat with
# the dyadic mean / invstd: integers times invstd.
GATE = [(2, 37, 29, 64), (1, 5, 7, 1024)]
GATE_TYPES = [("bf16", "f32", "f32"), ("fp16", "f32", "f32"), ("bf16", "bf16", "bf16"), ("fp16", "fp16", "fp16"),
              ("bf16", "f32", "bf16"), ("fp16", "fp16", "f32")]      # y2, s2 / s3 (and their gradients), the concats (and theirs)
GATE_ABSENT = [(True, True, True), (False, True, True), (True, False, True), (True, True, False)]     # g_out, g_x2n, g_x3n present


@_cached
def gate_case(shape):
    B, H, W, C = shape
    rows = H * W
    gen = torch.Generator().manual_seed(SEED_GATE)
    s = (B, rows, C)
    P = SimpleNamespace(groups=B, rows=rows, C=C)
    P.x1 = E.ints(s, SEED_GATE + 1, lo=-8, hi=8)
    P.y2 = E.ints(s, SEED_GATE + 2, lo=-8, hi=8)
    P.scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (B, C), generator=gen)]
    P.shift = torch.randint(-2, 3, (B, C), generator=gen).float()
    P.zero = torch.zeros(s)
    P.g_out = 4.0 * E.ints(s, SEED_GATE + 3, lo=-3, hi=3)
    P.g_x2n = 4.0 * E.ints((B, rows, 2 * C), SEED_GATE + 4, lo=-3, hi=3)
    P.g_x3n = 4.0 * E.ints((B, rows, 2 * C), SEED_GATE + 5, lo=-3, hi=3)
    P.mean, P.invstd, _ = _dyadic_params(B, C, SEED_GATE)
    P.s1 = P.y2.double() * P.scale.double()[:, None, :] + P.shift.double()[:, None, :]
    P.out = P.x1.double() + P.s1 / 4.0
    P.cat = torch.cat([P.zero.double(), P.out], -1)         # x2n = cat(s3, out), x3n = cat(s2, out), s2 = s3 = 0
    # routing: y2 = 0 and shift = 0 make s1 = 0 and out = x1 whatever the gates are; s2 in 1 .. 15, s3 in -15 .. -1
    P.s2r, P.s3r = E.ints(s, SEED_GATE + 6, lo=1, hi=15), E.ints(s, SEED_GATE + 7, lo=-15, hi=-1)
    return P


def gate_bwd_ref(P, has_out, has_2, has_3):
    """float64 g_x1, g_s1, g_s2, g_s3, sum1, sum2 with any of the incoming gradients absent"""
    C = P.C
    G = torch.zeros(P.x1.shape, dtype=torch.float64)
    e2, e3 = torch.zeros_like(G), torch.zeros_like(G)
    if has_out:
        G = G + P.g_out.double()
    if has_2:
        G = G + P.g_x2n.double()[..., C:]
        e3 = P.g_x2n.double()[..., :C]
    if has_3:
        G = G + P.g_x3n.double()[..., C:]
        e2 = P.g_x3n.double()[..., :C]
    gs1 = G / 4.0
    xhat = (P.y2.double() - P.mean.double()[:, None, :]) * P.invstd.double()[:, None, :]
    return SimpleNamespace(g_x1=G, g_s1=gs1, g_s2=G * P.s1 / 8.0 + e2, g_s3=G * P.s1 / 8.0 + e3, sum1=gs1.sum(1), sum2=(gs1 * xhat).sum(1),
                           xhat=xhat)


# ------------------------------------------------------------------------------------------------ 4. statistics: a derived bound
# Inputs: integers in -8 .. 8 plus a per-channel integer offset in {0, 100}; the first and the last row of every group hold 200
# (plus the offset) - sentinels: a kernel that drops either moves the channel's mean and M2 by far more than the bound.
#
# What the kernels do (norm_stats_partial / _v2, then norm_stats_final), per (group, channel), u = 2^-24, R = max |x|,
# D = max x - min x of the channel, N rows, M2 the channel's exact sum of squared deviations:
#   a lane takes every rpi-th row of its chunk: K = its first value, sm = sum (x - K), ss = sum (x - K)^2.  On integers below
#   2^12 these are exact whatever the contraction (|x - K| <= 508, ss <= 2^18 n).  Then inv = 1 / n (1 rounding),
#   mean_l = K + sm inv (2: the product and the sum), M2_l = ss - (sm sm) inv (3 for the product, 1 for the difference).
#       mean: |sm / n| <= D, |mean_l| <= R:                       e_lane  <= (2 D + R) u             <= 5 R u
#       M2:   (sm sm) inv <= ss (Cauchy-Schwarz), ss_l <= M2_l + n_l D^2:   sum over lanes <= 4 u (M2 + N D^2)
#   m = min(rpi, rows) - 1 float merges per chunk at most (empty lanes are skipped):
#       d = mb - ma (1), w = nb / nt (1), ma += d w (2);  qa += qb + (d d) (na nb / nt) (d: 1 twice, d d: 1, the quotient: 1, the
#       product: 1, two sums: 2; na nb is an exact small integer).
#       mean: the update is a convex combination, so earlier errors do not grow; each merge adds at most 3 u |d| w + u |ma'|
#             <= (3 D + R) u <= 7 R u:                            e_mean  <= (5 + 7 m) R u
#       M2:   T_j = d^2 na nb / nt are the between-lane parts: sum T_j <= M2 and every qa <= M2: the roundings add at most
#             (5 + 2 m) u M2; d carries the error of two means (2 e_mean), which moves sum T_j by at most
#             sum w_j (4 |d_j| e_mean + 4 e_mean^2) <= 4 e_mean sqrt(N M2) + 4 e_mean^2 N  (Cauchy-Schwarz, sum w_j <= N)
#   norm_stats_final merges the chunks in double (3 levels of merges count the term above: lanes, chunk lanes, the 8 lanes):
#   its own roundings are 2^-53 relative, below u^2 (chunks + 8); the result is rounded to fp32 once: u R and u M2.
def row_geom_ok(C):
    c8 = C // 8
    return C % 8 == 0 and 1 <= c8 <= TPB and c8 & (c8 - 1) == 0


def stats_merges(rows, C, v2):
    """float merges per chunk at most: row lanes per block (second generation: 256 / (C / 8); first: 256 / (C / 4)) less one"""
    rpi = TPB // (C // 8) if v2 else TPB // (C // 4)
    return min(rpi, rows) - 1


def stats_bound(x64, merges):
    """(mean bound, relative M2 bound) per (group, channel) for x64 [groups][rows][C] (float64)"""
    N = x64.shape[1]
    R = float(x64.abs().max())
    D = x64.max(1).values - x64.min(1).values
    M2 = ((x64 - x64.mean(1, keepdim=True)) ** 2).sum(1)
    e_mean = (5 + 7 * merges) * R * U32
    mean_b = e_mean + R * U32 + 64 * R * U32 * U32
    m2_abs = U32 * (4 * (M2 + N * D * D) + (5 + 2 * merges) * M2 + M2) + 3 * (4 * e_mean * torch.sqrt(N * M2) + 4 * e_mean * e_mean * N)
    return torch.full_like(M2, mean_b), m2_abs / M2


STATS_SHAPES = TWO_PASS
STATS_STRIDED = (1073, 64, 96)      # rows, C, cs: the first-generation kernel takes the stride


@_cached
def stats_case(groups, rows, C, dtype="f32"):
    """x as the kernel gets it (every value here is exact in bf16 and fp16 too) and the float64 mean / M2 of those values"""
    off = 100.0 * ((torch.arange(C) // 3) % 2).float()
    base = E.ints((groups, rows, C), 800 + rows, lo=-8, hi=8)
    base[:, 0] = 200.0
    base[:, -1] = 200.0
    x = (base + off).to(DTYPES[dtype])
    x64 = x.double()
    assert torch.equal(x64, (base + off).double())
    mean = x64.mean(1)
    m2 = ((x64 - mean[:, None, :]) ** 2).sum(1)
    return SimpleNamespace(x=x, mean=mean, m2=m2)


def sentinel_effect(x64):
    """the least change of (mean, relative M2) per (group, channel) when the first or the last row is dropped, in float64"""
    def st(t):
        m = t.mean(1)
        return m, ((t - m[:, None, :]) ** 2).sum(1)
    m, q = st(x64)
    m_a, q_a = st(x64[:, 1:])
    m_b, q_b = st(x64[:, :-1])
    return torch.minimum((m_a - m).abs(), (m_b - m).abs()), torch.minimum((q_a - q).abs(), (q_b - q).abs()) / q


def col_geom(groups, rows, C, col_chunks=COL_CHUNKS):
    """pointwise.hip: col_geom -> (chunks, rows_per_chunk)"""
    rpi = TPB // (C // 4)
    want = max(1, (col_chunks // 2 if groups < 16 else col_chunks) // max(groups, 1))
    maxc = max(1, rows // (rpi * 8))
    chunks = min(want, maxc, 1024)
    return chunks, -(-rows // chunks)


def emulate_stats(x, groups, rows, C, v2=True):
    """norm_stats_partial_v2 (v2 = False: norm_stats_partial, the same arithmetic with 256 / (C / 4) row lanes) in numpy float32,
    operation for operation without contraction (per lane ascending rows with the shift K, then the rpi - 1 float Chan
    merges), then norm_stats_final's merge in double -> fp32 (mean, M2) [groups][C]"""
    f = np.float32
    xs = x.numpy().astype(np.float32).reshape(groups, rows, C)
    rpi = TPB // (C // 8) if v2 else TPB // (C // 4)
    chunks, rpc = col_geom(groups, rows, C)
    mean_o, m2_o = np.zeros((groups, C), np.float32), np.zeros((groups, C), np.float32)
    for gi in range(groups):
        na, ma, qa = np.zeros(C), np.zeros(C), np.zeros(C)      # the double merge over chunks (per-lane order does not matter at 2^-53)
        for ch in range(chunks):
            r0, r1 = ch * rpc, min(rows, (ch + 1) * rpc)
            ln, lm, lq = [], [], []
            for rsub in range(rpi):
                blk = xs[gi, r0 + rsub:r1:rpi]
                n = blk.shape[0]
                if n == 0:
                    ln.append(f(0)); lm.append(np.zeros(C, f)); lq.append(np.zeros(C, f))
                    continue
                K = blk[0]
                sm, ss = np.zeros(C, f), np.zeros(C, f)
                for row in blk:
                    d = row - K
                    sm = sm + d
                    ss = ss + d * d
                inv = f(1) / f(n)
                q = ss - sm * sm * inv
                ln.append(f(n)); lm.append(K + sm * inv); lq.append(np.maximum(q, f(0)))
            n_a, m_a, q_a = ln[0], lm[0].copy(), lq[0].copy()
            for j in range(1, rpi):
                nb = ln[j]
                if nb > 0:
                    nt = f(n_a + nb)
                    d = lm[j] - m_a
                    m_a = m_a + d * f(nb / nt)
                    q_a = q_a + (lq[j] + d * d * f(f(n_a * nb) / nt))
                    n_a = nt
            if n_a > 0:
                nb, mb, qb = float(n_a), m_a.astype(np.float64), q_a.astype(np.float64)
                nt = na + nb
                d = mb - ma
                ma = ma + d * (nb / nt)
                qa = qa + qb + d * d * (na * nb / nt)
                na = nt
        mean_o[gi], m2_o[gi] = ma.astype(f), qa.astype(f)
    return torch.from_numpy(mean_o), torch.from_numpy(m2_o)


STATS_FINDING = 0.5


def stats_ratio(mean, m2, P, merges):
    """worst got / bound over the (group, channel) pairs -> (mean ratio, M2 ratio); the callers print them and assert
    STATS_FINDING: the bound itself is 1, a ratio above 1/2 is already a finding"""
    mb, qb = stats_bound(P.x.double(), merges)
    rm = ((mean.double().cpu() - P.mean).abs() / mb).max()
    rq = (((m2.double().cpu() - P.m2).abs() / P.m2) / qb).max()
    return float(rm), float(rq)


# ------------------------------------------------------------------------------------------------ the merge kernels
MERGE_CHUNKS = (1, 3, 9, 57, 64, 65)    # below the 8 chunk lanes; on both sides of the 32- and 64-stride loops (k + 24, k + 56 < chunks)
MERGE_GROUPS, MERGE_C = 2, 40
MERGE_EPS, MERGE_MOMENTUM = 1e-5, 0.1


@_cached
def merge_case(chunks):
    """partials [groups][chunks][3][C]: the FIRST partial of every (group, channel) is empty (n = 0), and so are all the
    partials chunk lane 2 merges (k % 8 == 2); every group has the same total count (the entry points take one count)"""
    g = torch.Generator().manual_seed(900 + chunks)
    G, C = MERGE_GROUPS, MERGE_C
    n = torch.randint(1, 5, (1, chunks, 1, 1), generator=g).float().expand(G, chunks, 1, C).clone() * 16
    if chunks > 1:
        n[:, 0] = 0
        n[:, 2::8] = 0
    mean = torch.randn(G, chunks, 1, C, generator=g) * 0.5 + 3.0
    m2 = torch.rand(G, chunks, 1, C, generator=g) * n
    part = torch.cat([n, mean, m2], 2).contiguous()
    nd, md, qd = n.double().squeeze(2), mean.double().squeeze(2), m2.double().squeeze(2)
    count = nd.sum(1)
    mean_w = (nd * md).sum(1) / count
    m2_w = (qd + nd * (md - mean_w[:, None]) ** 2).sum(1)
    assert bool((count == count[0, 0]).all()) and float(count[0, 0]) > 0
    return SimpleNamespace(part=part, count=float(count[0, 0]), mean=mean_w, m2=m2_w)


def ulps(got, want64):
    """|got - want| in units of the fp32 ulp at want (got: fp32 tensor, want: float64)"""
    w = want64.double()
    _, ex = torch.frexp(w.abs())
    ulp = torch.ldexp(torch.ones_like(w), ex - 24).clamp_min(2.0 ** -149)
    return (got.double().cpu() - w).abs() / ulp


def finalize_ref(mean32, m2_32, count, eps, gamma=None, beta=None):
    """float64 (scale, shift, invstd) of norm_finalize_kernel's formula applied to the RETURNED fp32 mean / M2"""
    var = m2_32.double() / count
    is_ = 1.0 / torch.sqrt(var + float(np.float32(eps)))
    gm = gamma.double() if gamma is not None else 1.0
    bt = beta.double() if beta is not None else 0.0
    sc = gm * is_
    return sc, bt - mean32.double() * sc, is_


# ------------------------------------------------------------------------------------------------ sums in a dgrad's epilogue
# mmh_conv3x3_lp16_dgrad_nbr: the 16-bit dx of an integer problem of tests/_exact.py (integers under the bf16 cap) is the
# gradient g of a norm's output; xn, mean, invstd and the keep bits as in the dyadic design.  (B, H, W, Cin, Cout), reflect,
# one group (BatchNorm), masked, drop_p
NBR = [(E.FOLD_IN_KERNEL[0], True, False, True, 0.5),       # 2 x 2 tiles, every tile folds a corner
       (E.FOLD_IN_KERNEL[1], True, False, False, 0.0),      # 2 x 3 tiles, no keep bits
       ((2, 16, 16, 256, 64), False, False, True, 0.5),     # zero padding (mode 1): one 16 x 16 tile per image
       (E.FOLD_IN_KERNEL[1], True, True, True, 0.0)]        # both images as ONE group (BatchNorm), keep bits without dropout


@_cached
def nbr_case(case):
    (B, H, W, Cin, Cout), reflect, batch, masked, drop_p = case
    conv = E.problem(B, H, W, Cin, Cout, 3, 1, 1, reflect, 0, E.CAP_F32, E.CAP_BF16)
    groups = 1 if batch else B
    R = B * H * W // groups
    gen = torch.Generator().manual_seed(SEED_NBR)
    P = SimpleNamespace(conv=conv, groups=groups, rows=R, C=Cin, drop_p=drop_p, dsc=1.0 / (1.0 - drop_p), masked=masked)
    P.x = E.ints((groups, R, Cin), SEED_NBR + 2, lo=-8, hi=8)
    P.keep = torch.rand((groups, R, Cin), generator=gen) < 0.6 if masked else torch.ones((groups, R, Cin), dtype=torch.bool)
    P.kb = keep_bytes(P.keep)
    P.mean, P.invstd, _ = _dyadic_params(groups, Cin, SEED_NBR)
    g = conv.dx.reshape(groups, R, Cin)
    P.dz, P.s1, P.s2, _ = norm_bwd_ref(g, P.keep, P.dsc, P.x, P.mean, P.invstd, None, float(next_pow2(R)))
    return P


# ------------------------------------------------------------------------------------------------ epilogue statistics
# mmh_conv3x3_lp16_fprop_stats, mmh_conv_lp16_fprop_stats, mmh_conv_stem16_stats on integer problems with |y| <= 16 (the weight
# density lowered until the oracle's y meets it).  wave_tile_stats (device_prims.h) divides only by powers of two, so every
# partial (n, mean, M2) is exact: |y| <= 16 in 5 bits, a mean over 2^k values adds k fraction bits, a squared deviation
# doubles them - within fp32's 24.  (B, H, W, Cin, Cout, k, stride, pad, reflect), weight density
EPI_STATS = {"halo": ((2, 16, 16, 64, 256, 3, 1, 1, True), 1.0 / 48),
             "s2": ((2, 32, 32, 64, 128, 3, 2, 1, False), 1.0 / 32),
             "stem": ((2, 32, 32, 8, 64, 7, 1, 3, True), 1.0 / 16)}
EPI_CAP = 16.0


def epi_problem(kind):
    spec, density = EPI_STATS[kind]
    return E.problem(*spec, 0, EPI_CAP, E.CAP_F32, density)
