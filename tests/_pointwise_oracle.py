"""Exact problems for the HBM-bound kernels of csrc/pointwise.hip and their float64 references (plain module, no fixtures).

The method of tests/_exact.py carried over to the pointwise, loss, pooling and Adam kernels: on integer or dyadic inputs
these kernels are exact in fp32 - whatever the order of evaluation and whether or not the compiler contracts a * b + c into
an FMA - so a correct kernel equals the float64 reference bit for bit, element by element, and one missing, doubled or
misrouted element moves a result by a whole unit.  The conditions that make "exact" true are checked on the reference alone
(check_exact, check_sum; tests/test_pointwise_exact_cpu.py runs them over every case list here): each value is exactly
representable in the type it is stored in, each sum stays below 2^24.  A case that breaks a condition gets smaller inputs.

Sizes.  The launchers cap the grid (grid_for: 4096 blocks of 256 threads; mmh_adam_step 8192; mmh_pool_exchange 256 per
image); past the cap a thread takes a second turn of its grid-stride loop.  Every family runs at one vector, at one block
short by a vector (255 vectors), at one block plus a vector (257) and at the cap plus 257 vectors, where the second turn is
ragged and ends in the middle of a block.

The families with transcendentals (BCE, the gate with real sigmoids, Adam) are held element by element to
|got - want| <= TOL * S + 2^-126, S the float64 sum of the absolute values of the terms added at that element
(within(), below); their references are pinned to torch's CPU implementations by the CPU test file.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from tests import _exact as E

TPB = 256
CAP = 4096 * TPB                                    # lanes of a capped grid_for() launch
N_F4 = (4, 4 * 255, 4 * 257, 4 * (CAP + 257))       # float4 kernels and the fp32 losses: 4, 1020, 1028, 4 195 332
N_8 = (8, 8 * 255, 8 * 257, 8 * (CAP + 257))        # 8-wide 16-bit kernels: 8, 2040, 2056, 8 390 664
N_ADAM = (1, 255, 257, 8192 * TPB + 257)            # one element per lane: 2 097 409
POOL_ELEMS = 4 * (256 * TPB + 257)                  # mmh_pool_exchange, per image: 263 172
assert N_F4[3] == 4195332 and N_ADAM[3] == 2097409 and POOL_ELEMS == 263172

_CACHES = []


def _cached(fn):
    """one entry per case, computed once and shared (read-only!) by the tests of a module.  Unbounded on purpose - every case of a
    list is wanted again by the next test - but large: the cases at 4.2 M and 8.4 M elements and the (2, 260, 260, 128) pooling
    case hold about 1 GB with their float64 references, so each test module drops them at teardown (clear_caches)."""
    fn = functools.lru_cache(maxsize=None)(fn)
    _CACHES.append(fn)
    return fn


def clear_caches():
    for fn in _CACHES:
        fn.cache_clear()


DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
FLOOR = 2.0 ** -126                                 # a flushed subnormal


def check_exact(t64, dtypes, what):
    """every value of the float64 reference is finite and survives a round trip through each storage type"""
    assert t64.dtype == torch.float64, what
    assert bool(torch.isfinite(t64).all()), f"{what}: the reference holds a NaN or an inf"
    for name in dtypes:
        back = t64.to(DTYPES[name]).double()
        assert torch.equal(back, t64), f"{what}: not exactly representable in {name}: {int((back != t64).sum())} values - use smaller inputs"


def check_sum(total, what):
    assert abs(float(total)) < 2 ** 24 and float(total) == round(float(total)), f"{what}: the sum {total} is not an integer below 2^24"


def within(got, want64, S64, tol, what, dtype=None):
    """|got - want| <= tol * S + 2^-126 element by element; for a 16-bit `dtype` want is first rounded to it and one unit in
    its last place is added.  Returns the worst (|got - want| - 2^-126) / S over the elements with S > 0, which the callers
    print (the floor taken off: a flushed subnormal would otherwise read as an error of 1)."""
    g = got.detach().double().cpu().reshape(-1)
    want64, S64 = want64.reshape(-1), S64.reshape(-1)
    assert g.shape == want64.shape, (what, g.shape, want64.shape)
    allow = tol * S64 + FLOOR
    if dtype is not None and dtype != "f32":
        want64 = want64.to(DTYPES[dtype]).double()
        p, tiny = (8, 2.0 ** -133) if dtype == "bf16" else (11, 2.0 ** -24)      # significand bits, smallest subnormal
        _, ex = torch.frexp(want64.abs())                                        # |v| = m * 2^ex, m in [0.5, 1): ulp = 2^(ex - p)
        ulp = torch.ldexp(torch.ones_like(want64), ex - p).clamp_min(tiny)
        allow = allow + torch.where(want64 == 0, torch.full_like(ulp, tiny), ulp)
    err = (g - want64).abs()
    bad = ~(err <= allow)                                             # a NaN is bad
    pos = S64 > 0
    worst = float(((err[pos] - FLOOR).clamp_min(0.0) / S64[pos]).max()) if bool(pos.any()) else 0.0
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements out of bound; first at {i}: got {float(g[i])!r}, "
                             f"want {float(want64[i])!r}, S {float(S64[i])!r}, allowed {float(allow[i])!r}; worst |got - want| / S = {worst:.3e}")
    return worst


# ------------------------------------------------------------------------------------------------ 1. activation backward
# y in k/8 (exact zeros and +-1 among them), g in -3 .. 3: g * (1 - y^2) = g (64 - k^2) / 64 has a numerator below 2^8, so it is
# exact in fp32, fp16 and bf16 (8 significand bits); g * [y > 0] trivially
ACT_RELU, ACT_TANH = 1, 2


@_cached
def act_bwd_case(n):
    g = E.ints((n,), 11, lo=-3, hi=3)
    y = E.ints((n,), 12, lo=-8, hi=8) / 8.0
    gd, yd = g.double(), y.double()
    want = {ACT_RELU: gd * (yd > 0), ACT_TANH: gd * (1.0 - yd * yd)}
    return SimpleNamespace(g=g, y=y, want=want)


# ------------------------------------------------------------------------------------------------ 2. MaxPool2d(2, 2)
# integer x in -1 .. 1: most windows tie; g in 1 .. 4: a gradient sent to two places or to none shows
MAXPOOL = [(1, 2, 2, 4),            # one window, one lane
           (3, 6, 10, 12),          # C / 4 = 3, Wo = 5: neither divides the lane index evenly
           (2, 14, 2, 64),          # Wo = 1: 2 * 7 * 1 * 16 = 224 lanes, one block short
           (2, 260, 260, 128)]      # 2 * 130 * 130 * 32 = 1 081 600 lanes > 1 048 576: 33 024 take a second turn


def maxpool_ref(x, g):
    """float64 (y, dx): the gradient goes to the FIRST maximum of the window in scan order (0,0), (0,1), (1,0), (1,1)"""
    x, g = x.double(), g.double()
    taps = [(0, 0), (0, 1), (1, 0), (1, 1)]
    v = [x[:, r::2, c::2] for r, c in taps]
    m, k = v[0].clone(), torch.zeros(v[0].shape, dtype=torch.int64)
    for j in (1, 2, 3):
        better = v[j] > m                                   # strictly: an equal later tap does not take over
        m = torch.where(better, v[j], m)
        k = torch.where(better, torch.full_like(k, j), k)
    dx = torch.full_like(x, float("nan"))                   # every element is written below, as the kernel must
    for j, (r, c) in enumerate(taps):
        dx[:, r::2, c::2] = torch.where(k == j, g, torch.zeros_like(g))
    return m, dx


@_cached
def maxpool_case(shape):
    B, H, W, C = shape
    x = E.ints(shape, 21)
    g = E.ints((B, H // 2, W // 2, C), 22, lo=1, hi=4)
    y, dx = maxpool_ref(x, g)
    return SimpleNamespace(x=x, g=g, y=y, dx=dx)


# ------------------------------------------------------------------------------------------------ 3, 4. L1 / MSE losses
# a, b in {-1, 0, 1}: |a - b| <= 2 and (a - b)^2 <= 4 are integers and every partial sum stays below 2^24 (checked), so with
# weight = denom = 1 the output is the integer sum itself.  Backward: weight / denom = 2^-3 and gscalar = 0.75 give
# k = 3 * 2^-5; k * sign, 2 k * (a - b) and [a > 0] * k * sign have numerators of at most 4 bits.  A third of the pairs have a == b.
LOSS_WEIGHTED = (10.0,)             # one more forward case: weight 10, denom n, rounded once from double
BWD_WEIGHT, BWD_DENOM, BWD_GS = 1.0, 8.0, 0.75


@_cached
def loss_case(n):
    a, b = E.ints((n,), 31), E.ints((n,), 32)
    d = a.double() - b.double()
    kk = float(np.float32(np.float32(BWD_WEIGHT / BWD_DENOM) * np.float32(BWD_GS)))
    return SimpleNamespace(a=a, b=b, l1=float(d.abs().sum()), mse=float((d * d).sum()), n_equal=int((d == 0).sum()),
                           l1_bwd=kk * torch.sign(d), mse_bwd=2.0 * kk * d, l1_relu_bwd=kk * torch.sign(d) * (a.double() > 0))


def weighted(total, weight, n):
    """what loss_final_kernel leaves: double(sum) * (double(float(weight)) / denom), rounded once to float"""
    return float(np.float32(np.float64(total) * (np.float64(np.float32(weight)) / np.float64(n))))


# ------------------------------------------------------------------------------------------------ 5. scale, shift, activation
# x in -8 .. 8, scale in {0, +-0.5, +-1, +-2}, shift in -4 .. 4: |x * scale + shift| <= 20 in steps of 0.5; the survivors of a
# dropout with p = 0.5 are doubled exactly (<= 40); the residual in -8 .. 8 makes |out| <= 48, a multiple of 0.5: 7 bits.
# (groups, rows, C): block = 256 lanes = (256 / c8) rows x c8 = C / 8 column groups; a block covers step = 4 * 256 / c8 rows per
# iteration; chunks = min(row_chunks / groups, rows / (2 step)), rows_per_chunk = ceil(ceil(rows / chunks) / step) * step
SSA_GEOMS = [(2, 1073, 64),      # c8 = 8: 32 rows per iteration, step 128; row_chunks 4096: min(2048, 1073 / 256 = 4) -> 384 rows per
                                 # chunk, 3 chunks, the last with 305 rows (2 full iterations + 49 rows: u = 0, 1 and 17 lanes of u = 1's
                                 # row group); row_chunks 5: 2 chunks of 640; row_chunks 1: 1 chunk, 1152 >= rows
             (1, 1500, 8),       # c8 = 1: 256 rows per iteration, step 1024 > rows / 2: one chunk of 2048 rows whatever row_chunks says,
                                 # the second iteration 476 rows (u = 0 full, u = 1 with 220 lanes, u = 2, 3 idle)
             (3, 37, 2048),      # c8 = 256: one row per iteration and lane group, step 4; min(1365, 37 / 8 = 4) -> 12 rows per chunk,
                                 # 4 chunks, the last with ONE row (u = 1 .. 3 idle); row_chunks 5: 5 / 3 = 1 chunk of 40
             (2, 36, 24),        # c8 = 3 is no power of two: the first-generation kernel whatever pw_v2 says; 432 lanes, two blocks
             (1, 6561, 96)]      # c8 = 12: first generation; 157 464 lanes, 616 blocks, the last with 24 lanes
SSA_MODES = [(False, False, False), (True, False, False), (False, False, True), (True, True, False), (True, True, True)]  # relu, drop, residual
SSA_OPTIONS = [(v2, rc) for v2 in (0, 1) for rc in (1, 5, 4096)]
_SCALES = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])


@_cached
def ssa_case(geom):
    groups, rows, C = geom
    pick = (torch.arange(C)[None, :] + 3 * torch.arange(groups)[:, None]) % 7      # every scale in every group, even at C = 8
    return SimpleNamespace(x=E.ints((groups, rows, C), 42, lo=-8, hi=8), scale=_SCALES[pick],
                           shift=E.ints((groups, C), 43, lo=-4, hi=4), residual=E.ints((groups, rows, C), 44, lo=-8, hi=8),
                           mask=E.ints((groups, rows, C), 45, lo=0, hi=1).to(torch.uint8))


@_cached
def ssa_ref(geom, mode):
    """float64 out and the keep bits (uint8, one byte per 4 channels, bit e = value e BEFORE the residual > 0)"""
    relu, drop, res = mode
    P = ssa_case(geom)
    r = P.x.double() * P.scale.double()[:, None, :] + P.shift.double()[:, None, :]
    if relu:
        r = r.clamp_min(0.0)
    if drop:
        r = torch.where(P.mask != 0, 2.0 * r, torch.zeros_like(r))
    k = (r > 0).reshape(-1, 4).to(torch.uint8)
    bits = (k[:, 0] | (k[:, 1] << 1) | (k[:, 2] << 2) | (k[:, 3] << 3)).reshape(geom[0], geom[1], geom[2] // 4)
    if res:
        r = r + P.residual.double()
    return r, bits


# ------------------------------------------------------------------------------------------------ 6. PATBlock gate, routing
# With s2 = s3 = 0 both sigmoids are exactly 0.5 (1 / (1 + exp(0))).  Forward, call A: out = x1 + s1 / 4 with x1 in -8 .. 8 and
# s1 in 4 * (-4 .. 4): integers within 12.  Call B pins where s2 and s3 are COPIED: s1 = 0 makes out = x1 whatever the gates are,
# s2 in 1 .. 15 and s3 in -15 .. -1 (distinct, non-zero): x2n = cat(s3, out), x3n = cat(s2, out).
# Backward: s1 in 16 * (-2 .. 2), gradients in -3 .. 3: G = g_out + g_x2n[.., C:] + g_x3n[.., C:] (|G| <= 9), g_x1 = G, g_s1 = G / 4,
# g_s2 = G * s1 * a3 * a2 * (1 - a2) + g_x3n[.., :C] = G * s1 / 8 + g_x3n[.., :C], g_s3 = G * s1 / 8 + g_x2n[.., :C]: integers within 39.
GATE_SHAPES = [(37, 8), (1073, 64), (5, 2048)]          # rows x C: 74 lanes; 17 168 lanes = 67 blocks + 16 lanes; C / 4 = 512 > a block


@_cached
def gate_exact_case(shape):
    rows, C = shape
    P = SimpleNamespace(x1=E.ints(shape, 51, lo=-8, hi=8), s1f=4.0 * E.ints(shape, 52, lo=-4, hi=4), s1b=16.0 * E.ints(shape, 53, lo=-2, hi=2),
                        s2c=E.ints(shape, 54, lo=1, hi=15), s3c=E.ints(shape, 55, lo=-15, hi=-1), zero=torch.zeros(shape),
                        g_out=E.ints(shape, 56, lo=-3, hi=3), g_x2n=E.ints((rows, 2 * C), 57, lo=-3, hi=3), g_x3n=E.ints((rows, 2 * C), 58, lo=-3, hi=3))
    out_a = P.x1.double() + P.s1f.double() / 4.0
    P.fwd_a = (out_a, torch.cat([P.zero.double(), out_a], -1), torch.cat([P.zero.double(), out_a], -1))
    out_b = P.x1.double()
    P.fwd_b = (out_b, torch.cat([P.s3c.double(), out_b], -1), torch.cat([P.s2c.double(), out_b], -1))
    return P


def gate_exact_bwd(P, has_out, has_2, has_3):
    """float64 (g_x1, g_s1, g_s2, g_s3) at s2 = s3 = 0 and s1 = P.s1b, with any of the incoming gradients absent"""
    C = P.x1.shape[1]
    G = torch.zeros(P.x1.shape, dtype=torch.float64)
    e2, e3 = torch.zeros_like(G), torch.zeros_like(G)
    if has_out:
        G = G + P.g_out.double()
    if has_2:
        G = G + P.g_x2n.double()[:, C:]
        e3 = P.g_x2n.double()[:, :C]
    if has_3:
        G = G + P.g_x3n.double()[:, C:]
        e2 = P.g_x3n.double()[:, :C]
    return G, G / 4.0, G * P.s1b.double() / 8.0 + e2, G * P.s1b.double() / 8.0 + e3


# ------------------------------------------------------------------------------------------------ 7. image pool exchange
POOL_B, POOL_SLOTS = 3, 4
POOL_SRC = (2, -2, 0)       # out[0] = slot 2 (which dst[0] overwrites in the same call: its OLD content), out[1] = image 1, out[2] = slot 0
POOL_DST = (2, -1, 3)       # slot 2 <- image 0, image 1 is not stored, slot 3 <- image 2; slots 0 and 1 stay


@_cached
def pool_case():
    pool = E.ints((POOL_SLOTS, POOL_ELEMS), 61, lo=-100, hi=100)
    images = E.ints((POOL_B, POOL_ELEMS), 62, lo=-100, hi=100)
    out = torch.stack([pool[s] if s >= 0 else images[-1 - s] for s in POOL_SRC])
    after = pool.clone()
    for i, d in enumerate(POOL_DST):
        if d >= 0:
            after[d] = images[i]
    return SimpleNamespace(pool=pool, images=images, out=out.double(), after=after.double())


# ------------------------------------------------------------------------------------------------ 8. non-finite gradient flag
NONFINITE_N = N_F4[3]       # + r, r in 0 .. 3


def nonfinite_positions(r):
    """element indices at n = NONFINITE_N + r: the first element, the last vector of the first turn (vector CAP - 1), the first
    vector of the second turn (vector CAP), and each of the r scalar tail elements behind the n / 4 whole vectors"""
    n = NONFINITE_N + r
    return [0, 4 * (CAP - 1) + 3, 4 * CAP] + [4 * (n // 4) + j for j in range(r)]


# ------------------------------------------------------------------------------------------------ 9. BCE with logits
# loss_partial_kernel<0>: t = exp(-|x|); softplus(-|x|) = t * (1 - t / 2) where t < 2^-10 (|x| > 10 ln 2 = 6.9315), log(1 + t) above
BCE_POINTS = [0.0,
              2.0 ** -20,       # log branch, t = 1 - 2^-20: log(2 - 2^-20)
              0.5,              # log branch
              6.90, 6.92,       # log branch: t = 1.032 and 1.012 x 2^-10
              6.94, 6.96,       # series branch: t = 0.9915 and 0.972 x 2^-10
              10.0, 20.0,       # series branch; at 20 the second term is below an ulp
              87.0,             # exp(-87) = 1.6e-38 is the last normal fp32 value on this grid
              89.0,             # exp(-89) = 2.2e-39 is subnormal (may be flushed), exp(89) overflows fp32
              100.0, 1e4]       # exp(-x) underflows to 0 (and at 1e4 in float64 too)
BCE_THRESHOLD = 2.0 ** -10
BCE_LOG_SIDE, BCE_SERIES_SIDE = (0.0, 2.0 ** -20, 0.5, 6.90, 6.92), (6.94, 6.96, 10.0, 20.0, 87.0, 89.0, 100.0, 1e4)
BCE_MARGIN = {6.92: 0.01, 6.94: 0.008}      # the two nearest points are 1.15 % and 0.85 % off the threshold; every other point >= 2 %
BCE_GRID = sorted([0.0] + [s * p for p in BCE_POINTS[1:] for s in (-1.0, 1.0)])
# the forward returns a sum: groups of four neighbours of the sorted grid (similar magnitudes, so that no point hides behind another),
# the last group padded with its own last point - and every point once more on its own, four times over
BCE_GROUPS = [tuple((BCE_GRID + [BCE_GRID[-1]] * 3)[i:i + 4]) for i in range(0, len(BCE_GRID), 4)] + [(p,) * 4 for p in BCE_GRID]
BCE_K, BCE_GS = 0.125, 0.75     # backward: weight / denom and the incoming gradient (k = 3 * 2^-5 is exact)


def f32(values):
    """the float64 values of the fp32 numbers the kernel is given"""
    return torch.tensor(values, dtype=torch.float32).double()


def _softplus(z):
    return torch.logaddexp(torch.zeros_like(z), z)


def sigmoid64(x):
    return torch.exp(-_softplus(-x))


def bce_terms(x64, target):
    """float64 per-element loss and S = max(x, 0) + |x * target| + softplus(-|x|)"""
    sp = _softplus(-x64.abs())
    return x64.clamp_min(0.0) - x64 * target + sp, x64.clamp_min(0.0) + (x64 * target).abs() + sp


def bce_bwd(x64, target, k):
    """float64 per-element gradient k * (sigmoid(x) - target) and S = |k| * (sigmoid(x) + target)"""
    s = sigmoid64(x64)
    return k * (s - target), abs(k) * (s + target)


@_cached
def bce_large(n=N_F4[3]):
    reps = -(-n // len(BCE_GRID))
    return torch.tensor(BCE_GRID, dtype=torch.float32).repeat(reps)[:n].contiguous()


# ------------------------------------------------------------------------------------------------ 10. gate with real sigmoids
GATE_S = sorted([0.0] + [s * v for v in (0.25, 1.0, 4.0, 12.0, 30.0, 90.0) for s in (-1.0, 1.0)])
GATE_REAL_SHAPE = (len(GATE_S) ** 2, 8)     # one row per (s2, s3) pair, 8 channels of x1 / s1 / gradients each: 169 x 8


def mk(shape, seed):
    """tests/test_pointwise_gpu.py::_mk on the CPU"""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@_cached
def gate_real_case():
    rows, C = GATE_REAL_SHAPE
    grid = torch.tensor(GATE_S, dtype=torch.float32)
    s2 = grid.repeat_interleave(len(GATE_S))[:, None].expand(rows, C).contiguous()
    s3 = grid.repeat(len(GATE_S))[:, None].expand(rows, C).contiguous()
    P = SimpleNamespace(x1=mk((rows, C), 71), s1=mk((rows, C), 72), s2=s2, s3=s3, g_out=mk((rows, C), 73),
                        g_x2n=mk((rows, 2 * C), 74), g_x3n=mk((rows, 2 * C), 75))
    P.fwd, P.fwd_S, P.bwd, P.bwd_S = gate_real_ref(P.x1, P.s1, P.s2, P.s3, P.g_out, P.g_x2n, P.g_x3n)
    return P


def gate_real_ref(x1, s1, s2, s3, g_out, g_x2n, g_x3n):
    """closed forms in float64: (out, x2n, x3n), S(out), (g_x1, g_s1, g_s2, g_s3), their S"""
    x1, s1, s2, s3, g_out, g_x2n, g_x3n = (t.double() for t in (x1, s1, s2, s3, g_out, g_x2n, g_x3n))
    C = x1.shape[1]
    a2, a3 = sigmoid64(s2), sigmoid64(s3)
    out = x1 + s1 * a2 * a3
    t2, e3, t3, e2 = g_x2n[:, C:], g_x2n[:, :C], g_x3n[:, C:], g_x3n[:, :C]
    G = g_out + t2 + t3
    S_G = g_out.abs() + t2.abs() + t3.abs()
    # 1 - sigmoid(s) = sigmoid(-s): no cancellation in the reference
    bwd = (G, G * a2 * a3, G * s1 * a3 * a2 * sigmoid64(-s2) + e2, G * s1 * a2 * a3 * sigmoid64(-s3) + e3)
    bwd_S = (S_G, S_G, S_G * s1.abs() + e2.abs(), S_G * s1.abs() + e3.abs())
    return (out, torch.cat([s3, out], -1), torch.cat([s2, out], -1)), x1.abs() + s1.abs(), bwd, bwd_S


# ------------------------------------------------------------------------------------------------ 11. Adam
ADAM = dict(lr=2e-4, beta1=0.5, beta2=0.999, eps=1e-8, grad_scale=0.5, loss_scale=1024.0)      # both scalings are exact
ADAM_STEPS = 3
ADAM_P_RTOL, ADAM_P_ATOL = 1e-5, 1e-7       # tests/test_pointwise_gpu.py::test_adam_matches_torch_fixture


@_cached
def adam_case(n):
    """p0 and three gradients; g is 2048 * randn, so that g * grad_scale / loss_scale is randn exactly"""
    return SimpleNamespace(p0=mk((n,), 81), grads=[mk((n,), 82 + i) * 2048.0 for i in range(ADAM_STEPS)])


def adam_coef(step, lr=ADAM["lr"], beta1=ADAM["beta1"], beta2=ADAM["beta2"]):
    """the two bias-correction coefficients as the host forms them: in double from the fp32 lr and betas, then rounded to float"""
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    return float(np.float32(float(np.float32(lr)) / (1.0 - b1 ** step))), float(np.float32(1.0 / np.sqrt(1.0 - b2 ** step)))


def adam_ref(p, g, m, v, step, cfg=None):
    """one step in float64 on fp32 inputs -> (p, m, v), (S_m, S_v)"""
    cfg = cfg or ADAM
    p, g, m, v = (t.double() for t in (p, g, m, v))
    b1, b2, eps = float(np.float32(cfg["beta1"])), float(np.float32(cfg["beta2"])), float(np.float32(cfg["eps"]))
    step_size, inv_sqrt_bc2 = adam_coef(step, cfg["lr"], cfg["beta1"], cfg["beta2"])
    gr = g * (cfg["grad_scale"] / cfg["loss_scale"])
    mm = b1 * m + (1.0 - b1) * gr
    vv = b2 * v + (1.0 - b2) * gr * gr
    pp = p - step_size * (mm / (torch.sqrt(vv) * inv_sqrt_bc2 + eps))
    return (pp, mm, vv), ((b1 * m).abs() + ((1.0 - b1) * gr).abs(), b2 * v + (1.0 - b2) * gr * gr)
