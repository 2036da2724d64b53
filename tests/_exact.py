"""Integer-exact convolution problems and their float64 oracle (plain module, no fixtures).

Convolution is exact on small integers: with x, w, dy in {-1, 0, 1} every product and every partial sum is an integer far
below 2^24, so it is exactly representable in fp32 - and in the fp32 accumulators that bf16 / fp16 operands feed - whatever
the order of summation, the split-K slab order or the number of summation levels.  A correct direct kernel therefore equals
the float64 oracle (oracle/ops_ref.py) bit for bit, element by element; one missing product, or one product too many,
moves an element by at least 1.  The whole-tensor relative L1 the other tests use cannot see one wrong element
(tests/test_conv_exact_cpu.py writes that gap down as a test).

The conditions on the INPUTS are checked on the oracle's result alone, before anything is compared: every result is
integer-valued and within the cap of the type it will be stored in.  A case that exceeds a cap gets a lower weight density,
never a higher cap.

Input recipe (a different seed per operand): x, dy in {-1, 0, 1} dense; w in {-1, 0, 1} with one third of the entries
non-zero; bias in {-2 .. 2}; addend within +-8.

The case lists of tests/test_conv_exact_gpu.py live here, so that tests/test_conv_exact_cpu.py checks the caps of every
(shape, density) pair without a GPU.

What the capped families test, and what they cannot: with every result inside the exact range of its storage type no 16-bit
store ever rounds, so these families test the SUMS (which products, how often) and say nothing about the STORE.  The
round-once families at the end of this file lift the caps: operands are integers the 16-bit type still holds exactly, the
fp32 accumulator still holds the exact sum, and the one correct stored value is the round-to-nearest-even of that sum,
taken once, after bias and activation (rne16, assert_rounded_once; tests/test_conv_round16_gpu.py and _cpu.py).
"""
import contextlib
import functools
from types import SimpleNamespace

import torch

from oracle import ops_ref as R

CAP_F32 = float(2 ** 24)    # fp32 outputs: integers up to 2^24 are exact
CAP_BF16 = 256.0            # bf16-stored outputs (out16 / dx16): 8 significand bits
CAP_FP16 = 2048.0           # fp16-stored outputs: 11 significand bits
W_DENSITY = 1.0 / 3.0

SEED_X, SEED_W, SEED_B, SEED_DY, SEED_ADD = 1, 2, 3, 4, 7


def ints(shape, seed, density=1.0, lo=-1, hi=1):
    """Seeded integer-valued fp32 tensor in [lo, hi]; a seeded mask keeps a `density` share of the entries."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g).to(torch.float32)
    if density < 1.0:
        t = t * (torch.rand(tuple(shape), generator=g) < density).to(torch.float32)
    return t


def _check(t, cap, what):
    if t is None:
        return
    assert torch.equal(t, t.round()), f"oracle {what} is not integer-valued: the inputs are not integers"
    m = float(t.abs().max()) if t.numel() else 0.0
    assert m <= cap, f"oracle {what}: max |value| {m} exceeds the cap {cap} of its storage type - lower the weight density"


def exact_conv(x, w, bias, dy, stride, pad, reflect, act=0, cap_y=CAP_F32, cap_dx=CAP_F32):
    """float64 y, dx, dw, db of a Conv2d (x NHWC, w [kh,kw,Cin,Cout]); act 0 | 1 only (tanh is not exact)."""
    assert act in (0, 1)
    y, dx, dw, db = R.conv2d_grads(x, w, bias, dy, stride, pad, reflect, act)
    _check(y, cap_y, "y"); _check(dx, cap_dx, "dx"); _check(dw, CAP_F32, "dw"); _check(db, CAP_F32, "db")
    return y, dx, dw, db


def exact_convT(x, w, bias, dy, cap_y=CAP_F32, cap_dx=CAP_F32):
    """float64 y, dx, dw, db of ConvTranspose2d(k3, s2, p1, op1) (x NHWC [B,h,w,CinT], w [kh,kw,CoutT,CinT])."""
    y, dx, dw, db = R.convT2d_grads(x, w, bias, dy)
    _check(y, cap_y, "y"); _check(dx, cap_dx, "dx"); _check(dw, CAP_F32, "dw"); _check(db, CAP_F32, "db")
    return y, dx, dw, db


def _first_diff(got, want):
    bad = got != want
    n = int(bad.sum())
    idx = tuple(int(i) for i in bad.nonzero()[0])
    return n, idx, float((got - want).abs().max())


def assert_exact(got, want, what):
    """got (any device / dtype) == want (float64, CPU) element by element; the message says WHERE they differ."""
    g = got.detach().double().cpu()
    assert tuple(g.shape) == tuple(want.shape), (what, tuple(g.shape), tuple(want.shape))
    if torch.equal(g, want):
        return
    n, idx, worst = _first_diff(g, want)
    raise AssertionError(f"{what}: {n} of {want.numel()} elements differ; first at index (b, h, w, c) = {idx}: got {float(g[idx])}, "
                         f"want {float(want[idx])}; largest |got - want| = {worst}")


def assert_rounds(got, want, what):
    """fp32 Winograd: not exact (non-dyadic transform constants), but every correct output is an integer plus rounding
    noise and a dropped product moves an element by at least 1 - so got must ROUND to want, element by element (a derived
    bound of 0.5).  Returns max |got - want| (reported; a value above 0.05 is a finding)."""
    g = got.detach().double().cpu()
    assert tuple(g.shape) == tuple(want.shape), (what, tuple(g.shape), tuple(want.shape))
    worst = float((g - want).abs().max())
    print(f"\n[round] {what}: max |got - want| = {worst:.3e}")
    if not torch.equal(g.round(), want):
        n, idx, _ = _first_diff(g.round(), want)
        raise AssertionError(f"{what}: {n} of {want.numel()} elements do not round to the oracle; first at index (b, h, w, c) = {idx}: "
                             f"got {float(g[idx])}, want {float(want[idx])}; largest |got - want| = {worst}")
    return worst


@contextlib.contextmanager
def option(key, value):
    """mmh_set_option(key, value) for the body, then back to the value the key HAD (mmh_get_option), not to a default this file
    believes in; asserts that the restore took.  Options are process-global and the suite runs in one process."""
    from mmhand_amd import lib
    key = key.encode() if isinstance(key, str) else key
    old = lib.get_option(key)
    lib.check(lib.load().mmh_set_option(key, int(value)), "mmh_set_option")       # not lib.call: a test's spy counts kernels only
    try:
        yield old
    finally:
        lib.check(lib.load().mmh_set_option(key, old), "mmh_set_option")
        assert lib.get_option(key) == old, (key, old, lib.get_option(key))


@contextlib.contextmanager
def options(**kv):
    """several option()s at once: options(conv_xcd=0, conv_bn256=0)"""
    with contextlib.ExitStack() as stack:
        for k, v in kv.items():
            stack.enter_context(option(k, v))
        yield


# one entry per distinct problem of the case lists below, so that every oracle is computed once per process whatever the order
# of the tests (70 problems; the two 364 x 364 ones hold about 0.3 GB between them)
@functools.lru_cache(maxsize=96)
def problem(B, H, W, Cin, Cout, k, stride, pad, reflect, act=0, cap_y=CAP_F32, cap_dx=CAP_F32, density=W_DENSITY, kind="conv"):
    """One seeded integer problem and its oracle, computed once and shared (read-only!) by the tests that need it.
    kind "conv": Conv2d.  kind "convT": ConvTranspose2d(k3, s2, p1, op1) with x [B,H,W,Cin], w [3,3,Cout,Cin].
    kind "head": Conv2d whose last output channel is padding (the Generator head, 3 -> 4): its weights, bias and dy are 0."""
    x = ints((B, H, W, Cin), SEED_X)
    bias = ints((Cout,), SEED_B, lo=-2, hi=2)
    if kind == "convT":
        w = ints((3, 3, Cout, Cin), SEED_W, density)
        dy = ints((B, 2 * H, 2 * W, Cout), SEED_DY)
        y, dx, dw, db = exact_convT(x, w, bias, dy, cap_y, cap_dx)
    else:
        w = ints((k, k, Cin, Cout), SEED_W, density)
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        dy = ints((B, Ho, Wo, Cout), SEED_DY)
        if kind == "head":
            w[..., -1] = 0; bias[-1] = 0; dy[..., -1] = 0
        y, dx, dw, db = exact_conv(x, w, bias, dy, stride, pad, reflect, act, cap_y, cap_dx)
    return SimpleNamespace(x=x, w=w, bias=bias, dy=dy, y=y, dx=dx, dw=dw, db=db)


# ------------------------------------------------------------------------------------------------ case lists
# Each family: the cases as tests/test_conv_exact_gpu.py parametrises them, and spec(case) -> the arguments of problem().
# A family run in bf16 AND fp16 with 16-bit outputs is held to the smaller (bf16) cap.
# Every problem is the plain conv (act 0): dx and dw of the raw wrappers know no activation; where a test asks the kernel for
# its ReLU epilogue it compares with relu(y) of the same oracle (integer-valued and under the same cap as y).

def _conv(B, H, W, Cin, Cout, k, s, p, refl, act=0, cap_y=CAP_F32, cap_dx=CAP_F32, kind="conv"):
    return (B, H, W, Cin, Cout, k, s, p, refl, act, cap_y, cap_dx, W_DENSITY, kind)


# fp32 direct kernels ----------------------------------------------------------------------------------------
IGEMM = [(1, 12, 20, 256, 256, 3, 1, 1, True), (3, 8, 8, 12, 20, 3, 1, 1, True), (2, 18, 14, 16, 32, 3, 2, 1, False),
         (1, 16, 16, 44, 64, 7, 1, 3, True), (2, 16, 16, 64, 4, 7, 1, 3, True), (2, 16, 16, 4, 64, 3, 1, 1, False)]
LEVELS2 = [("3x3", 1, 24, 40, 256, 128), ("s2", 2, 32, 32, 128, 256)]
CONVT = [(2, 6, 10, 128, 64), (2, 8, 8, 32, 16)]
DGRAD_S2 = [(b, h, w, ci, co) for (b, h, w) in [(1, 20, 36), (1, 2, 2), (1, 18, 4)] for (ci, co) in [(64, 128), (128, 256)]]
DGRAD_S2_PERSISTENT = [(6, 128, 256, 64, 128), (6, 128, 256, 128, 256)]
WGRAD_S2 = [(1, 20, 36, 64, 128), (1, 2, 2, 64, 128), (2, 34, 66, 128, 256)]
STEM_F32 = [(2, 9, 37, 8, True), (1, 20, 24, 44, True), (1, 24, 32, 48, False)]
STEM_WGRAD_F32 = [(2, 8, 64, 8), (2, 8, 64, 44), (1, 6, 128, 8), (1, 6, 128, 44)]
THIN = [(1, 20, 70, 64, 4, True), (2, 37, 130, 8, 4, True), (1, 8, 8, 16, 4, False)]
THIN_WGRAD = [(2, 9, 33, 128)]
COLSUM = (5000, 256)

# 16-bit kernels (each in bf16 and fp16) ---------------------------------------------------------------------
HALO_FPROP = [(2, 9, 11, 64, 256, True), (3, 7, 5, 512, 256, True), (1, 16, 16, 256, 512, False)]
FOLD_DGRAD = [(1, 32, 16, 256, 256), (1, 16, 48, 256, 128)]
FOLD_IN_KERNEL = [(1, 32, 32, 256, 128), (2, 32, 48, 256, 64)]     # the smallest images that take the in-kernel fold (mode 2)
DGRAD_ADD = [(2, 17, 33, 256, 128, True)]
SLICE = [(1, 20, 40, 256, 512, True)]
LP16G = [(1, 32, 20, 128, 256, 2, False), (2, 16, 16, 64, 128, 2, False)]
S2_LP16 = [(3, 16, 32, 64, 128), (2, 16, 96, 128, 256)]           # the ragged (B odd / H != W) cases of test_conv_s2_lp16_gpu
S1_LP16 = [(1, 8, 16), (3, 24, 48), (1, 40, 40)]                  # VGG conv1_2, 64 -> 64; 40 x 40 is off the 8 x 16 tile
FLAT_STEMS = [(2, 12, 13, 8, 64, 7, True), (1, 16, 16, 44, 64, 7, True)]
STEM16 = [(2, 9, 33, 44, True), (1, 12, 12, 3, False)]
STEM16_3X3 = [(3, 19, 21, 3)]
WGRAD3X3 = [(3, 7, 5, 512, 256, True), (2, 9, 11, 256, 256, True)]
WGRAD_S2_9TAP = [(3, 6, 70, 64, 128), (2, 34, 8, 64, 256)]
WGRAD_FLAT = [(2, 12, 13, 8, 64, 7, 1, True)]
WGRAD_STEM16 = [(2, 9, 33, 44, True)]
HEAD_WGRAD = [(2, 70, 21), (3, 19, 33)]
HEAD_DGRAD = [(3, 19, 33), (1, 8, 8)]
N4_HEAD = [(2, 37, 130, True), (3, 9, 17, False)]
N4_STEM_DGRAD = [(2, 37, 66, 8, True), (1, 20, 70, 24, True)]
N4_VGG_DGRAD = [(2, 37, 66)]

# fp32 Winograd (held to `round`) ----------------------------------------------------------------------------
WINO6 = [(2, 13, 17, 128, 128, True), (1, 37, 12, 32, 32, True), (1, 19, 13, 64, 32, True), (2, 25, 16, 32, 32, True),
         (1, 24, 18, 128, 64, False)]
WINO6_FUSED = [WINO6[0], WINO6[3]]
WINO24 = [(1, 12, 20, 256, 256, True), (2, 8, 8, 64, 128, False)]
WINO2_FWD = [(2, 12, 20, 256, 256, True)]
WINO_WGRAD_DMA = (16, 64, 256, 256)     # (planes, tiles, Cin, Cout) of tests/test_wino_gemm_gpu.py

# ---------------------------------------------------------------------------- variants and partitions (round 2 of this file)
# The lists above run every family at its smallest ragged shapes; most dispatch decisions in csrc/ sit ABOVE those shapes.
# Each case below is there for one branch; its comment gives the arithmetic that selects it (BM = 128 rows per tile, BK = 32).
# tests/test_conv_variants_gpu.py runs them, tests/test_conv_exact_cpu.py checks their caps and the host-only queries.

# fp32 implicit GEMM, 3x3 s1 reflect -------------------------------------------------------------------------
IGEMM_BN128 = [(1, 9, 11, 16, 128),      # 64 < N, N % 256 != 0: conv_igemm_kernel<128,2,2> (and <..., DBUF> with conv_dbuf)
               (1, 9, 11, 16, 256)]      # conv_bn256 = 0: the same template with gx = 2
IGEMM_XCD = [(1, 33, 35, 8, 192),        # M = 1155: gy = 10 >= 8, band = 1: 8 row tiles remapped, 2 keep their ids, the last holds
                                         # 3 rows; gx = 2 on the 128 template, the second column tile half empty
             (1, 33, 35, 8, 512),        # the 256-wide template, gx = 2, same rows
             (1, 33, 35, 8, 64),         # gx = 1: remapped only because of conv_xcd1
             (1, 32, 32, 8, 192),        # M = 1024: gy = 8, no ragged rest
             (1, 33, 35, 192, 8)]        # dgrad: N = Cin = 192, gx = 2, gy = 10 (the main piece of the folded dgrad)
IGEMM_CW = [(1, 15, 17, 128, 64),        # Cin = 128: 4 chunks of 32 per tap: conv_cw 1, 2 (= auto), 4; M = 255
            (1, 15, 17, 96, 64)]         # Cin = 96: 3 chunks: auto 1, conv_cw 3
IGEMM_TALL = [(1, 364, 364, 4, 64)]      # conv_tall = 2: 32 < N <= 64 and M = 132496 >= 256 * 512, M % 256 = 144 (zero padding)
DGRAD_S2_TALL = [(1, 364, 364, 64, 8)]   # stride-2 dgrad, 32 < Cin <= 64, M per parity class = 182 * 182 = 33124 >= 256 * 128: the
                                         # 256-row multi-piece kernel (conv_tall = 1); Cout = 8 keeps it off the halo kernel

# fp32 wgrad, 3x3 s1 reflect: Mrows = 9 * Cin <= 128 and N <= 128 give one tile, so splits = P / 256 ---------
WGRAD_SPLITS = [(1, 5, 461, 8, 32),      # P = 2305: 9 splits of 288 pixels, the last has 1
                (1, 13, 197, 8, 32),     # P = 2561: 10 splits of 288, split 9 is empty
                (2, 64, 65, 8, 32),      # P = 8320: 32 splits of 288, 29..31 empty: slab_reduce_par_kernel<8>
                (1, 40, 135, 8, 32)]     # P = 5400: 21 splits: slab_reduce_par_kernel<4>, one unrolled round + remainder 16, 20
WGRAD_SPLITS_N = {2305: 9, 2561: 10, 8320: 32, 5400: 21}
WGRAD_SLOTS = (4, 4)                     # wgrad_slots = 4 at P = 2305: 4 splits fill one round of 4 slots, 9 do not
WGRAD_TEMPLATES = [(2, 9, 11, 12, 128),  # Mrows = 108 (ragged over 128); <128,2,2> and, with wgrad_dbuf, its DBUF form
                   (2, 9, 11, 12, 256),  # <256,2,2>; wgrad_bn256 = 0: <128,2,2> with two column tiles
                   (2, 9, 11, 12, 48),   # <64,2,2>, 16 columns masked
                   (2, 9, 11, 12, 20)]   # <32,4,1>, 12 columns masked

# fp32 Winograd F(6x6,3x3) (held to `round`) -----------------------------------------------------------------
WINO_PERSIST = [(2, 72, 72, 64, 256, True)]   # 288 tiles: MT = 3, NT = 2, W = 64 * 6 = 384, Wx = 48 > 32 * occ at wino_gemm_occ = 1;
                                              # K = 64 > WINO_FOLD * BK: the two-level fold; input transform: nblk = 288 * 64 / 256 = 72
# Winograd-domain GEMMs at the stage level (integer operands: plain GEMMs, exact) ---------------------------
WINO_WGRAD_PERSIST = (64, 2403, 128, 256)     # (planes, tiles, Cin, Cout): 9 splits of 288 tiles (the last has 99), MT = 1, NT = 2:
                                              # W = 64 * 9 * 2 = 1152, Wx = 144 > 32 * 4: two items per workgroup at occ 3 and 4
WINO_BF16_PERSIST = (16, 1100, 256, 512)      # (planes, tiles, K, N): MT = 9, NT = 4: W = 576, Wx = 72 > 64 (bk 128) and > 32 (occ 1)

# 16-bit halo kernel, persistent: more than 256 (16 x 16-pixel, 256-channel) tiles on 256 CUs ---------------------
HALO_PERSIST_FPROP = [(1, 184, 184, 64, 512, True)]     # 12 x 12 ragged pixel tiles x 2 column tiles = 288
HALO_PERSIST_DGRAD = [(1, 192, 192, 512, 64)]           # dgrad: N = Cin = 512: 12 x 12 x 2 = 288; multiples of 16: mode 2 folds
HALO_TILE, HALO_TBN = 16, 256

_B16 = dict(cap_y=CAP_BF16, cap_dx=CAP_BF16)

FAMILIES = {
    "igemm": (IGEMM, lambda c: _conv(*c)),
    "levels2": (LEVELS2, lambda c: _conv(c[1], c[2], c[3], c[4], c[5], 3, 2 if c[0] == "s2" else 1, 1, c[0] != "s2")),
    "convT": (CONVT, lambda c: (c[0], c[1], c[2], c[3], c[4], 3, 2, 1, False, 0, CAP_F32, CAP_F32, W_DENSITY, "convT")),
    "dgrad_s2": (DGRAD_S2 + DGRAD_S2_PERSISTENT, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], 3, 2, 1, False)),
    "wgrad_s2": (WGRAD_S2, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], 3, 2, 1, False)),
    "stem_f32": (STEM_F32, lambda c: _conv(c[0], c[1], c[2], c[3], 64, 7, 1, 3, c[4])),
    "stem_wgrad_f32": (STEM_WGRAD_F32, lambda c: _conv(c[0], c[1], c[2], c[3], 64, 7, 1, 3, True)),
    "thin": (THIN, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], 7, 1, 3, c[5])),
    "thin_wgrad": (THIN_WGRAD, lambda c: _conv(c[0], c[1], c[2], c[3], 4, 7, 1, 3, True)),
    "halo_fprop": (HALO_FPROP, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], 3, 1, 1, c[5], 0, **_B16)),
    "fold_dgrad": (FOLD_DGRAD, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], 3, 1, 1, True, 0, **_B16)),
    "fold_in_kernel": (FOLD_IN_KERNEL, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], 3, 1, 1, True, 0, **_B16)),
    "dgrad_add": (DGRAD_ADD, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], 3, 1, 1, c[5])),
    "slice": (SLICE, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], 3, 1, 1, c[5], 0, **_B16)),
    "lp16g": (LP16G, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], 3, c[5], 1, c[6], 0, **_B16)),
    "s2_lp16": (S2_LP16, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], 3, 2, 1, False, 0, **_B16)),
    "s1_lp16": (S1_LP16, lambda c: _conv(c[0], c[1], c[2], 64, 64, 3, 1, 1, False, 0, **_B16)),
    "flat_stems": (FLAT_STEMS, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], c[5], 1, c[5] // 2, c[6], 0, **_B16)),
    "stem16": (STEM16, lambda c: _conv(c[0], c[1], c[2], c[3], 64, 7, 1, 3, c[4], 0, **_B16)),
    "stem16_3x3": (STEM16_3X3, lambda c: _conv(c[0], c[1], c[2], c[3], 64, 3, 1, 1, False, 0, **_B16)),
    "wgrad3x3": (WGRAD3X3, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], 3, 1, 1, c[5])),
    "wgrad_s2_9tap": (WGRAD_S2_9TAP, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], 3, 2, 1, False)),
    "wgrad_flat": (WGRAD_FLAT, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[5] // 2, c[7])),
    "wgrad_stem16": (WGRAD_STEM16, lambda c: _conv(c[0], c[1], c[2], c[3], 64, 7, 1, 3, c[4])),
    "head_wgrad": (HEAD_WGRAD, lambda c: _conv(c[0], c[1], c[2], 64, 4, 7, 1, 3, True, kind="head")),
    "head_dgrad": (HEAD_DGRAD, lambda c: _conv(c[0], c[1], c[2], 64, 4, 7, 1, 3, True, 0, kind="head", **_B16)),
    "n4_head": (N4_HEAD, lambda c: _conv(c[0], c[1], c[2], 64, 4, 7, 1, 3, c[3])),
    "n4_stem_dgrad": (N4_STEM_DGRAD, lambda c: _conv(c[0], c[1], c[2], c[3], 64, 7, 1, 3, c[4])),
    "n4_vgg_dgrad": (N4_VGG_DGRAD, lambda c: _conv(c[0], c[1], c[2], 4, 64, 3, 1, 1, False)),
    "wino6": (WINO6, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], 3, 1, 1, c[5])),
    "wino24": (WINO24, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], 3, 1, 1, c[5], 0)),
    "wino2_fwd": (WINO2_FWD, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], 3, 1, 1, c[5])),
    "igemm_bn128": (IGEMM_BN128, lambda c: _conv(*c, 3, 1, 1, True)),
    "igemm_xcd": (IGEMM_XCD, lambda c: _conv(*c, 3, 1, 1, True)),
    "igemm_cw": (IGEMM_CW, lambda c: _conv(*c, 3, 1, 1, True)),
    "igemm_tall": (IGEMM_TALL, lambda c: _conv(*c, 3, 1, 1, False)),
    "dgrad_s2_tall": (DGRAD_S2_TALL, lambda c: _conv(*c, 3, 2, 1, False)),
    "wgrad_splits": (WGRAD_SPLITS, lambda c: _conv(*c, 3, 1, 1, True)),
    "wgrad_templates": (WGRAD_TEMPLATES, lambda c: _conv(*c, 3, 1, 1, True)),
    "wino_persist": (WINO_PERSIST, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], 3, 1, 1, c[5])),
    "halo_persist_fprop": (HALO_PERSIST_FPROP, lambda c: _conv(c[0], c[1], c[2], c[3], c[4], 3, 1, 1, c[5], 0, **_B16)),
    "halo_persist_dgrad": (HALO_PERSIST_DGRAD, lambda c: _conv(*c, 3, 1, 1, True, 0, cap_dx=CAP_BF16)),
}


def case_problem(family, case):
    return problem(*FAMILIES[family][1](case))


# ================================================================================================ the store: round once
# The families above keep every result where its storage type is exact.  The families below do the opposite on purpose:
# operands are integers the 16-bit type holds exactly (|v| <= 256 in bf16, <= 2048 in fp16), optionally times one power of
# two per operand, so every product and partial sum is still an integer (times that power) below 2^24 and the fp32
# accumulator holds the exact sum in any order - but the sum no longer fits the 16-bit type.  The one correct stored value
# is RNE(exact sum + bias, after the activation), bit for bit.  No tolerance anywhere: every expectation is derived.
TD = {"bf16": torch.bfloat16, "fp16": torch.float16}
_SIG = {torch.bfloat16: 8, torch.float16: 11}          # significand bits incl. the hidden one
_EMIN = {torch.bfloat16: -126, torch.float16: -14}     # exponent of the smallest normal
XMAX = {torch.bfloat16: 256, torch.float16: 2048}      # integers up to here are exact operands

# the conditions on the oracle alone (shares of all elements); a case that misses one gets another xm or density
MIN_INEXACT, MIN_TIES, MIN_TIES_UP, MIN_TIES_DOWN, MIN_NEG_INEXACT = 0.25, 0.10, 0.04, 0.04, 0.10


def _same(a, b):
    """element-wise a == b with NaN == NaN"""
    return (a == b) | (a.isnan() & b.isnan())


def rne16(t64, td):
    """round-to-nearest-even of a float64 tensor to bf16 / fp16 (inf on overflow, gradual underflow).  The values must be
    fp32 values (that is what an accumulator can hold): float64 -> fp32 is then exact and fp32 -> 16 bits rounds once.
    tests/test_conv_round16_cpu.py checks the cast against integer arithmetic on the fp32 bit pattern."""
    assert t64.dtype == torch.float64 and td in _SIG, (t64.dtype, td)
    f = t64.to(torch.float32)
    assert bool(_same(f.double(), t64).all()), "rne16: a value is not exactly representable in fp32"
    return f.to(td)


def _bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def assert_bits16(got16, want16, what, exact64=None):
    """got16 == want16 bit for bit (zeros with their sign); NaN matches NaN whatever the payload"""
    assert got16.dtype == want16.dtype, (what, got16.dtype, want16.dtype)
    g, w_ = got16.detach().cpu(), want16.detach().cpu()
    assert tuple(g.shape) == tuple(w_.shape), (what, tuple(g.shape), tuple(w_.shape))
    ok = (_bits16(g) == _bits16(w_)) | (g.isnan() & w_.isnan())
    if bool(ok.all()):
        return
    bad = ~ok
    idx = tuple(int(i) for i in bad.nonzero()[0])
    ex = "" if exact64 is None else f" (exact value {float(exact64[idx])!r})"
    raise AssertionError(f"{what}: {int(bad.sum())} of {w_.numel()} elements differ bit for bit; first at index {idx}: got "
                         f"{float(g[idx])!r} (0x{int(_bits16(g)[idx]):04x}), want {float(w_[idx])!r} (0x{int(_bits16(w_)[idx]):04x}){ex}")


def assert_rounded_once(got16, exact64, td, what):
    """got16 (any device) == RNE(exact64) in td, element by element and bit for bit"""
    assert got16.dtype == td, (what, got16.dtype, td)
    assert_bits16(got16, rne16(exact64, td), what, exact64)


def round_shares(v64, td):
    """shares of the elements of v64 that are not representable in td, exact ties, ties that RNE rounds up / down in
    magnitude, and negative AND not representable - by float64 arithmetic on the value's own 16-bit grid, without a cast"""
    a = v64.abs()
    _, e = torch.frexp(a)                                               # a = m 2^e with m in [0.5, 1)
    e = (e - 1).clamp_min(_EMIN[td])                                    # subnormals share the smallest normal's grid
    q = a / torch.ldexp(torch.ones_like(a), e - (_SIG[td] - 1))         # in units of the grid: exact (powers of two)
    fl = q.floor()
    fr = q - fl
    tie, odd = fr == 0.5, fl % 2 == 1
    m = lambda t: float(t.double().mean())     # noqa: E731
    return dict(inexact=m(fr != 0), ties=m(tie), ties_up=m(tie & odd), ties_down=m(tie & ~odd), neg_inexact=m((fr != 0) & (v64 < 0)))


def check_round_conditions(v64, td, what, scale=1.0, relu=False):
    """the conditions of a round-once problem, on the oracle alone; returns the shares"""
    assert bool((v64.float().double() == v64).all()), f"{what}: a result is not exactly representable in fp32"
    assert float(v64.abs().max()) < CAP_F32 * scale, f"{what}: |result| reaches 2^24 x the scale"
    assert bool(rne16(v64, td).isfinite().all()), f"{what}: a result is not finite in {td} - lower xm"
    s = round_shares(v64, td)
    for key, least in (("inexact", MIN_INEXACT), ("ties", MIN_TIES), ("ties_up", MIN_TIES_UP), ("ties_down", MIN_TIES_DOWN)) + \
            ((("neg_inexact", MIN_NEG_INEXACT),) if relu else ()):
        assert s[key] >= least, f"{what}: share of {key} elements {s[key]:.3f} < {least} - another xm or density, not a lower share"
    return s


def _xm(nterms, td):
    """operand magnitude (a power of two, at most what td holds exactly) at which a sum of `nterms` products x * (+-1), x
    uniform in [-xm, xm] (variance about xm^2 / 3), has a standard deviation of about twice the exact range of td"""
    import math
    cap = 2.0 * (CAP_BF16 if td is torch.bfloat16 else CAP_FP16)
    return int(min(XMAX[td], 2 ** round(math.log2(cap / math.sqrt(nterms / 3.0)))))


# round-once families: cases (the shapes the 16-bit families above already have) and spec(case) ->
# (B, H, W, Cin, Cout, k, stride, pad, reflect, kind, w density, outputs held to the conditions)
def _r(B, H, W, Cin, Cout, k, s, p, refl, kind="conv", density=W_DENSITY, outs=("y", "dx")):
    return (B, H, W, Cin, Cout, k, s, p, refl, kind, density, outs)


ROUND_FAMILIES = {
    "halo_fprop": (HALO_FPROP, lambda c: _r(c[0], c[1], c[2], c[3], c[4], 3, 1, 1, c[5], outs=("y",))),
    "halo_persist_fprop": (HALO_PERSIST_FPROP, lambda c: _r(c[0], c[1], c[2], c[3], c[4], 3, 1, 1, c[5], outs=("y",))),
    "fold_dgrad": (FOLD_DGRAD, lambda c: _r(c[0], c[1], c[2], c[3], c[4], 3, 1, 1, True, outs=("dx",))),
    "fold_in_kernel": (FOLD_IN_KERNEL, lambda c: _r(c[0], c[1], c[2], c[3], c[4], 3, 1, 1, True, outs=("dx",))),
    "halo_persist_dgrad": (HALO_PERSIST_DGRAD, lambda c: _r(*c, 3, 1, 1, True, outs=("dx",))),
    "lp16g": (LP16G, lambda c: _r(c[0], c[1], c[2], c[3], c[4], 3, c[5], 1, c[6])),
    "s2_lp16": (S2_LP16, lambda c: _r(c[0], c[1], c[2], c[3], c[4], 3, 2, 1, False)),
    "s1_lp16": (S1_LP16, lambda c: _r(c[0], c[1], c[2], 64, 64, 3, 1, 1, False)),
    "flat_stems": (FLAT_STEMS, lambda c: _r(c[0], c[1], c[2], c[3], c[4], c[5], 1, c[5] // 2, c[6], outs=("y",))),
    "stem16": (STEM16, lambda c: _r(c[0], c[1], c[2], c[3], 64, 7, 1, 3, c[4], density=1.0 if c[3] <= 3 else W_DENSITY, outs=("y",))),
    "stem16_3x3": (STEM16_3X3, lambda c: _r(c[0], c[1], c[2], c[3], 64, 3, 1, 1, False, density=1.0, outs=("y",))),
    "head_dgrad": (HEAD_DGRAD, lambda c: _r(c[0], c[1], c[2], 64, 4, 7, 1, 3, True, kind="head", outs=("dx",))),
    # the same with dense weights: 147 products per element, enough of them to steer an element to the fp16 threshold
    "head_dgrad_dense": (HEAD_DGRAD[:1], lambda c: _r(c[0], c[1], c[2], 64, 4, 7, 1, 3, True, kind="head", density=1.0, outs=("dx",))),
    # ConvTranspose2d(k3, s2, p1, op1) of the two LP16G shapes seen from the other side: x [B, H/2, W/2, Cout], w as it is
    "convT": ([(c[0], c[1] // 2, c[2] // 2, c[4], c[3]) for c in LP16G],
              lambda c: _r(c[0], c[1], c[2], c[3], c[4], 3, 2, 1, False, kind="convT")),
}


def _nterms(spec):
    """average number of non-zero products per element of y and of dx"""
    B, H, W, Cin, Cout, k, stride, pad, reflect, kind, density, outs = spec
    nz = density * 2.0 / 3.0
    if kind == "convT":
        return k * k * Cin / 4.0 * nz, k * k * Cout * nz
    co = Cout - 1 if kind == "head" else Cout
    return k * k * Cin * nz, k * k * co / float(stride * stride) * nz


def _round_oracle(spec, x, w, bias, dy):
    """float64 (y before the activation, dx) of the conv that spec describes"""
    B, H, W, Cin, Cout, k, stride, pad, reflect, kind, density, outs = spec
    if kind == "convT":
        y, dx, _, _ = R.convT2d_grads(x, w, bias, dy)
    else:
        y, dx, _, _ = R.conv2d_grads(x, w, bias, dy, stride, pad, reflect, 0)
    return y.detach(), dx.detach()


@functools.lru_cache(maxsize=64)
def round_problem(family, case, lp, edge=None):
    """One seeded round-once problem and its exact float64 results (shared, read-only!).  lp: "bf16" | "fp16".
    edge None: integer operands, x in [-xm_x, xm_x], dy in [-xm_dy, xm_dy], w in {-1, 0, 1}, bias in [-2 cap, 2 cap].
    edge "scaled": the same kind of problem times a power of two per operand - fp16: x, w, dy times 2^-13 with |x|, |dy| <= 8,
    so that every result is a multiple of 2^-26 below 2^-14 (stored as an fp16 subnormal); bf16: x, w, dy times 2^56, results
    around 2^120 (the scale is no no-op: one binade lower in the exponent field and everything changes).
    The conditions (check_round_conditions) are asserted here, on the oracle alone, before anything is compared."""
    td = TD[lp]
    spec = ROUND_FAMILIES[family][1](case)
    B, H, W, Cin, Cout, k, stride, pad, reflect, kind, density, outs = spec
    ny, ndx = _nterms(spec)
    xm_x, xm_dy = _xm(ny, td), _xm(ndx, td)
    bm = int(2 * (CAP_BF16 if td is torch.bfloat16 else CAP_FP16))
    s_op = 1.0
    if edge == "scaled":
        if td is torch.float16:
            xm_x = xm_dy = 8
            bm, s_op = 64, 2.0 ** -13
        else:
            s_op = 2.0 ** 56
    else:
        assert edge is None, edge
    s_out = s_op * s_op
    x = ints((B, H, W, Cin), SEED_X, lo=-xm_x, hi=xm_x) * s_op
    bias = ints((Cout,), SEED_B, lo=-bm, hi=bm) * s_out
    if kind == "convT":
        w = ints((3, 3, Cout, Cin), SEED_W, density) * s_op
        dy = ints((B, 2 * H, 2 * W, Cout), SEED_DY, lo=-xm_dy, hi=xm_dy) * s_op
    else:
        w = ints((k, k, Cin, Cout), SEED_W, density) * s_op
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        dy = ints((B, Ho, Wo, Cout), SEED_DY, lo=-xm_dy, hi=xm_dy) * s_op
        if kind == "head":
            w[..., -1] = 0; bias[-1] = 0; dy[..., -1] = 0
    y, dx = _round_oracle(spec, x, w, bias, dy)
    for name, t in (("x", x), ("w", w), ("dy", dy)):
        assert torch.equal(t.to(td).float(), t), f"operand {name} is not exact in {td}"
    what = f"{family} {case} {lp}" + (f" {edge}" if edge else "")
    shares = {}
    if "y" in outs:
        shares["y"] = check_round_conditions(y, td, what + " y", s_out, relu=True)
        if edge == "scaled" and td is torch.float16:
            assert float(y.abs().max()) < 2.0 ** -14, what
    if "dx" in outs:
        shares["dx"] = check_round_conditions(dx, td, what + " dx", s_out)
        if edge == "scaled" and td is torch.float16:
            assert float(dx.abs().max()) < 2.0 ** -14, what
    return SimpleNamespace(x=x, w=w, bias=bias, dy=dy, y=y, dx=dx, td=td, lp=lp, shares=shares, xm=(xm_x, xm_dy), spec=spec)


def round_cases():
    """every (family, case, lp, edge) the GPU file uses: the main problems of every family in both types, and the scaled
    edge once per family (its first case)"""
    out = []
    for fam, (cases, _) in ROUND_FAMILIES.items():
        for lp in ("bf16", "fp16"):
            out += [(fam, c, lp, None) for c in cases]
            if "persist" not in fam:            # the two large problems run once per type: their epilogues are halo_fprop's
                out.append((fam, cases[0], lp, "scaled"))
    return out


# ------------------------------------------------------------------------------------------------ fp16 overflow
# One problem per family whose exact results straddle the fp16 overflow threshold: a few elements of ONE output row are
# steered, by hand-placed operands, to the values below - six in (65504, 65520), which round to +-65504, and six at or above
# 65520, which must be +-inf (65520 itself is the tie between 65504 and 2^16: to even, that is to inf).  Every other
# element stays finite.  Steering is exact: the coefficient of an operand element in a target is a weight (by the oracle on
# a one-hot, linearity), only operands that reach ONE target are moved, and every operand stays an integer of |v| <= 2048.
# The case of each family that is steered: its first, except where that one has too few products per element to reach 65520
# with operands of |v| <= 2048 (the 8-channel flat stem; the sparse head, for which head_dgrad_dense is there).  The 3-channel
# 3x3 stem form (27 products, at most 55296 + bias) cannot reach it at all: its epilogue is the 7x7 stem's, which is steered.
OVERFLOW_CASES = {"halo_fprop": HALO_FPROP[0], "fold_dgrad": FOLD_DGRAD[0], "fold_in_kernel": FOLD_IN_KERNEL[0], "lp16g": LP16G[0],
                  "s2_lp16": S2_LP16[0], "s1_lp16": S1_LP16[0], "flat_stems": FLAT_STEMS[1], "stem16": STEM16[0],
                  "head_dgrad_dense": HEAD_DGRAD[0], "convT": (1, 16, 10, 256, 128)}
FP16_MAX, FP16_INF_FROM = 65504.0, 65520.0
OVERFLOW_TARGETS = (65505.0, 65512.0, 65519.0, -65505.0, -65519.0, 65511.0, 65520.0, 65536.0, -65520.0, 70000.0, -66000.0, 65521.0)
MIN_EACH_SIDE = 4


def _coeffs(spec, w, out, t, xshape, dyshape):
    """d out[t] / d operand (x for "y", dy for "dx") as a tensor of the operand's shape"""
    if out == "y":
        one = torch.zeros(dyshape); one[t] = 1.0
        return _round_oracle(spec, torch.zeros(xshape), w, None, one)[1]
    one = torch.zeros(xshape); one[t] = 1.0
    return _round_oracle(spec, one, w, None, torch.zeros(dyshape))[0]


def _steer(opnd, gs, cur, wants, what):
    """Move the flat integer operand `opnd` (in place, |v| <= 2048 kept) until target j, whose value is cur[j] and whose
    coefficients are gs[j], equals wants[j] for every j.  Each correction is spread evenly over ALL operands that reach the
    target with a coefficient of +-1 - the smallest change per operand, so that the elements nobody steers move little and
    stay finite - and what that does to the other targets (known: the coefficients) is corrected in the next sweep; the
    last sweeps use only operands that reach one target alone, and end exactly."""
    cur = list(cur)
    reach = sum((g != 0).to(torch.int32) for g in gs)
    for sweep in range(12):
        if all(c == w_ for c, w_ in zip(cur, wants)):
            return
        for j, g in enumerate(gs):
            rem = wants[j] - cur[j]
            if rem == 0:
                continue
            s = 1.0 if rem > 0 else -1.0
            cand = ((g.abs() == 1) & ((reach == 1) if sweep >= 4 else (reach >= 1))).nonzero().reshape(-1)
            gf = g[cand]
            c = opnd[cand].double() * gf                                # each candidate's contribution to the target now
            add, left = torch.zeros_like(c), abs(rem)
            while left > 0:
                room = 2048.0 - s * c - add
                free = (room > 0).nonzero().reshape(-1)
                assert len(free) > 0, f"{what}: target {j} is out of reach (sweep {sweep})"
                q = float(left // len(free))
                if q == 0:
                    add[free[:int(left)]] += 1.0
                    break
                inc = torch.minimum(room[free], torch.full_like(room[free], q))
                add[free] += inc
                left -= float(inc.sum())
            step = s * add * gf                                         # the change of the operand itself
            opnd[cand] = (opnd[cand].double() + step).float()
            for i, gi in enumerate(gs):
                cur[i] += float((gi[cand] * step).sum())
    raise AssertionError(f"{what}: the targets did not converge")


@functools.lru_cache(maxsize=16)
def overflow_problem(family, case):
    P0 = round_problem(family, case, "fp16")
    spec = P0.spec
    x, dy, w, bias = P0.x.clone(), P0.dy.clone(), P0.w, P0.bias
    targets = {}
    for out in spec[-1]:
        res, opnd = (P0.y, x) if out == "y" else (P0.dx, dy)
        _, Ho, Wo, C = res.shape
        n = len(OVERFLOW_TARGETS)
        up = 1 if (spec[6] == 2 and (out == "dx") == (spec[9] != "convT")) else 0      # the up-sampled side of a stride-2 conv: odd
        ts = [(0, (Ho // 2) | up, ((j * Wo) // n) | up, (7 * j + 3) % C) for j in range(n)]     # coordinates see four taps, not one
        assert len(set(ts)) == n
        gs = [_coeffs(spec, w, out, t, x.shape, dy.shape).reshape(-1) for t in ts]
        _steer(opnd.reshape(-1), gs, [float(res[t]) for t in ts], OVERFLOW_TARGETS, f"overflow_problem {family} {out}")
        targets[out] = ts
    y, dx = _round_oracle(spec, x, w, bias, dy)
    for out, ts in targets.items():
        res = y if out == "y" else dx
        for t, want in zip(ts, OVERFLOW_TARGETS):
            assert float(res[t]) == want, (family, out, t, float(res[t]), want)
        a = res.abs()
        n_inf, n_edge = int((a >= FP16_INF_FROM).sum()), int(((a > FP16_MAX) & (a < FP16_INF_FROM)).sum())
        assert n_edge >= MIN_EACH_SIDE and n_inf >= MIN_EACH_SIDE, (family, out, n_edge, n_inf)
        assert n_inf == sum(1 for v in OVERFLOW_TARGETS if abs(v) >= FP16_INF_FROM), f"{family} {out}: an element overflows that was not steered"
        assert bool((res.float().double() == res).all()) and float(a.max()) < CAP_F32
    for name, t in (("x", x), ("dy", dy)):
        assert torch.equal(t.to(torch.float16).float(), t), f"operand {name} is not exact in fp16"
    return SimpleNamespace(x=x, w=w, bias=bias, dy=dy, y=y, dx=dx, td=torch.float16, lp="fp16", spec=spec, targets=targets)


# ------------------------------------------------------------------------------------------------ NaN and inf
@functools.lru_cache(maxsize=32)
def special_problem(family, case, lp):
    """The main problem with a NaN in the LAST pixel of the operand (the tail of the last, ragged tile) and +inf in pixel
    (0, 0, 1).  The oracle propagates both (0 x NaN and 0 x inf are NaN, as in the MFMA); the condition on the oracle: its
    non-finite elements are exactly those whose receptive field holds one of the two - every channel of those pixels,
    found by running the same conv on the indicator with all-ones weights."""
    P0 = round_problem(family, case, lp)
    spec = P0.spec
    x, dy, w, bias = P0.x.clone(), P0.dy.clone(), P0.w, P0.bias
    ind_x, ind_dy = torch.zeros_like(x), torch.zeros_like(dy)
    for out in spec[-1]:
        opnd, ind = (x, ind_x) if out == "y" else (dy, ind_dy)
        c = 0 if spec[9] == "head" else opnd.shape[3] - 1
        last = (opnd.shape[0] - 1, opnd.shape[1] - 1, opnd.shape[2] - 1, c)
        opnd[last] = float("nan"); opnd[0, 0, 1, 0] = float("inf")
        ind[last] = 1.0; ind[0, 0, 1, 0] = 1.0
    y, dx = _round_oracle(spec, x, w, bias, dy)
    fy, fdx = _round_oracle(spec, ind_x, torch.ones_like(w), None, ind_dy)
    for out in spec[-1]:
        res, field = (y, fy) if out == "y" else (dx, fdx)
        assert torch.equal(~res.isfinite(), field > 0), f"special_problem {family} {out}: the oracle's non-finite set is not the receptive field"
        assert 0 < int((field > 0).sum()) < field.numel() // 2
    return SimpleNamespace(x=x, w=w, bias=bias, dy=dy, y=y, dx=dx, td=TD[lp], lp=lp, spec=spec)


# ------------------------------------------------------------------------------------------------ paths that round twice, by design
def border_sequence(P, td):
    """mode-1 dgrad of a ReflectionPad2d(1) conv with a 16-bit dx (mmh_conv3x3_lp16 mode 1, then mmh_conv2d_dgrad_border):
    the halo / row-tile kernel stores RNE(main), main = the zero-padded dgrad; border_add_kernel (conv_igemm.hip) reads that
    16-bit value at the ring pixels (rows 1, H - 2, columns 1, W - 2), adds the fp32 sum of the border terms - integers,
    exact in any order - and stores RNE again.  Two roundings at the ring, one elsewhere, in a fixed sequence:
    dx16 = RNE(RNE(main) + (dx - main)) on the ring, RNE(main) off it; returns (that, the share of elements where it
    differs from RNE(dx))."""
    B, H, W, Cin, Cout, k, stride, pad, reflect, kind, density, outs = P.spec
    main = R.conv2d_grads(P.x, P.w, None, P.dy, 1, 1, False, 0)[1].detach()
    ring = torch.zeros(main.shape, dtype=torch.bool)
    ring[:, [1, H - 2], :, :] = True
    ring[:, :, [1, W - 2], :] = True
    assert bool(_same(main, P.dx)[~ring].all())                     # the border terms land on the ring and nowhere else
    once = rne16(main, td)
    # at a ring pixel the stored value goes through one more fp32 addition (a -0 comes back as +0) and one more rounding;
    # where main itself is not finite, the stored inf / NaN plus the border terms is what float64 makes of dx = main + border
    again = torch.where(main.isfinite(), rne16(once.double() + (P.dx - main), td), rne16(P.dx, td))
    twice = torch.where(ring, again, once)
    return twice, float((_bits16(twice) != _bits16(rne16(P.dx, td))).double().mean())


def head_dgrad_sequence(P, td, dx16):
    """mmh_conv7_head_dgrad_lp16 (conv_stem16.hip): conv_stem16_kernel stores the gradient over the PADDED domain
    [B][H + 6][W + 6][64] in 16 bits (RNE, store4); head_dgrad_fold_kernel adds up to nine of those 16-bit values per pixel in
    fp32 (the transpose of ReflectionPad2d(3); integers, exact in any order) and stores fp32 or, dx_is16, RNE again.
    dx32 = sum RNE(padded terms); dx16 = RNE(dx32).  dy and w are converted to 16 bits on the way in (exact here or, where a
    test asks for it, RNE: pass the problem with the rounded operands)."""
    import torch.nn.functional as F
    wt = P.w.double().permute(3, 2, 0, 1).contiguous()                                   # [Cout, Cin, kh, kw]
    dxpad = F.conv_transpose2d(R.to_nchw(P.dy.double()), wt)                             # [B, 64, H + 6, W + 6]
    dxpad16 = rne16(dxpad, td).double()
    xz = torch.zeros(P.x.shape[0], P.x.shape[3], P.x.shape[1], P.x.shape[2], dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(F.pad(xz, (3, 3, 3, 3), mode="reflect"), xz, dxpad16)
    dx32 = R.to_nhwc(g)
    return rne16(dx32, td) if dx16 else dx32


# ------------------------------------------------------------------------------------------------ the conversion kernels' corner table
def corner_table(td):
    """One fixed table of fp32 values (built from bit patterns) for the fp32 -> 16-bit conversion kernels: ties to even in both
    directions at several exponents with the values just either side of each (incl. the tie that carries into the next
    exponent), the largest finite values, for fp16 65519.99.., 65520 and results that land on subnormals (the 2^-25 tie to
    zero and its neighbours among them), fp32 subnormals, +-0, +-inf, NaNs.  Starts with (below a tie, the tie, above it),
    and its length is 6 mod 8: table + table[:2] is a whole number of 8-element vectors whose LAST element is a tie."""
    import numpy as np
    drop = 16 if td is torch.bfloat16 else 13              # fp32 mantissa bits the type drops
    keep = 23 - drop
    exps = (-126, -60, -1, 0, 1, 7, 64, 127) if td is torch.bfloat16 else (-14, -5, 0, 1, 10, 15)
    bits = []
    for e in exps:
        for hi in (0, 1, (1 << keep) - 2, (1 << keep) - 1):            # kept mantissa even / odd / odd with a carry out of the mantissa
            tie = ((e + 127) << 23) | (hi << drop) | (1 << (drop - 1))
            for sign in (0, 0x80000000):
                bits += [(tie - 1) | sign, tie | sign, (tie + 1) | sign]
    if td is torch.float16:
        bits += [0x477FE000, 0x477FEFFF, 0x477FF000, 0x477FF001, 0x47800000, 0xC77FEFFF, 0xC77FF000]      # 65504, 65519.99.., 65520 ..
        for k in (0, 1, 2, 5, 511, 1022, 1023):                                                              # (k + 1/2) 2^-24: subnormal ties
            v = np.float32((k + 0.5) * 2.0 ** -24)
            for f in (np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(1))):
                b = int(np.float32(f).view(np.uint32))
                bits += [b, b | 0x80000000]
        bits += [0x33800000, 0x33000000 - (1 << 23), 0x387FC000]                                            # 2^-24, 2^-26, the largest subnormal
    else:
        bits += [0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000]                              # around the largest finite bf16
        bits += [0x00008000, 0x00007FFF, 0x00008001, 0x00018000, 0x00010000, 0x80008000]                  # bf16 subnormals and their ties
    bits += [0x00000001, 0x007FFFFF, 0x80000001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001]
    while len(bits) % 8 != 6:
        bits.append(0x80000000 if len(bits) % 2 else 0)
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())
