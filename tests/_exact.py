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
