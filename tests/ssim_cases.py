"""Deterministic SSIM test images (numpy.RandomState), float32 in [-1, 1], shared by tests/golden/make_ssim_golden.py and
the GPU tests.  Each case is a pair (a, b) of [N, C, H, W] batches; the flat and saturated cases are the ones where the
reference's formula loses precision in fp32 (sigma^2 = E[x^2] - mu^2 cancels against C2)."""
import numpy as np

KINDS = ("uniform", "close", "smooth", "flat", "saturated", "identical")
SHAPES = ((3, 256, 256), (3, 67, 45), (1, 16, 16), (3, 9, 9))
WINDOWS = (11, 7)
N = 2      # images per case


def _smooth(rs, shape):
    x = rs.uniform(-1, 1, size=shape)
    for axis in (-1, -2):                      # a few box blurs: correlated, slowly varying fields
        for _ in range(3):
            x = (np.roll(x, 1, axis) + x + np.roll(x, -1, axis)) / 3.0
    return np.clip(x * 3.0, -1, 1)


def make_case(kind, shape, seed=0):
    rs = np.random.RandomState(KINDS.index(kind) * 1000 + SHAPES.index(shape) * 10 + seed)
    full = (N,) + tuple(shape)
    if kind == "uniform":
        a, b = rs.uniform(-1, 1, full), rs.uniform(-1, 1, full)
    elif kind == "close":
        a = rs.uniform(-1, 1, full)
        b = a + 0.05 * rs.standard_normal(full)
    elif kind == "smooth":
        a, b = _smooth(rs, full), _smooth(rs, full)
    elif kind == "flat":
        base = np.where(np.arange(full[-1]) < full[-1] // 2, 0.98, 0.999) * np.ones(full)
        a = base + 1e-3 * rs.standard_normal(full)
        b = base + 1e-3 * rs.standard_normal(full)
    elif kind == "saturated":
        # tanh output at both ends: a -1 background with a +1 block, 5e-4 noise pointing inwards (a -1 background alone
        # maps to 0 in [0, 1], where E[x^2] - mu^2 does not cancel; the +1 block is where it does)
        hi = np.zeros(full, dtype=bool)
        hi[..., full[-2] // 4:, full[-1] // 3:] = True
        a = np.where(hi, 1.0, -1.0) - np.where(hi, 5e-4, -5e-4) * np.abs(rs.standard_normal(full))
        b = np.where(hi, 1.0, -1.0) - np.where(hi, 5e-4, -5e-4) * np.abs(rs.standard_normal(full))
    elif kind == "identical":
        a = rs.uniform(-1, 1, full)
        b = a.copy()
    else:
        raise KeyError(kind)
    return np.clip(a, -1, 1).astype(np.float32), np.clip(b, -1, 1).astype(np.float32)


def cases():
    """(name, a, b, window) for every case, shape and window"""
    for kind in KINDS:
        for shape in SHAPES:
            a, b = make_case(kind, shape)
            for w in WINDOWS:
                yield f"{kind}_{'x'.join(map(str, shape))}_w{w}", a, b, w
