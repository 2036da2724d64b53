"""CPU rounding model (numpy, no GPU): F(2x2,3x3) with two-level summation in its 16 GEMMs against the direct two-level
implicit GEMM, relative L1 to float64, per contraction depth.  Both sum fresh fp32 chains of 32 contraction elements that are
folded into a running total; the direct conv walks (tap, channel) = 9 * Cin elements, the Winograd GEMMs Cin per plane.
The Winograd side adds the fp32 roundings of its transforms (input: one subtraction per dimension, filter: two additions and
a halving per dimension, output: two additions per dimension) - a floor that does not shrink with Cin, while the direct
kernel's chain error does.  So the ratio of the two errors GROWS as Cin falls; the per-conv test bars follow this table.

    python tools/wino2_error_model.py [--seeds 3]
"""
import argparse
import numpy as np
ap = argparse.ArgumentParser(); ap.add_argument("--seeds", type=int, default=3); a = ap.parse_args()
f32 = np.float32
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], f32)
G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], f32)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], f32)
T, N = 256, 16


def mm32(A, x, axis):
    """fp32 matrix-times-tensor along one axis with a rounding after every addition (coefficients are exact)"""
    x = np.moveaxis(x, axis, 0)
    out = []
    for row in A:
        acc = None
        for c, xi in zip(row, x):
            if c == 0:
                continue
            t = (f32(c) * xi).astype(f32)
            acc = t if acc is None else (acc + t).astype(f32)
        out.append(acc)
    return np.moveaxis(np.stack(out), 0, axis)


def two_level(terms):
    """terms [K, ...] fp32 products' operands already multiplied in float64 (the MFMA rounds once per accumulate): chains of 32"""
    total = np.zeros(terms.shape[1:], f32)
    for k0 in range(0, terms.shape[0], 32):
        part = np.zeros(terms.shape[1:], f32)
        for k in range(k0, min(k0 + 32, terms.shape[0])):
            part = (part.astype(np.float64) + terms[k]).astype(f32)      # fused multiply-add: one rounding
        total = (total + part).astype(f32)
    return total


print("Cin : direct two-level | F(2x2) two-level | ratio   (relative L1 to float64, %d seeds)" % a.seeds)
for K in (512, 256, 128, 64, 32):
    ed, ew = [], []
    for s in range(a.seeds):
        r = np.random.default_rng(s)
        d = r.uniform(-1, 1, (T, 4, 4, K)).astype(f32)
        g = (r.uniform(-1, 1, (3, 3, K, N)) * 0.05).astype(f32)
        d64, g64 = d.astype(np.float64), g.astype(np.float64)
        ref = sum(np.einsum("tijk,kn->tijn", d64[:, p:p + 2, q:q + 2], g64[p, q]) for p in range(3) for q in range(3))
        terms = np.concatenate([np.einsum("tijk,kn->ktijn", d64[:, p:p + 2, q:q + 2], g64[p, q]) for p in range(3) for q in range(3)])
        ed.append(np.abs(two_level(terms) - ref).sum() / np.abs(ref).sum())
        V = mm32(BT, mm32(BT, d, 1), 2)                     # [T,4,4,K]
        U = mm32(G, mm32(G, g, 0), 1)                       # [4,4,K,N]
        M = two_level(np.einsum("tijk,ijkn->ktijn", V.astype(np.float64), U.astype(np.float64)))
        y = mm32(AT, mm32(AT, M, 1), 2)
        ew.append(np.abs(y - ref).sum() / np.abs(ref).sum())
    print(f"{K:4d}: {np.mean(ed):.3e} | {np.mean(ew):.3e} | {np.mean(ew) / np.mean(ed):.3f}", flush=True)
