"""float64 numpy restatement of the sampling rule of mmh_decode_inputs_affine / mmh_decode_inputs_indexed_affine
(--augment_geom), shared by the CPU test that pins it to torch.nn.functional.grid_sample and the GPU tests that hold the
kernels to it.  The matrix builders here are written independently of mmhand_amd/data.py (3x3 homogeneous matrices and
numpy's general inverse, where data.py has closed forms), so that the two check each other.

Per output pixel (x, y) and matrix A = [a00 a01 a02; a10 a11 a12]: sx = (a00 x + a01 y) + a02, sy = (a10 x + a11 y) + a12,
each product and sum rounded on its own; clamped to [0, Ws - 1] x [0, Hs - 1] (a NaN to 0); x0 = min(floor(sx), Ws - 1),
x1 = min(x0 + 1, Ws - 1), weight sx - x0, the same in y; the four taps combined as tests/_resize_oracle.py combines them."""
import numpy as np

MAX_RAW_DEPTH = 767.0       # the largest 256 G + R of the fixtures (G <= 2, R <= 255)


def coords(A, Ho, Wo):
    """-> (sx, sy) float64 [Ho, Wo], unclamped"""
    A = np.asarray(A, dtype=np.float64).reshape(2, 3)
    y, x = np.mgrid[0:Ho, 0:Wo].astype(np.float64)
    sx = (A[0, 0] * x + A[0, 1] * y) + A[0, 2]
    sy = (A[1, 0] * x + A[1, 1] * y) + A[1, 2]
    return sx, sy


def outside_share(A, src, dst):
    """share of the output pixels whose source coordinate lies outside the image (the ones the clamp moves)"""
    (Hs, Ws), (Ho, Wo) = src, dst
    sx, sy = coords(A, Ho, Wo)
    return float(((sx < 0) | (sx > Ws - 1) | (sy < 0) | (sy > Hs - 1)).mean())


def _tap(s, n):
    s = np.where(s > 0.0, s, 0.0)                   # a NaN compares false: 0
    s = np.where(s < n - 1.0, s, n - 1.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    return i0, i1, s - i0


def warp(a, A, Ho, Wo):
    """a: float64 [..., Hs, Ws] -> float64 [..., Ho, Wo] sampled through A"""
    a = np.asarray(a, dtype=np.float64)
    sx, sy = coords(A, Ho, Wo)
    x0, x1, wx = _tap(sx, a.shape[-1])
    y0, y1, wy = _tap(sy, a.shape[-2])
    top = a[..., y0, x0] * (1.0 - wx) + a[..., y0, x1] * wx
    bot = a[..., y1, x0] * (1.0 - wx) + a[..., y1, x1] * wx
    return top * (1.0 - wy) + bot * wy


def decode_affine(img_bgr, dep_bgr, A, Ho, Wo):
    """uint8 [Hs,Ws,3] BGR image and depth PNG -> float64 (H [3,Ho,Wo] RGB in [-1,1], D [Ho,Wo]): taps from the raw bytes
    (colour per channel; depth as 256 G + R per tap), then the loader's normalisation, nothing rounded on the way"""
    rgb = warp(img_bgr[:, :, ::-1].astype(np.float64).transpose(2, 0, 1), A, Ho, Wo)
    h = ((rgb / 255.0) - 0.5) / 0.5
    raw = 256.0 * dep_bgr[:, :, 1].astype(np.float64) + dep_bgr[:, :, 2].astype(np.float64)
    d = ((warp(raw, A, Ho, Wo) / 700.0) - 0.5) / 0.5
    return h, d


# ----------------------------------------------------------------------------- matrices, as 3x3 homogeneous products
def _h(m):
    return np.vstack([np.asarray(m, dtype=np.float64).reshape(2, 3), [0.0, 0.0, 1.0]])


def forward(theta_deg, scale, tx, ty, flip, src):
    """p' = c + t + s R(theta) F (p - c) on the Hs x Ws grid, [2,3]"""
    Hs, Ws = src
    q = (theta_deg / 90.0) % 4
    if q == int(q):                                 # quarter turns are exact
        cos, sin = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][int(q)]
    else:
        cos, sin = np.cos(np.deg2rad(theta_deg)), np.sin(np.deg2rad(theta_deg))
    cx, cy = (Ws - 1) / 2.0, (Hs - 1) / 2.0
    to_centre = _h([[1, 0, -cx], [0, 1, -cy]])
    F = _h([[-1.0 if flip else 1.0, 0, 0], [0, 1, 0]])
    R = _h([[scale * cos, -scale * sin, 0], [scale * sin, scale * cos, 0]])
    back = _h([[1, 0, cx + tx * Ws], [0, 1, cy + ty * Hs]])
    return (back @ R @ F @ to_centre)[:2]


def resize_map(src, dst):
    """u' = (u + 0.5) Wo / Ws - 0.5, v' likewise, [2,3]"""
    (Hs, Ws), (Ho, Wo) = src, dst
    return np.array([[Wo / Ws, 0.0, 0.5 * Wo / Ws - 0.5], [0.0, Ho / Hs, 0.5 * Ho / Hs - 0.5]])


def inverse(fwd, src, dst):
    """the sampling matrix: output pixel -> source coordinate = inverse of (fwd, then the resize map), [2,3]"""
    return np.linalg.inv(_h(resize_map(src, dst)) @ _h(fwd))[:2]


def joints(uv, fwd, src, dst):
    """uv [..., 2 or 3] through fwd and the resize map; further components unchanged"""
    m = _h(resize_map(src, dst)) @ _h(fwd)
    out = np.array(uv, dtype=np.float64, copy=True)
    u, v = out[..., 0].copy(), out[..., 1].copy()
    out[..., 0] = m[0, 0] * u + m[0, 1] * v + m[0, 2]
    out[..., 1] = m[1, 0] * u + m[1, 1] * v + m[1, 2]
    return out


def f32_tolerance(want64):
    """'within 1 ulp of the float64 result rounded to fp32': the fp32 spacing at the expected value, plus the distance two
    float64 evaluations of the same formula may keep.  The coordinates, and with them taps and weights, are identical in
    both (no contraction); the tap combination is not: (1 - wy) * ((1 - wx) * v00 + wx * v01) + wy * (...) passes a value
    through at most six roundings - 1 - wx, a product, a sum, 1 - wy, a product, a sum -, each at most 2^-53 relative to a
    magnitude of at most the largest raw value, 767 (G <= 2: tests/_resize_oracle.py's argument had 65536 there).  A device
    evaluation that fuses some of them and this one each stay within 6 * 767 * 2^-53 of the exact value, so they differ by
    at most 12 * 767 * 2^-53 = 1.03e-12 before the normalisation and 2 / 700 of that, 2.9e-15, after it; the
    normalisation's own roundings (/ 700, - 0.5, / 0.5 on magnitudes <= 2.2) add 4 * 2.2 * 2^-53 < 1e-15 over both
    evaluations.  Together < 4e-15 (colour, 255 / 255, is smaller).  Without that term an expected 0.0 would admit
    nothing but 0.0."""
    w32 = np.asarray(want64, dtype=np.float64).astype(np.float32)
    return w32, np.spacing(np.abs(w32)).astype(np.float64) + 4e-15
