"""float64 numpy restatement of mmh_hpe_augment_normalize (train_hpe --augment_geom / --augment_color), on
tests/_affine_oracle.warp, shared by the CPU tests that pin the host's colour maths and the GPU tests that hold the kernel to it.

Per image and output pixel, everything in float64 (include/mmhand_hip.h at the entry point):
 1. sample R, G, B through the matrix A with _affine_oracle's rule (coordinates without contraction, edge replicate, four taps
    of the raw bytes);
 2. v_c = (cm[c,0] R + cm[c,1] G) + cm[c,2] B, each product and sum rounded on its own, clamped to [0, 255] (a NaN to 0);
 3. gamma != 1: v_c = 255 * np.power(v_c / 255, gamma);
 4. mn / mx over the output pixels and the three channels; (v - mn) / (mx - mn); mx == mn gives zeros.

The colour matrix is built here a second, independent way - not from data.color_matrix's closed forms: `jitter` acts on
pixels, as grey + s (rgb - grey) with grey = 0.299 R + 0.587 G + 0.114 B, then a rotation by the hue angle written in an
orthonormal basis (e1, e2, n) with n = (1,1,1) / sqrt(3), then the gains; `matrix` is `jitter` of the three unit vectors.  The
two check each other.

Tolerance (`tolerance`), the way _affine_oracle.f32_tolerance derives its own: the fp32 spacing at the expected value - the
kernel rounds once, at the store - plus the distance two float64 evaluations of the same formula may keep:
  * the coordinates, taps and weights are identical in both (no contraction).  The tap combination passes a value through at
    most six roundings (1 - wx, a product, a sum, 1 - wy, a product, a sum), each at most 2^-53 relative to a magnitude of at
    most 255; a device evaluation that fuses some of them and this one each stay within 6 * 255 * 2^-53 of the exact value, so
    R, G, B differ by at most e_tap = 12 * 255 * 2^-53 = 3.4e-13;
  * the matrix row is the same five operations in both (three products, two sums, no contraction) on inputs that differ by
    e_tap: that difference comes out multiplied by at most r = the largest row sum of |cm| (at least 1), and each of the five
    roundings is at most 2^-53 relative to a magnitude of at most 255 r, in either evaluation: e_v = (12 + 10) * 255 * r * 2^-53.
    The clamp does not widen a difference;
  * gamma != 1: the curve f(v) = 255 (v / 255)^g carries e_v through with its slope.  For g > 1 the slope is at most g (at
    255).  For g < 1 it is at most g 255^(1 - g) on v >= 1 but unbounded towards 0, where the curve is Hoelder continuous
    instead: |f(a) - f(b)| <= 255 (|a - b| / 255)^g; an expected v below 1 takes that bound (7.6e-10 at g = 0.8, r = 1: the
    clamp may hold one evaluation at 0 where the other keeps a rounding error's worth above it).  On top, pow itself:
    OpenCL's bound for double-precision pow is 16 ulp, on a result of magnitude at most 255, in each of the two
    evaluations, and the division and the product around it are one rounding each: (2 * 16 + 4) * 255 * 2^-53 = 1.0e-12;
  * the normalisation: out = (v - mn) / (mx - mn) moves by at most (e(v) + 2 e(mn) + e(mx)) / (mx - mn) for |v - mn| <= mx -
    mn, e() being the bounds above at that element; its own subtraction and division round a value of at most 1 twice per
    evaluation: 4 * 2^-53.
CONDITION: every toleranced case has an oracle range mx - mn >= MIN_RANGE = 32 (asserted by the tests, on the CPU too), so that
the division cannot hide an error: with it the float64 term stays below 1e-13 without gamma and below 2e-10 with it."""
import numpy as np

from tests import _affine_oracle as AO

MIN_RANGE = 32.0
LUMA = np.array([0.299, 0.587, 0.114])
IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


# ----------------------------------------------------------------------------- the colour jitter, per pixel
def jitter(rgb, saturation, hue_deg, gains):
    """rgb float64 [..., 3] -> float64 [..., 3]: towards / away from the luma grey, a turn about the grey axis, gains"""
    rgb = np.asarray(rgb, dtype=np.float64)
    grey = (rgb * LUMA).sum(-1, keepdims=True)
    v = grey + saturation * (rgb - grey)
    n = np.ones(3) / np.sqrt(3.0)
    e1 = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
    e2 = np.cross(n, e1)                                            # (e1, e2, n) right-handed
    a, b, c = v @ e1, v @ e2, v @ n
    t = np.deg2rad(hue_deg)
    a2, b2 = a * np.cos(t) - b * np.sin(t), a * np.sin(t) + b * np.cos(t)
    v = a2[..., None] * e1 + b2[..., None] * e2 + c[..., None] * n
    return v * np.asarray(gains, dtype=np.float64)


def matrix(saturation, hue_deg, gains):
    """the 3x3 matrix of `jitter` on column vectors (R, G, B): its images of the unit vectors are the columns"""
    return jitter(np.eye(3), saturation, hue_deg, gains).T


# ----------------------------------------------------------------------------- the pass
def values(img_bgr, A=None, cm=None, gamma=None, out=None):
    """uint8 [Hs,Ws,3] BGR -> float64 [3,Ho,Wo] = R, G, B after steps 1-3 (before the normalisation)"""
    img_bgr = np.asarray(img_bgr)
    assert img_bgr.dtype == np.uint8 and img_bgr.ndim == 3 and img_bgr.shape[2] == 3
    Ho, Wo = out or img_bgr.shape[:2]
    rgb = img_bgr[:, :, ::-1].astype(np.float64).transpose(2, 0, 1)
    R, G, B = AO.warp(rgb, IDENTITY if A is None else A, Ho, Wo)
    if cm is not None:
        m = np.asarray(cm, dtype=np.float64).reshape(3, 3)
        v = np.stack([(m[c, 0] * R + m[c, 1] * G) + m[c, 2] * B for c in range(3)])
    else:
        v = np.stack([R, G, B])
    v = np.where(v > 0.0, v, 0.0)                                   # a NaN compares false: 0
    v = np.where(v < 255.0, v, 255.0)
    if gamma is not None and float(gamma) != 1.0:
        v = 255.0 * np.power(v / 255.0, float(gamma))
    return v


def normalize(v):
    """float64 [3,Ho,Wo] -> (float64 [Ho,Wo,3] in [0, 1], mx - mn)"""
    mn, mx = v.min(), v.max()
    out = (v - mn) / (mx - mn) if mx > mn else np.zeros_like(v)
    return out.transpose(1, 2, 0), float(mx - mn)


def augment_normalize(img_bgr, A=None, cm=None, gamma=None, out=None):
    """-> (float64 [Ho,Wo,3] = lanes 0..2 of the kernel's output before its one rounding, the range mx - mn)"""
    return normalize(values(img_bgr, A, cm, gamma, out))


def tolerance(img_bgr, A=None, cm=None, gamma=None, out=None):
    """-> (want fp32 [Ho,Wo,3], tol float64 [Ho,Wo,3], range): see the module docstring"""
    u = 2.0 ** -53
    v = values(img_bgr, A, cm, gamma, out)
    r = 1.0 if cm is None else max(1.0, float(np.abs(np.asarray(cm, dtype=np.float64).reshape(3, 3)).sum(1).max()))
    e_v = (12.0 + 10.0) * 255.0 * r * u
    g = 1.0 if gamma is None else float(gamma)
    if g == 1.0:
        e = np.full(v.shape, e_v)
    else:
        pre = values(img_bgr, A, cm, None, out)                     # the curve's argument
        if g > 1.0:
            e = np.full(v.shape, g * e_v)
        else:
            e = np.where(pre >= 1.0, g * 255.0 ** (1.0 - g) * e_v, 255.0 * (e_v / 255.0) ** g)
        e = e + (2 * 16 + 4) * 255.0 * u
    want, rng = normalize(v)
    if rng <= 0.0:
        return want.astype(np.float32), np.zeros(want.shape), rng
    e_mn, e_mx = e.flat[int(v.argmin())], e.flat[int(v.argmax())]
    f64 = (e + 2.0 * e_mn + e_mx) / rng + 4.0 * u
    w32 = want.astype(np.float32)
    return w32, np.spacing(np.abs(w32)).astype(np.float64) + f64.transpose(1, 2, 0), rng


# ----------------------------------------------------------------------------- fixtures
def images(B, H, W, seed, lo=0, hi=256):
    """uint8 [B,H,W,3] BGR with bytes in [lo, hi), seeded"""
    rs = np.random.RandomState(seed)
    return rs.randint(lo, hi, size=(B, H, W, 3)).astype(np.uint8)


def blob_image(H, W, u, v):
    """one 3x3 white blob centred on the joint (u, v) of a black H x W image, uint8 BGR"""
    img = np.zeros((H, W, 3), dtype=np.uint8)
    img[v - 1:v + 2, u - 1:u + 2] = 255
    return img


# ----------------------------------------------------------------------------- the toleranced cases, shared by CPU and GPU tests
SRC = (24, 40)                                                      # rows != columns
# (theta in degrees, scale, tx, ty, flip) of the three images of a batch: inside and beyond the default ranges
DRAWS = [(12.0, 1.08, 0.04, -0.03, False), (-35.0, 0.8, -0.1, 0.07, True), (171.0, 1.3, 0.0, 0.2, False)]
# (saturation, hue in degrees, gains) inside the default ranges 0.3 / 10 / 0.1
COLORS = [(1.25, 8.0, (1.07, 0.93, 1.0)), (0.72, -9.5, (0.91, 1.1, 1.04)), (1.0, 4.0, (1.0, 1.0, 0.95))]
GAMMAS = [0.8, 1.25, 0.8]


def cases():
    """[(name, images uint8 [B,24,40,3], A float64 [B,2,3] | None, cm float64 [B,3,3] | None, gamma float64 [B] | None, out)]:
    B = 3 with three different matrices and colour rows (per-image indexing), outputs 24 x 40 and 16 x 24, and one image whose
    136 x 128 output is more than the 64 x 256 pixels one round of the reduction's chunks covers (a second turn of its loop)"""
    img = images(3, *SRC, seed=21)
    out = []
    for dst in (SRC, (16, 24)):
        A = np.stack([AO.inverse(AO.forward(*d, SRC), SRC, dst) for d in DRAWS])
        cm = np.stack([matrix(*c) for c in COLORS])
        tag = "%dx%d" % dst
        out.append(("geom_" + tag, img, A, None, None, dst))
        out.append(("all_" + tag, img, A, cm, np.array(GAMMAS), dst))
    out.append(("color", img, None, np.stack([matrix(*c) for c in COLORS]), None, SRC))
    out.append(("gamma", img, None, None, np.array(GAMMAS), SRC))
    big = (136, 128)
    out.append(("second_turn", img[:1], AO.inverse(AO.forward(*DRAWS[0], SRC), SRC, big)[None], matrix(*COLORS[0])[None],
                np.array(GAMMAS[:1]), big))
    return out
