"""float64 numpy restatement of the sampling rule of mmh_decode_inputs_resized, shared by the CPU test that pins it to
torch.nn.functional.interpolate and the GPU tests that hold the kernel to it.

Per output pixel (half-pixel centres, edge clamp): sx = (x + 0.5) * Ws / Wo - 0.5 clamped below at 0, x0 = floor(sx),
x1 = min(x0 + 1, Ws - 1), weight sx - x0; the same in y.  Joints: u' = (u + 0.5) * Wo / Ws - 0.5, v' likewise."""
import numpy as np


def taps(n_src, n_out):
    s = (np.arange(n_out, dtype=np.float64) + 0.5) * n_src / n_out - 0.5
    s = np.maximum(s, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_src - 1)
    i1 = np.minimum(i0 + 1, n_src - 1)
    return i0, i1, s - i0


def bilinear(a, Ho, Wo):
    """a: float64 [..., Hs, Ws] -> float64 [..., Ho, Wo]"""
    a = np.asarray(a, dtype=np.float64)
    y0, y1, wy = taps(a.shape[-2], Ho)
    x0, x1, wx = taps(a.shape[-1], Wo)
    wy = wy[:, None]
    top = a[..., y0, :][..., :, x0] * (1.0 - wx) + a[..., y0, :][..., :, x1] * wx
    bot = a[..., y1, :][..., :, x0] * (1.0 - wx) + a[..., y1, :][..., :, x1] * wx
    return top * (1.0 - wy) + bot * wy


def scale_joints(uv, src, dst):
    """uv [..., 2] (u, v) on the Hs x Ws grid -> on the Ho x Wo grid, float64"""
    (Hs, Ws), (Ho, Wo) = src, dst
    out = np.array(uv, dtype=np.float64, copy=True)
    out[..., 0] = (out[..., 0] + 0.5) * float(Wo) / float(Ws) - 0.5
    out[..., 1] = (out[..., 1] + 0.5) * float(Ho) / float(Hs) - 0.5
    return out


def decode_resized(img_bgr, dep_bgr, Ho, Wo):
    """uint8 [Hs,Ws,3] BGR image and depth PNG -> float64 (H [3,Ho,Wo] RGB in [-1,1], D [Ho,Wo]): the taps combined from
    the raw bytes (colour per channel; depth as 256 G + R per tap), then the loader's normalisation
    (data/generic_dataset.py:140-158), all in float64 - nothing rounded on the way"""
    rgb = bilinear(img_bgr[:, :, ::-1].astype(np.float64).transpose(2, 0, 1), Ho, Wo)
    h = ((rgb / 255.0) - 0.5) / 0.5
    raw = 256.0 * dep_bgr[:, :, 1].astype(np.float64) + dep_bgr[:, :, 2].astype(np.float64)
    d = ((bilinear(raw, Ho, Wo) / 700.0) - 0.5) / 0.5
    return h, d


def f32_tolerance(want64):
    """'within 1 ulp of the float64 result rounded to fp32': the fp32 spacing at the expected value, plus the distance two
    float64 evaluations of the same formula may keep - the taps' products are summed in another order, a few 2^-53 of the
    interpolated value (< 2^16), and the `- 0.5` of the normalisation turns that relative error into an absolute one:
    65536 / 700 * 2 * 4 * 2^-53 < 1e-13.  Without that term an expected 0.0 would admit nothing but 0.0."""
    w32 = np.asarray(want64, dtype=np.float64).astype(np.float32)
    return w32, np.spacing(np.abs(w32)).astype(np.float64) + 1e-13
