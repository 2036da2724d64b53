"""Image quality metrics on the device: SSIM (pytorch_ssim/__init__.py:17-37, one image at a time as the reference's
Evaluator calls it, utils.py:100-111), mean |a-b|, mean (a-b)^2 and PSNR of image pairs, from one pass of
mmh_image_metrics (csrc/metrics.hip).

Both images of a pair are mapped to [0, 1] before anything is computed:

* ``range="pm1"``: generator output / decoded images in [-1, 1], ``(x + 1) / 2``; fp32, bf16 or fp16 [B,C,H,W] with any
  strides (an NCHW view of an NHWC buffer included);
* ``range="unit"``: values already in [0, 1];
* ``range="u8_bgr_hwc"``: 8-bit pixels [B,H,W,3] in B,G,R order (as the loader reads PNGs), ``u8 / 255``, scored as RGB.

This is the range a written PNG represents, so scoring the generator's tensors and scoring the PNGs aug.py wrote agree up
to quantisation.  (The reference's bench_poseTransfer.py compares a tanh output in [-1, 1] with a target in [0, 1]; that
mismatch is deliberately not reproduced.)  SSIM is the reference's formula with its window (11 taps, sigma 1.5, zero
padding, C1 = 0.01^2, C2 = 0.03^2) and is within 1e-6 of that formula evaluated in float64.  PSNR = 10 log10(1 / MSE),
+inf when MSE is 0.  Every per-image value is float64 and bit-identical from run to run.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import lib as L
from .ops import _ptr, _stream

C1, C2, SIGMA = 0.01 ** 2, 0.03 ** 2, 1.5
RANGES = {"pm1": (0.5, 0.5), "unit": (1.0, 0.0), "u8_bgr_hwc": (1.0 / 255.0, 0.0)}
_DTYPES = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.FP16}
_taps = {}


def gaussian_taps(window, sigma=SIGMA):
    """The 1-D window exactly as pytorch_ssim.gaussian builds it (:7-9): exp in float64, rounded to fp32, divided by the
    fp32 sum - torch's own summation, whose last bit the result depends on."""
    key = (int(window), float(sigma))
    if key not in _taps:
        g = torch.tensor([math.exp(-(x - window // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window)],
                         dtype=torch.float32)
        _taps[key] = np.ascontiguousarray((g / g.sum()).numpy())
    return _taps[key]


def _check_window(window):
    if not (isinstance(window, int) and 3 <= window <= 15 and window % 2 == 1):
        raise ValueError(f"window {window!r}: odd, from 3 to 15")


def _src(t, rng):
    """(mmh_image_src, B, C, H, W) of one side of the pair; the tensor must stay alive until the launch is enqueued."""
    scale, offset = RANGES[rng]
    if not t.is_cuda:
        raise ValueError("image_metrics: expected CUDA tensors")
    if rng == "u8_bgr_hwc":
        if t.dim() == 3:
            t = t.unsqueeze(0)
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
            raise ValueError(f"range 'u8_bgr_hwc': expected uint8 [B,H,W,3], got {t.dtype} {tuple(t.shape)}")
        B, H, W, Cc = t.shape
        sb, sh, sw, sc = t.stride()
        ptr = t.data_ptr() + (Cc - 1) * sc                       # channel 0 of the RGB view = the last byte (R)
        src = L.ImageSrc(ptr, L.U8, scale, offset, sb, -sc, sh, sw)
    else:
        if t.dim() == 3:
            t = t.unsqueeze(0)
        if t.dtype not in _DTYPES or t.dim() != 4:
            raise ValueError(f"range {rng!r}: expected fp32 / bf16 / fp16 [B,C,H,W], got {t.dtype} {tuple(t.shape)}")
        B, Cc, H, W = t.shape
        sb, sc, sh, sw = t.stride()
        src = L.ImageSrc(t.data_ptr(), _DTYPES[t.dtype], scale, offset, sb, sc, sh, sw)
    return src, (B, Cc, H, W)


@torch.no_grad()
def image_metrics(a, b, range="pm1", window=11):
    """Per-image metrics of the pairs (a[i], b[i]) -> dict of float64 device tensors [B]: ssim, l1, mse, psnr.
    Enqueued on the current stream; nothing is synchronised."""
    if range not in RANGES:
        raise ValueError(f"range {range!r}: one of {sorted(RANGES)}")
    _check_window(window)
    sa, shape = _src(a, range)
    sb, shape_b = _src(b, range)
    if shape != shape_b or a.device != b.device:
        raise ValueError(f"image_metrics: shapes differ, {shape} vs {shape_b} (or devices {a.device} / {b.device})")
    B, Cc, H, W = shape
    lib = L.load()
    nbytes = lib.mmh_image_metrics_ws_bytes(B, Cc, H, W, window)
    if nbytes == 0:
        raise ValueError(f"image_metrics: shape {shape} / window {window} refused")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
    out = torch.empty((B, 3), dtype=torch.float64, device=a.device)
    taps = gaussian_taps(window)
    L.call("mmh_image_metrics", C.byref(sa), C.byref(sb), B, Cc, H, W, window, taps.ctypes.data_as(C.c_void_p), C1, C2,
           _ptr(ws), nbytes, _ptr(out), _stream())
    mse = out[:, 2]
    return {"ssim": out[:, 0], "l1": out[:, 1], "mse": mse, "psnr": -10.0 * torch.log10(mse)}


def ssim(a, b, range="pm1", window=11):
    """Per-image SSIM [B] (float64, device)."""
    return image_metrics(a, b, range=range, window=window)["ssim"]


class QualityMeter:
    """Accumulates per-image metrics over batches; ``result()`` gives the summary under the reference Evaluator's keys
    (utils.py:63-70: SSIM_avg, SSIM_std as np.std) plus L1_avg, PSNR_avg (over the images with a finite PSNR), n, and
    the per-image rows.  The per-image columns are the COLUMNS table; a further metric is one more column and one more
    summary entry.  ``feed`` only enqueues: the values are read back in ``result()``."""

    COLUMNS = ("ssim", "l1", "mse", "psnr")

    def __init__(self, range="pm1", window=11):
        if range not in RANGES:
            raise ValueError(f"range {range!r}: one of {sorted(RANGES)}")
        _check_window(window)
        self.range, self.window = range, window
        self._batches = []

    def feed(self, pred, target, paths=None):
        """pred, target: one batch in this meter's range.  paths: None or one dict per image (e.g. {"target": ...,
        "source": ...}), copied into that image's row."""
        m = image_metrics(pred, target, range=self.range, window=self.window)
        n = m["ssim"].shape[0]
        if paths is not None and len(paths) != n:
            raise ValueError(f"feed: {len(paths)} paths for {n} images")
        self._batches.append((torch.stack([m[k] for k in self.COLUMNS], 1), paths))

    def rows(self):
        out = []
        for vals, paths in self._batches:
            v = vals.cpu().numpy()
            for i in range(v.shape[0]):
                row = dict(paths[i]) if paths is not None else {}
                row.update({k: float(v[i, j]) for j, k in enumerate(self.COLUMNS)})
                out.append(row)
        return out

    @staticmethod
    def summarize(rows):
        s = np.array([r["ssim"] for r in rows], dtype=np.float64)
        l1 = np.array([r["l1"] for r in rows], dtype=np.float64)
        psnr = np.array([r["psnr"] for r in rows], dtype=np.float64)
        finite = psnr[np.isfinite(psnr)]
        return {"SSIM_avg": float(np.mean(s)) if len(s) else None, "SSIM_std": float(np.std(s)) if len(s) else None,
                "L1_avg": float(np.mean(l1)) if len(l1) else None,
                "PSNR_avg": float(np.mean(finite)) if len(finite) else None, "n": len(rows)}

    def result(self):
        rows = self.rows()
        return {"summary": self.summarize(rows), "rows": rows}
