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

``image_metrics(..., mask=)`` (mmh_image_metrics_masked) also gives the means over a region - evaluate's hand region, from
``hand_mask`` - out of the same pass: the same zero-padded SSIM map, |a-b| and (a-b)^2, averaged over the mask's pixels.
This is NOT PATN's mask-SSIM, which multiplies both images by the mask first and scores the products over the whole frame;
hence the name "hand".  ``ms_ssim`` (mmh_ms_ssim) is multi-scale SSIM (Wang, Simoncelli, Bovik 2003): the contrast-structure
term of every level but the last and the SSIM of the last, each over the pixels whose window lies inside the image, 2 x 2
average pooling between levels, combined as prod pow(max(v_l, 0), w_l) per channel and averaged over the channels.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import lib as L
from .ops import _ptr, _stream

C1, C2, SIGMA = 0.01 ** 2, 0.03 ** 2, 1.5
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)            # Wang, Simoncelli, Bovik 2003, five scales
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


def _pair(fn, a, b, range, window):
    """both sides' descriptors and the common shape, after the argument checks the entry points share"""
    if range not in RANGES:
        raise ValueError(f"range {range!r}: one of {sorted(RANGES)}")
    _check_window(window)
    sa, shape = _src(a, range)
    sb, shape_b = _src(b, range)
    if shape != shape_b or a.device != b.device:
        raise ValueError(f"{fn}: shapes differ, {shape} vs {shape_b} (or devices {a.device} / {b.device})")
    return sa, sb, shape


@torch.no_grad()
def image_metrics(a, b, range="pm1", window=11, mask=None):
    """Per-image metrics of the pairs (a[i], b[i]) -> dict of float64 device tensors [B]: ssim, l1, mse, psnr.
    mask: None, or a bool / uint8 CUDA [B,H,W] of any strides (non-zero = inside, one mask for all channels of its image);
    then also ssim_hand, l1_hand, mse_hand, psnr_hand - the same maps averaged over the mask's pixels, NaN where it is
    empty - and mask_count, from the one pass of mmh_image_metrics_masked.  Enqueued on the current stream; nothing is
    synchronised."""
    sa, sb, shape = _pair("image_metrics", a, b, range, window)
    B, Cc, H, W = shape
    lib = L.load()
    taps = gaussian_taps(window)
    if mask is None:
        nbytes = lib.mmh_image_metrics_ws_bytes(B, Cc, H, W, window)
        if nbytes == 0:
            raise ValueError(f"image_metrics: shape {shape} / window {window} refused")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
        out = torch.empty((B, 3), dtype=torch.float64, device=a.device)
        L.call("mmh_image_metrics", C.byref(sa), C.byref(sb), B, Cc, H, W, window, taps.ctypes.data_as(C.c_void_p), C1, C2,
               _ptr(ws), nbytes, _ptr(out), _stream())
        mse = out[:, 2]
        return {"ssim": out[:, 0], "l1": out[:, 1], "mse": mse, "psnr": -10.0 * torch.log10(mse)}
    if not (torch.is_tensor(mask) and mask.is_cuda and mask.device == a.device and mask.dtype in (torch.bool, torch.uint8) and
            tuple(mask.shape) == (B, H, W)):
        raise ValueError(f"image_metrics: mask must be a bool / uint8 CUDA tensor {(B, H, W)} on the images' device")
    m8 = mask.view(torch.uint8) if mask.dtype == torch.bool else mask          # a bool is one byte, 0 or 1
    nbytes = lib.mmh_image_metrics_masked_ws_bytes(B, Cc, H, W, window)
    if nbytes == 0:
        raise ValueError(f"image_metrics: shape {shape} / window {window} refused")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
    out = torch.empty((B, 7), dtype=torch.float64, device=a.device)
    L.call("mmh_image_metrics_masked", C.byref(sa), C.byref(sb), m8.data_ptr(), *m8.stride(), B, Cc, H, W, window,
           taps.ctypes.data_as(C.c_void_p), C1, C2, _ptr(ws), nbytes, _ptr(out), _stream())
    mse, mse_hand = out[:, 2], out[:, 5]
    return {"ssim": out[:, 0], "l1": out[:, 1], "mse": mse, "psnr": -10.0 * torch.log10(mse),
            "ssim_hand": out[:, 3], "l1_hand": out[:, 4], "mse_hand": mse_hand, "psnr_hand": -10.0 * torch.log10(mse_hand),
            "mask_count": out[:, 6]}


def ms_ssim_min_side(window, levels):
    """mmh_ms_ssim's rule: min(H, W) must EXCEED this, so that the last level holds a whole window"""
    return (window - 1) * 2 ** (levels - 1)


@torch.no_grad()
def ms_ssim(a, b, range="pm1", window=11, weights=MS_WEIGHTS):
    """Multi-scale SSIM of the pairs (a[i], b[i]) over len(weights) levels (1 .. 5) -> {"ms_ssim": [B], "scales": [B,C,L]},
    float64 device tensors: scales[b][c][l] is the mean contrast-structure of level l (the mean SSIM at the last level) over the
    pixels whose window lies inside the image, unclamped; ms_ssim[b] = mean over c of prod over l of max(scales, 0) ** weights[l].
    min(H, W) must exceed (window - 1) * 2 ** (L - 1).  Enqueued on the current stream; nothing is synchronised."""
    sa, sb, shape = _pair("ms_ssim", a, b, range, window)
    B, Cc, H, W = shape
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
    levels = int(w.shape[0])
    if not (1 <= levels <= 5 and np.all(np.isfinite(w)) and np.all(w > 0)):
        raise ValueError(f"ms_ssim: weights {weights!r}: 1 to 5 finite values > 0")
    if min(H, W) <= ms_ssim_min_side(window, levels):
        raise ValueError(f"ms_ssim: shape {shape}: min(H, W) must exceed (window - 1) * 2 ** (levels - 1) = "
                         f"{ms_ssim_min_side(window, levels)}")
    lib = L.load()
    nbytes = lib.mmh_ms_ssim_ws_bytes(B, Cc, H, W, window, levels)
    if nbytes == 0:
        raise ValueError(f"ms_ssim: shape {shape} / window {window} / {levels} levels refused")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
    scales = torch.empty((B, Cc, levels), dtype=torch.float64, device=a.device)
    out = torch.empty((B,), dtype=torch.float64, device=a.device)
    taps = gaussian_taps(window)
    L.call("mmh_ms_ssim", C.byref(sa), C.byref(sb), B, Cc, H, W, window, taps.ctypes.data_as(C.c_void_p), C1, C2, levels,
           w.ctypes.data_as(C.c_void_p), _ptr(ws), nbytes, _ptr(scales), _ptr(out), _stream())
    return {"ms_ssim": out, "scales": scales}


@torch.no_grad()
def hand_mask(uv, size, radius):
    """The hand region of a pose: uint8 [B,H,W], 1 where one of the 20 bones, drawn as a capsule of `radius` pixels, covers the
    pixel.  uv: float64 [B,21,2] joints (u, v) on the scored grid; size = (H, W).  The coverage of ops.render_pose_depth (and so
    of tests/_render_oracle.py) with z = 0 and bg = 255: a covered pixel stores (0 / 255 - 0.5) / 0.5 = -1, the background +1."""
    from . import ops
    uv = torch.as_tensor(uv)
    if not (uv.is_cuda and uv.dtype == torch.float64 and uv.dim() == 3 and tuple(uv.shape[1:]) == (21, 2)):
        raise ValueError(f"hand_mask: uv must be a float64 CUDA tensor [B,21,2], got {uv.dtype} {tuple(uv.shape)}")
    xyz = torch.cat((uv, torch.zeros_like(uv[:, :, :1])), 2).contiguous()
    depth = ops.render_pose_depth(xyz, size=(int(size[0]), int(size[1])), radius=float(radius), bg=255.0)
    return (depth[..., 0] < 0).to(torch.uint8)


def ssim(a, b, range="pm1", window=11):
    """Per-image SSIM [B] (float64, device)."""
    return image_metrics(a, b, range=range, window=window)["ssim"]


class QualityMeter:
    """Accumulates per-image metrics over batches; ``result()`` gives the summary under the reference Evaluator's keys
    (utils.py:63-70: SSIM_avg, SSIM_std as np.std) plus L1_avg, PSNR_avg (over the images with a finite PSNR), n, and
    the per-image rows.  The per-image columns are the COLUMNS table; a further metric is one more column and one more
    summary entry.  ``feed`` only enqueues: the values are read back in ``result()``.

    ms_ssim=True: also an ``ms_ssim`` column (``ms_ssim`` over ``ms_weights``) and MS_SSIM_avg, MS_SSIM_std, ms_weights in the
    summary.  hand=True: ``feed`` takes a mask per batch; the HAND_COLUMNS and ``hand_fraction`` (mask_count / (H W)) join the
    rows, and SSIM_hand_avg, SSIM_hand_std, L1_hand_avg, PSNR_hand_avg (finite values), hand_fraction_avg - all over the n_hand
    images whose mask is not empty - the summary.  Without the flags rows and summary are what they always were."""

    COLUMNS = ("ssim", "l1", "mse", "psnr")
    HAND_COLUMNS = ("ssim_hand", "l1_hand", "mse_hand", "psnr_hand", "mask_count")

    def __init__(self, range="pm1", window=11, ms_ssim=False, hand=False, ms_weights=MS_WEIGHTS):
        if range not in RANGES:
            raise ValueError(f"range {range!r}: one of {sorted(RANGES)}")
        _check_window(window)
        self.range, self.window = range, window
        self.ms_ssim, self.hand, self.ms_weights = bool(ms_ssim), bool(hand), tuple(float(w) for w in ms_weights)
        self.columns = self.COLUMNS + (self.HAND_COLUMNS if self.hand else ()) + (("ms_ssim",) if self.ms_ssim else ())
        self._batches = []

    def feed(self, pred, target, paths=None, mask=None):
        """pred, target: one batch in this meter's range.  paths: None or one dict per image (e.g. {"target": ...,
        "source": ...}), copied into that image's row.  mask: the batch's region masks [B,H,W], given exactly when the meter
        was built with hand=True."""
        if self.hand != (mask is not None):
            raise ValueError("feed: a mask goes with hand=True, and only with it")
        m = image_metrics(pred, target, range=self.range, window=self.window, mask=mask)
        if self.ms_ssim:
            m["ms_ssim"] = ms_ssim(pred, target, range=self.range, window=self.window, weights=self.ms_weights)["ms_ssim"]
        n = m["ssim"].shape[0]
        if paths is not None and len(paths) != n:
            raise ValueError(f"feed: {len(paths)} paths for {n} images")
        pixels = int(mask.shape[1]) * int(mask.shape[2]) if mask is not None else None
        self._batches.append((torch.stack([m[k] for k in self.columns], 1), paths, pixels))

    def rows(self):
        out = []
        for vals, paths, pixels in self._batches:
            v = vals.cpu().numpy()
            for i in range(v.shape[0]):
                row = dict(paths[i]) if paths is not None else {}
                row.update({k: float(v[i, j]) for j, k in enumerate(self.columns)})
                if self.hand:
                    row["hand_fraction"] = row["mask_count"] / pixels
                out.append(row)
        return out

    @staticmethod
    def summarize(rows, ms_ssim=False, hand=False):
        s = np.array([r["ssim"] for r in rows], dtype=np.float64)
        l1 = np.array([r["l1"] for r in rows], dtype=np.float64)
        psnr = np.array([r["psnr"] for r in rows], dtype=np.float64)
        finite = psnr[np.isfinite(psnr)]
        out = {"SSIM_avg": float(np.mean(s)) if len(s) else None, "SSIM_std": float(np.std(s)) if len(s) else None,
               "L1_avg": float(np.mean(l1)) if len(l1) else None,
               "PSNR_avg": float(np.mean(finite)) if len(finite) else None, "n": len(rows)}
        if ms_ssim:
            ms = np.array([r["ms_ssim"] for r in rows], dtype=np.float64)
            out["MS_SSIM_avg"] = float(np.mean(ms)) if len(ms) else None
            out["MS_SSIM_std"] = float(np.std(ms)) if len(ms) else None
        if hand:
            inside = [r for r in rows if r["mask_count"] > 0]

            def mean(key, finite_only=False):
                v = np.array([r[key] for r in inside], dtype=np.float64)
                v = v[np.isfinite(v)] if finite_only else v
                return float(np.mean(v)) if len(v) else None

            sh = np.array([r["ssim_hand"] for r in inside], dtype=np.float64)
            out.update({"SSIM_hand_avg": mean("ssim_hand"), "SSIM_hand_std": float(np.std(sh)) if len(sh) else None,
                        "L1_hand_avg": mean("l1_hand"), "PSNR_hand_avg": mean("psnr_hand", finite_only=True),
                        "hand_fraction_avg": mean("hand_fraction"), "n_hand": len(inside)})
        return out

    def result(self):
        rows = self.rows()
        summary = self.summarize(rows, ms_ssim=self.ms_ssim, hand=self.hand)
        if self.ms_ssim:
            summary["ms_weights"] = list(self.ms_weights)
        return {"summary": summary, "rows": rows}
