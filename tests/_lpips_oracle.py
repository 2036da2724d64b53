"""float64 references for LPIPS (mmhand_amd/lpips.py, csrc/lpips.hip), written from the definition of the `lpips` package's
LPIPS(net="vgg", spatial=False): the scaling layer, the VGG-16 trunk (torch.nn.functional.conv2d on the CPU, float64 unless told
otherwise) and the per-layer distance, plus generated weights.  Generated weights: every figure says nothing about images."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256),
         (17, 256, 512), (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))
TAPS = (2, 7, 14, 21, 28)
POOL_AFTER = (2, 7, 14, 21)
WIDTHS = (64, 128, 256, 512, 512)
EPS = 1e-10
SHIFT = np.array([-.030, -.088, -.188], dtype=np.float32).astype(np.float64)
SCALE = np.array([.458, .448, .450], dtype=np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------- generated weights
def vgg16_state_dict(seed=0, prefix="features."):
    """He-normal 3x3 convolutions (std = sqrt(2 / fan_in): the ReLUs keep about half their inputs alive at every depth) and
    small biases, torchvision's key layout, fp32"""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for n, cin, cout in CONVS:
        sd[f"{prefix}{n}.weight"] = (torch.randn((cout, cin, 3, 3), generator=g, dtype=torch.float64) *
                                     np.sqrt(2.0 / (cin * 9))).to(torch.float32)
        sd[f"{prefix}{n}.bias"] = ((torch.rand((cout,), generator=g, dtype=torch.float64) - 0.5) * 0.1).to(torch.float32)
    return sd


def lin_state_dict(seed=1):
    """linear heads uniform in [-0.25, 1]: mostly positive, as trained ones are, with negative entries present"""
    g = torch.Generator().manual_seed(seed)
    return OrderedDict((f"lin{l}.model.1.weight",
                        (torch.rand((1, c, 1, 1), generator=g, dtype=torch.float64) * 1.25 - 0.25).to(torch.float32))
                       for l, c in enumerate(WIDTHS))


def lin_vectors(lin):
    """the five [C] float64 numpy weight vectors of a lin state dict, or all ones for "uniform" """
    if isinstance(lin, str) and lin == "uniform":
        return [np.ones(c) for c in WIDTHS]
    return [lin[f"lin{l}.model.1.weight"].double().numpy().reshape(-1) for l in range(5)]


# ------------------------------------------------------------------------------------------------- the three passes
def rgb_pm1(images, layout):
    """a host array in one of the accepted forms -> float64 [B,H,W,3] RGB in [-1, 1]: floats as they are, bytes u / 255 * 2 - 1"""
    x = np.asarray(images)
    if layout == "nchw":
        x = np.transpose(x, (0, 2, 3, 1))
    elif layout == "bgr_hwc":
        x = x[..., ::-1]
    else:
        raise ValueError(layout)
    if x.dtype == np.uint8:
        return x.astype(np.float64) / 255.0 * 2.0 - 1.0
    return x.astype(np.float64)


def preprocess(images, layout):
    """-> fp32 [B,H,W,4]: (v - shift) / scale in float64 rounded once, lane 3 zero"""
    v = rgb_pm1(images, layout)
    out = np.zeros(v.shape[:3] + (4,), dtype=np.float32)
    out[..., :3] = ((v - SHIFT) / SCALE).astype(np.float32)
    return out


def trunk(x, sd, dtype=torch.float64):
    """x: [B,H,W,>=3] (the preprocessed input; lanes 0..2 are read) -> the five taps as float64 numpy [B,h,w,C], the
    convolutions, ReLUs and pools in `dtype` on the CPU"""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x)[..., :3])).permute(0, 3, 1, 2).to(dtype)
    taps = []
    for n, _, _ in CONVS:
        t = F.relu(F.conv2d(t, sd[f"features.{n}.weight"].to(dtype), sd[f"features.{n}.bias"].to(dtype), padding=1))
        if n in TAPS:
            taps.append(t.permute(0, 2, 3, 1).double().numpy())
        if n in POOL_AFTER:
            t = F.max_pool2d(t, 2, 2)
    return taps


def layer(a, b, w):
    """a, b [B,H,W,C], w [C] -> (signed float64 [B], the same with |w|: the scale of the error bound)"""
    a, b, w = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(w, dtype=np.float64)
    na = np.sqrt(np.sum(a * a, axis=3, keepdims=True))
    nb = np.sqrt(np.sum(b * b, axis=3, keepdims=True))
    d2 = (a / (na + EPS) - b / (nb + EPS)) ** 2
    hw = a.shape[1] * a.shape[2]
    return np.sum(d2 * w, axis=(1, 2, 3)) / hw, np.sum(d2 * np.abs(w), axis=(1, 2, 3)) / hw


def layer_conv_form(a, b, w):
    """the same value the way the package writes it: normalize_tensor as x / (norm + eps) on NCHW tensors, the head as a 1x1
    convolution without bias, spatial_average as a mean over H and W - an independent formulation"""
    ta, tb = (torch.from_numpy(np.asarray(t, dtype=np.float64)).permute(0, 3, 1, 2) for t in (a, b))

    def normalize(t):
        norm = torch.sqrt(torch.sum(t ** 2, dim=1, keepdim=True))
        return t / (norm + EPS)

    diff = (normalize(ta) - normalize(tb)) ** 2
    head = torch.from_numpy(np.asarray(w, dtype=np.float64)).reshape(1, -1, 1, 1)
    return F.conv2d(diff, head).mean([2, 3]).reshape(-1).numpy()


def lpips(pred, pred_layout, target, target_layout, sd, lin, dtype=torch.float64):
    """-> (float64 [B,5] layer scores, the same with |w|) of the whole definition; `dtype`: the trunk's arithmetic"""
    ws = lin_vectors(lin)
    ta, tb = trunk(preprocess(pred, pred_layout), sd, dtype), trunk(preprocess(target, target_layout), sd, dtype)
    pairs = [layer(x, y, w) for x, y, w in zip(ta, tb, ws)]
    return np.stack([p[0] for p in pairs], 1), np.stack([p[1] for p in pairs], 1)
