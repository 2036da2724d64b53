"""Oracles of the PCK feature, written from the reference's behaviour in this project's own words:

* `forward_2d` / `forward_3d`: the two hand-pose machines (networks/net_hpm2d.py, net_hpm3d.py) as plain torch.nn.functional
  calls on a state dict, in any dtype (float64 = the truth, float32 = PyTorch's own distance from it);
* `normalize`, `upsample_argmax`, `measures`: float64 numpy of the passes of csrc/hpe.hip and of EvalUtil.get_measures;
* `hashed` / `state_dicts`: generated weights from a counter-based integer hash of (tensor index, element index), scaled per
  layer as He initialisation scales - no library RNG stream, so the same bits on any machine."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

JOINTS = 21
FULL = dict(c1=64, c2=128, c3=256, c4=512, c0=128, cpm=512, rep=128, fc=512)
NARROW = dict(c1=8, c2=8, c3=12, c4=16, c0=8, cpm=16, rep=8, fc=16)
TRUNK = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv3_4", "conv4_1", "conv4_2",
         "conv4_3", "conv4_4", "conv5_1", "conv5_2", "conv5_3_CPM")
POOL_AFTER = ("conv1_2", "conv2_2", "conv3_4")
REPEAT = ("conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7")


# ------------------------------------------------------------------------------------------------- generated weights
def _mix(x):
    """the 64-bit finaliser of splitmix64 on a uint64 array (wrapping arithmetic)"""
    x = x.copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


def hashed(tensor_index, n, seed=0):
    """n float64 values in [-1, 1): element i of tensor t is a function of (seed, t, i) alone"""
    with np.errstate(over="ignore"):
        key = _mix(np.full(1, (int(seed) << 32) + int(tensor_index) + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
        bits = _mix(np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + key)
    return (bits >> np.uint64(11)).astype(np.float64) / float(1 << 52) - 1.0


def images(B, H, W_, seed=0):
    """fp32 [B,3,H,W] in [-1, 1): the test images (a generator's output range)"""
    return hashed(9000, B * 3 * H * W_, seed).reshape(B, 3, H, W_).astype(np.float32)


def _layers(widths, in_nc, with_depth, head_hw):
    w = widths
    chans = [in_nc, w["c1"], w["c1"], w["c2"], w["c2"], w["c3"], w["c3"], w["c3"], w["c3"], w["c4"], w["c4"], w["c4"], w["c4"],
             w["c4"], w["c4"], w["c0"]]
    layers = [(n, (chans[i + 1], chans[i], 3, 3)) for i, n in enumerate(TRUNK)]
    layers += [("conv6_1_CPM", (w["cpm"], w["c0"], 1, 1)), ("conv6_2_CPM", (JOINTS, w["cpm"], 1, 1))]
    for s in ("stage2", "stage3", "stage4", "stage5", "stage6") + (("depth",) if with_depth else ()):
        layers.append((f"{s}.conv1", (w["rep"], w["c0"] + JOINTS, 7, 7)))
        layers += [(f"{s}.conv{i}", (w["rep"], w["rep"], 7, 7)) for i in (2, 3, 4, 5)]
        layers += [(f"{s}.conv6", (w["rep"], w["rep"], 1, 1)), (f"{s}.conv7", (JOINTS, w["rep"], 1, 1))]
    if with_depth:
        layers += [("depth_fc_1", (w["fc"], JOINTS * head_hw * head_hw)), ("depth_fc_2", (w["fc"], w["fc"])),
                   ("depth_fc_3", (JOINTS, w["fc"]))]
    return layers


def state_dict(kind, widths=FULL, head_hw=32, seed=0, dtype=torch.float64):
    """kind "2d" (input_nc 3) | "3d" (input_nc 21, with depth.* and depth_fc_*): the reference's keys in its order.  Weights
    uniform in +-sqrt(6 / fan_in) (variance 2 / fan_in), biases uniform in +-0.05; the Linear layers, which have no ReLU
    between them, +-sqrt(3 / fan_in)."""
    sd, t = OrderedDict(), (0 if kind == "2d" else 1000)
    for name, shape in _layers(widths, 3 if kind == "2d" else JOINTS, kind == "3d", head_hw):
        fan_in = int(np.prod(shape[1:]))
        a = np.sqrt((3.0 if len(shape) == 2 else 6.0) / fan_in)
        sd[name + ".weight"] = torch.from_numpy(hashed(t, int(np.prod(shape)), seed).reshape(shape) * a).to(dtype)
        sd[name + ".bias"] = torch.from_numpy(hashed(t + 1, shape[0], seed) * 0.05).to(dtype)
        t += 2
    return sd


def keys_and_shapes(sd):
    return [[k, list(v.shape)] for k, v in sd.items()]


# ------------------------------------------------------------------------------------------------- the two networks
def _conv(sd, name, x, relu=True):
    w = sd[name + ".weight"]
    y = F.conv2d(x, w, sd[name + ".bias"], padding=w.shape[2] // 2)
    return F.relu(y) if relu else y


def _repeat(sd, s, x):
    for c in REPEAT[:-1]:
        x = _conv(sd, f"{s}.{c}", x)
    return _conv(sd, f"{s}.conv7", x, relu=False)


def _front(sd, x, stages):
    for n in TRUNK:
        x = _conv(sd, n, x)
        if n in POOL_AFTER:
            x = F.max_pool2d(x, 2)
    out0 = x
    heat = _conv(sd, "conv6_2_CPM", _conv(sd, "conv6_1_CPM", out0), relu=False)
    for s in stages:
        heat = _repeat(sd, s, torch.cat((heat, out0), 1))
    return heat, out0


def forward_2d(sd, x):
    """x [B,3,H,W] -> the last stage's heat maps [B,21,H/8,W/8] in x's dtype (before the x8 upsample)"""
    sd = {k: v.to(x.dtype) for k, v in sd.items()}
    with torch.no_grad():
        return _front(sd, x, ("stage2", "stage3", "stage4", "stage5", "stage6"))[0]


def forward_3d(sd, x):
    """x [B,21,H,W] (upsampled heat maps) -> depths [B,21] in x's dtype; stage6 is not run, as in the reference"""
    sd = {k: v.to(x.dtype) for k, v in sd.items()}
    with torch.no_grad():
        heat, out0 = _front(sd, x, ("stage2", "stage3", "stage4", "stage5"))
        d = _repeat(sd, "depth", torch.cat((heat, out0), 1)).reshape(x.shape[0], -1)
        for n in ("depth_fc_1", "depth_fc_2", "depth_fc_3"):
            d = F.linear(d, sd[n + ".weight"], sd[n + ".bias"])
        return d


def rel_l1(a, b):
    """sum |a - b| / sum |b| in float64"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).sum() / np.abs(b).sum())


# ------------------------------------------------------------------------------------------------- the passes of hpe.hip
def normalize(img):
    """img [B,3,H,W] of any real dtype -> fp32 [B,H,W,4]: per image (x - min) / (max - min) in float64 rounded once, lane 3
    zero; a constant image gives zeros"""
    x = np.asarray(img).astype(np.float64)
    out = np.zeros((x.shape[0], x.shape[2], x.shape[3], 4), dtype=np.float32)
    for b in range(x.shape[0]):
        mn, mx = x[b].min(), x[b].max()
        if mx > mn:
            out[b, :, :, :3] = ((x[b] - mn) / (mx - mn)).astype(np.float32).transpose(1, 2, 0)
    return out


def _taps(n_src, n_out):
    scale = np.float64(n_src - 1) / np.float64(n_out - 1)
    s = scale * np.arange(n_out, dtype=np.float64)
    i0 = np.minimum(s.astype(np.int64), n_src - 1)
    return i0, np.minimum(i0 + 1, n_src - 1), s - i0


def upsample(heat, factor=8):
    """heat [B,h,w,C] -> float64 [B,8h,8w,C]: bilinear, align_corners=True, each operation rounded on its own"""
    v = np.asarray(heat).astype(np.float64)
    _, h, w, _ = v.shape
    y0, y1, wy = _taps(h, h * factor)
    x0, x1, wx = _taps(w, w * factor)
    wy, wx = wy[None, :, None, None], wx[None, None, :, None]
    top = (1.0 - wx) * v[:, y0][:, :, x0] + wx * v[:, y0][:, :, x1]
    bot = (1.0 - wx) * v[:, y1][:, :, x0] + wx * v[:, y1][:, :, x1]
    return (1.0 - wy) * top + wy * bot


def upsample_argmax(heat, factor=8):
    """heat fp32 [B,h,w,cs >= 21] -> (up fp32 [B,8h,8w,24] with lanes 21..23 zero, xy int32 [B,21,2], peak fp32 [B,21]): the
    arg-max is over the rounded fp32 values, the first in scan order among equals (np.argmax's rule)"""
    up64 = upsample(np.asarray(heat)[..., :JOINTS], factor)
    B, Ho, Wo, _ = up64.shape
    up = np.zeros((B, Ho, Wo, 24), dtype=np.float32)
    up[..., :JOINTS] = up64.astype(np.float32)
    flat = up[..., :JOINTS].reshape(B, Ho * Wo, JOINTS)
    idx = flat.argmax(1)
    xy = np.stack([idx % Wo, idx // Wo], -1).astype(np.int32)
    return up, xy, flat.max(1)


def top_two_gap(up):
    """up [B,H,W,>=21] -> [B,21]: the largest value minus the largest value at another pixel"""
    B, H, W_, _ = up.shape
    flat = np.sort(np.asarray(up, dtype=np.float64)[..., :JOINTS].reshape(B, H * W_, JOINTS), 1)
    return flat[:, -1] - flat[:, -2]


def measures(dist, max_px=30, steps=20):
    """EvalUtil.get_measures(0, max_px, steps) of dist [n,J], every joint visible -> (epe_mean, epe_median, auc, curve,
    thresholds)"""
    d = np.asarray(dist, dtype=np.float64)
    thr = np.linspace(0, max_px, steps)
    area = lambda y: np.sum((thr[1:] - thr[:-1]) * (y[1:] + y[:-1]) / 2.0)        # noqa: E731
    curves = np.stack([(d[:, j, None] <= thr[None]).mean(0) for j in range(d.shape[1])])
    auc = np.mean([area(c) / area(np.ones_like(thr)) for c in curves])
    return float(d.mean(0).mean()), float(np.median(d, 0).mean()), float(auc), curves.mean(0), thr


def distances(uv, xy, depth=None, z=None, height=None, z_scale=256.0):
    """EvalUtil.feed's distances for [n,21,2] targets and predictions; with depth / z also the 3D ones"""
    diff = np.asarray(uv, dtype=np.float64) - np.asarray(xy, dtype=np.float64)
    d2 = np.sqrt((diff ** 2).sum(2))
    if depth is None:
        return d2, None
    dz = np.asarray(depth, dtype=np.float64) * z_scale - np.asarray(z, dtype=np.float64) * height
    return d2, np.sqrt((diff ** 2).sum(2) + dz ** 2)
