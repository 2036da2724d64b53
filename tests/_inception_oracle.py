"""Oracles of the Inception-score feature, written from the public Inception-v3 graph and the reference's behaviour in this
project's own words:

* `forward`: Inception-v3 (eval, no aux head, transform_input=False) as plain torch.nn.functional calls on a state dict with
  UNFOLDED BatchNorm, in any dtype (float64 = the truth, float32 = PyTorch's own distance from it);
* `state_dict`: generated weights from `_hpe_oracle.hashed` - He-scaled convs, BatchNorm weights near 1, running_var in
  [0.5, 1.5], and an fc scale that makes the float64 score of `images` clearly different from 1;
* `pil_resize`, `preprocess`: a numpy model of PIL's two-pass fixed-point bilinear resize and of the Evaluator's transform chain;
* `max_pool`, `avg_pool`, `global_avgpool`, `score`: float64 numpy of the passes of csrc/inception.hip (the score with
  scipy.stats.entropy, as the reference)."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from tests._hpe_oracle import hashed

EPS = 0.001
# a deep random ReLU network sends every image close to one ray of feature space, so images differ mostly by a factor; the
# scale is large enough that this factor moves some images of `images` to another arg-max class (float64 score about 1.57 of 6)
FC_SCALE = 160.0
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ------------------------------------------------------------------------------------------------- the graph
def _unit(name, cin, cout, k, stride=1, pad=0):
    k = (k, k) if isinstance(k, int) else k
    pad = (pad, pad) if isinstance(pad, int) else pad
    return (name, cin, cout, k, stride, pad)


def _block_a(p, cin, pool):
    return [_unit(p + ".branch1x1", cin, 64, 1), _unit(p + ".branch5x5_1", cin, 48, 1), _unit(p + ".branch5x5_2", 48, 64, 5, pad=2),
            _unit(p + ".branch3x3dbl_1", cin, 64, 1), _unit(p + ".branch3x3dbl_2", 64, 96, 3, pad=1),
            _unit(p + ".branch3x3dbl_3", 96, 96, 3, pad=1), _unit(p + ".branch_pool", cin, pool, 1)]


def _block_b(p, cin):
    return [_unit(p + ".branch3x3", cin, 384, 3, 2), _unit(p + ".branch3x3dbl_1", cin, 64, 1),
            _unit(p + ".branch3x3dbl_2", 64, 96, 3, pad=1), _unit(p + ".branch3x3dbl_3", 96, 96, 3, 2)]


def _block_c(p, cin, c7):
    row, col = dict(k=(1, 7), pad=(0, 3)), dict(k=(7, 1), pad=(3, 0))
    return [_unit(p + ".branch1x1", cin, 192, 1), _unit(p + ".branch7x7_1", cin, c7, 1), _unit(p + ".branch7x7_2", c7, c7, **row),
            _unit(p + ".branch7x7_3", c7, 192, **col), _unit(p + ".branch7x7dbl_1", cin, c7, 1),
            _unit(p + ".branch7x7dbl_2", c7, c7, **col), _unit(p + ".branch7x7dbl_3", c7, c7, **row),
            _unit(p + ".branch7x7dbl_4", c7, c7, **col), _unit(p + ".branch7x7dbl_5", c7, 192, **row),
            _unit(p + ".branch_pool", cin, 192, 1)]


def _block_d(p, cin):
    return [_unit(p + ".branch3x3_1", cin, 192, 1), _unit(p + ".branch3x3_2", 192, 320, 3, 2), _unit(p + ".branch7x7x3_1", cin, 192, 1),
            _unit(p + ".branch7x7x3_2", 192, 192, (1, 7), pad=(0, 3)), _unit(p + ".branch7x7x3_3", 192, 192, (7, 1), pad=(3, 0)),
            _unit(p + ".branch7x7x3_4", 192, 192, 3, 2)]


def _block_e(p, cin):
    row, col = dict(k=(1, 3), pad=(0, 1)), dict(k=(3, 1), pad=(1, 0))
    return [_unit(p + ".branch1x1", cin, 320, 1), _unit(p + ".branch3x3_1", cin, 384, 1), _unit(p + ".branch3x3_2a", 384, 384, **row),
            _unit(p + ".branch3x3_2b", 384, 384, **col), _unit(p + ".branch3x3dbl_1", cin, 448, 1),
            _unit(p + ".branch3x3dbl_2", 448, 384, 3, pad=1), _unit(p + ".branch3x3dbl_3a", 384, 384, **row),
            _unit(p + ".branch3x3dbl_3b", 384, 384, **col), _unit(p + ".branch_pool", cin, 192, 1)]


def units(aux=False):
    """every conv + BatchNorm unit, in the order torchvision's module registers them"""
    u = [_unit("Conv2d_1a_3x3", 3, 32, 3, 2), _unit("Conv2d_2a_3x3", 32, 32, 3), _unit("Conv2d_2b_3x3", 32, 64, 3, pad=1),
         _unit("Conv2d_3b_1x1", 64, 80, 1), _unit("Conv2d_4a_3x3", 80, 192, 3)]
    u += _block_a("Mixed_5b", 192, 32) + _block_a("Mixed_5c", 256, 64) + _block_a("Mixed_5d", 288, 64) + _block_b("Mixed_6a", 288)
    u += _block_c("Mixed_6b", 768, 128) + _block_c("Mixed_6c", 768, 160) + _block_c("Mixed_6d", 768, 160) + _block_c("Mixed_6e", 768, 192)
    if aux:
        u += [_unit("AuxLogits.conv0", 768, 128, 1), _unit("AuxLogits.conv1", 128, 768, 5)]
    u += _block_d("Mixed_7a", 768) + _block_e("Mixed_7b", 1280) + _block_e("Mixed_7c", 2048)
    return u


UNITS = {u[0]: u for u in units()}


def state_dict(seed=0, aux=False, dtype=torch.float64):
    """torchvision's inception_v3 keys in its order (aux: with AuxLogits.*, which no forward here reads).  conv weights uniform in
    +-sqrt(6 / fan_in); bn.weight 1 +- 0.1, bn.bias +- 0.05, running_mean +- 0.1, running_var 1 +- 0.5; fc.weight uniform in
    +-FC_SCALE sqrt(3 / 2048), fc.bias +- 0.05."""
    sd, t = OrderedDict(), 20000

    def put(key, shape, scale, offset=0.0):
        nonlocal t
        if aux or not key.startswith("AuxLogits"):      # a tensor's counter does not depend on `aux`
            sd[key] = torch.from_numpy(hashed(t, int(np.prod(shape)), seed).reshape(shape) * scale + offset).to(dtype)
        t += 1

    def fc(prefix, n_in):
        put(prefix + ".weight", (1000, n_in), FC_SCALE * np.sqrt(3.0 / n_in))
        put(prefix + ".bias", (1000,), 0.05)

    for name, cin, cout, k, _, _ in units(True):
        put(name + ".conv.weight", (cout, cin) + k, np.sqrt(6.0 / (cin * k[0] * k[1])))
        put(name + ".bn.weight", (cout,), 0.1, 1.0)
        put(name + ".bn.bias", (cout,), 0.05)
        put(name + ".bn.running_mean", (cout,), 0.1)
        put(name + ".bn.running_var", (cout,), 0.5, 1.0)
        if aux or not name.startswith("AuxLogits"):
            sd[name + ".bn.num_batches_tracked"] = torch.tensor(0, dtype=torch.long)
        if name == "AuxLogits.conv1":
            fc("AuxLogits.fc", 768)
    fc("fc", 2048)
    return sd


def keys_and_shapes(sd):
    return [[k, list(v.shape)] for k, v in sd.items()]


def images(B, H, W_, seed=0):
    """fp32 [B,3,H,W] in [-1, 1]: noise of a per-image amplitude around a per-image colour (a generator's output range)"""
    noise = hashed(9100, B * 3 * H * W_, seed).reshape(B, 3, H, W_)
    colour = hashed(9101, B * 3, seed).reshape(B, 3, 1, 1) * 0.7
    amp = 0.15 + 0.15 * (hashed(9102, B, seed).reshape(B, 1, 1, 1) + 1.0)
    return np.clip(colour + amp * noise, -1.0, 1.0).astype(np.float32)


def net_inputs(shape, seed=0, index=0):
    """float64 [B,3,H,W] in the normalised images' range (about +-2): the golden network inputs"""
    return hashed(9200 + index, int(np.prod(shape)), seed).reshape(shape) * 2.0


def forward(sd, x, dtype=torch.float64, features=False):
    """x [B,3,H,W] (H, W >= 75) -> logits [B,1000] (features: the pooled [B,2048]) in `dtype`, BatchNorm applied as such"""
    sd = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    x = torch.as_tensor(x).to(dtype)

    def unit(name, x):
        _, _, _, _, stride, pad = UNITS[name]
        y = F.conv2d(x, sd[name + ".conv.weight"], None, stride, pad)
        y = F.batch_norm(y, sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"], sd[name + ".bn.weight"],
                         sd[name + ".bn.bias"], False, 0.0, EPS)
        return F.relu(y)

    def chain(p, names, x):
        for n in names:
            x = unit(p + "." + n, x)
        return x

    def avg(x):
        return F.avg_pool2d(x, 3, 1, 1)

    def a(p, x):
        return torch.cat([unit(p + ".branch1x1", x), chain(p, ["branch5x5_1", "branch5x5_2"], x),
                          chain(p, ["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], x), unit(p + ".branch_pool", avg(x))], 1)

    def b(p, x):
        return torch.cat([unit(p + ".branch3x3", x), chain(p, ["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], x),
                          F.max_pool2d(x, 3, 2)], 1)

    def c(p, x):
        return torch.cat([unit(p + ".branch1x1", x), chain(p, ["branch7x7_1", "branch7x7_2", "branch7x7_3"], x),
                          chain(p, ["branch7x7dbl_%d" % i for i in range(1, 6)], x), unit(p + ".branch_pool", avg(x))], 1)

    def d(p, x):
        return torch.cat([chain(p, ["branch3x3_1", "branch3x3_2"], x), chain(p, ["branch7x7x3_%d" % i for i in range(1, 5)], x),
                          F.max_pool2d(x, 3, 2)], 1)

    def e(p, x):
        t = unit(p + ".branch3x3_1", x)
        u = chain(p, ["branch3x3dbl_1", "branch3x3dbl_2"], x)
        return torch.cat([unit(p + ".branch1x1", x), unit(p + ".branch3x3_2a", t), unit(p + ".branch3x3_2b", t),
                          unit(p + ".branch3x3dbl_3a", u), unit(p + ".branch3x3dbl_3b", u), unit(p + ".branch_pool", avg(x))], 1)

    with torch.no_grad():
        for n in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
            x = unit(n, x)
        x = F.max_pool2d(x, 3, 2)
        x = unit("Conv2d_4a_3x3", unit("Conv2d_3b_1x1", x))
        x = F.max_pool2d(x, 3, 2)
        x = a("Mixed_5d", a("Mixed_5c", a("Mixed_5b", x)))
        x = b("Mixed_6a", x)
        for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = c(n, x)
        x = e("Mixed_7c", e("Mixed_7b", d("Mixed_7a", x)))
        x = x.mean((2, 3))
        return x if features else F.linear(x, sd["fc.weight"], sd["fc.bias"])


# ------------------------------------------------------------------------------------------------- preprocess
def to_bytes(x):
    """fp32 values in [-1, 1] -> the bytes aug writes: ((v * 0.5 + 0.5) * 255).round().clamp(0, 255), in fp32 (aug.py:142)"""
    x = np.asarray(x, dtype=np.float32)
    t = (x * np.float32(0.5) + np.float32(0.5)) * np.float32(255.0)
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def _axis_coefficients(n_in, n_out):
    """per output pixel (first input pixel, [22-bit integer weights]) of PIL's bilinear (triangle) filter along one axis"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    out = []
    for j in range(n_out):
        centre = (j + 0.5) * scale
        lo = max(int(centre - fs + 0.5), 0)
        hi = min(int(centre + fs + 0.5), n_in)
        w = []
        for i in range(lo, hi):
            a = abs((i - centre + 0.5) / fs)
            w.append(1.0 - a if a < 1.0 else 0.0)
        total = 0.0
        for v in w:
            total += v
        w = [v / total for v in w] if total != 0.0 else w
        out.append((lo, [int(0.5 + v * (1 << 22)) if v >= 0 else int(-0.5 + v * (1 << 22)) for v in w]))
    return out


def _resample_axis(img, n_out, axis):
    img = np.moveaxis(img.astype(np.int64), axis, 0)
    rows = []
    for lo, w in _axis_coefficients(img.shape[0], n_out):
        acc = np.full(img.shape[1:], 1 << 21, dtype=np.int64)
        for i, k in enumerate(w):
            acc = acc + img[lo + i] * k
        rows.append(np.clip(acc >> 22, 0, 255))
    return np.moveaxis(np.stack(rows), 0, axis).astype(np.uint8)


def pil_resize(img, oh, ow):
    """uint8 [H,W,3] -> uint8 [oh,ow,3] as PIL.Image.resize((ow, oh), BILINEAR): the horizontal pass to uint8, then the vertical"""
    return _resample_axis(_resample_axis(img, ow, 1), oh, 0)


def resized(H, W_, size):
    return (int(size * H / W_), size) if W_ <= H else (size, int(size * W_ / H))


def lut():
    """fp32 [3,256]: the torch chain ToTensor -> Normalize on every byte"""
    u = torch.arange(256).to(torch.uint8)
    t = u.to(torch.float32).div(255)[None].repeat(3, 1)
    return t.sub(torch.tensor(MEAN)[:, None]).div(torch.tensor(STD)[:, None]).numpy()


def preprocess(u8, size=299):
    """uint8 [B,H,W,3] RGB -> fp32 [B,size,size,4]: Resize(size), CenterCrop(size), ToTensor, Normalize; lane 3 zero"""
    B, H, W_, _ = u8.shape
    rh, rw = resized(H, W_, size)
    top, left = int(round((rh - size) / 2.0)), int(round((rw - size) / 2.0))
    table = lut()
    out = np.zeros((B, size, size, 4), dtype=np.float32)
    for b in range(B):
        r = pil_resize(u8[b], rh, rw)[top:top + size, left:left + size]
        for c in range(3):
            out[b, :, :, c] = table[c][r[:, :, c]]
    return out


# ------------------------------------------------------------------------------------------------- pools and score
def max_pool(x):
    """float64 NHWC: 3 x 3, stride 2, no padding, floor"""
    B, H, W_, C = x.shape
    Ho, Wo = (H - 3) // 2 + 1, (W_ - 3) // 2 + 1
    out = np.full((B, Ho, Wo, C), -np.inf)
    for dh in range(3):
        for dw in range(3):
            out = np.maximum(out, x[:, dh:dh + 2 * Ho - 1:2, dw:dw + 2 * Wo - 1:2])
    return out


def avg_pool(x):
    """float64 NHWC: 3 x 3, stride 1, zero padding 1, always / 9"""
    B, H, W_, C = x.shape
    p = np.zeros((B, H + 2, W_ + 2, C))
    p[:, 1:-1, 1:-1] = x
    return sum(p[:, dh:dh + H, dw:dw + W_] for dh in range(3) for dw in range(3)) / 9.0


def global_avgpool(x):
    return x.reshape(x.shape[0], -1, x.shape[3]).mean(1)


def score(logits):
    """float64: (kl [n], py [classes], exp(mean(kl))) of one group - softmax, mean row, scipy.stats.entropy per row"""
    from scipy.stats import entropy
    z = np.asarray(logits, dtype=np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    pyx = e / e.sum(1, keepdims=True)
    py = np.mean(pyx, axis=0)
    kl = np.array([entropy(pyx[i], py) for i in range(pyx.shape[0])])
    return kl, py, float(np.exp(np.mean(kl)))


def grouped(logits, group):
    """the Evaluator's figures: scores of consecutive groups (a tail on its own) -> (IS_avg, IS_std, IS_all, n_groups, kl)"""
    n = len(logits)
    parts = [score(logits[i:i + group]) for i in range(0, n, group)]
    s = [p[2] for p in parts]
    return float(np.mean(s)), float(np.std(s)), score(logits)[2], len(s), np.concatenate([p[0] for p in parts])
