"""LPIPS, the learned perceptual distance of Zhang et al. (CVPR 2018), on the device: the `lpips` package's
LPIPS(net="vgg", lpips=True, spatial=False) in eval mode, one value per image pair.  The reference Evaluator has no such metric;
pose-transfer papers report it beside SSIM and FID.

Definition (lpips/lpips.py, lpips/pretrained_networks.py: vgg16):

1. both images, RGB in [-1, 1] (bytes: u / 255 * 2 - 1), go through the ScalingLayer (ops.lpips_preprocess);
2. the trunk is torchvision's VGG-16 `features`: 3x3 zero-padded convolutions at indices 0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24,
   26, 28, a ReLU after each, a 2x2 max pool after 2, 7, 14 and 21.  The taps are the post-ReLU outputs of 2, 7, 14, 21 and 28
   (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3): 64, 128, 256, 512, 512 channels at H, H/2, H/4, H/8, H/16;
3. per tap and pixel both feature vectors are divided by (their length + 1e-10), the squared difference is weighted by the
   tap's linear head (weights of any sign) and summed over the channels; the tap's score is the mean over its pixels
   (ops.lpips_layer, float64);  LPIPS is the sum of the five scores.

The convolutions are mmh_conv2d_fprop (fp32 direct kernels, fused ReLU, summation pinned by hpe.direct_two_level), the pools
mmh_maxpool2x2_fwd: what hpe.py runs.  AlexNet-LPIPS is not offered: its first convolution has stride 4 and
mmh_conv2d_fprop[_rect] accept strides 1 and 2 only.  SqueezeNet-LPIPS is not offered either.

Weights.  No VGG-16 and no LPIPS file ships with this repository.  `Vgg16Lpips.load_state_dict` accepts

* torchvision's VGG-16 state dict: `features.N.weight` / `features.N.bias` for the thirteen N above; `classifier.*` and every
  other key are ignored; a leading `module.` is stripped;
* keys of the form `net.slice{K}.{N}.weight` / `.bias` with the same N and K = the slice that holds N (1: 0-3, 2: 4-8, 3: 9-15,
  4: 16-22, 5: 23-29), read as `features.N.*`.  This is believed to be the layout of `lpips.LPIPS(net="vgg").state_dict()`;
  it has not been checked against the package.

A file with a convolution at any other index (VGG-19 has them at 16, 23, 25, 30, 32, 34) is refused, and so is a missing key, by
name.  `load_lin` reads the package's linear heads, `lin{0..4}.model.1.weight` of shape [1, C, 1, 1] (the layout of the
package's weights/v0.1/vgg.pth; `lins.{l}.model.1.weight` of a full LPIPS state dict is accepted as well), or builds all-ones
heads for "uniform" - the package's lpips=False form: unweighted, and usable when only a VGG-16 file is at hand.  Every number
produced with generated weights says nothing about images."""
import contextlib
import re

import numpy as np
import torch

from . import hpe
from . import lib as L
from . import ops

# (features index, Cin, Cout) of the thirteen convolutions; a pool follows the ReLU of POOL_AFTER, a tap that of TAPS
CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256),
         (17, 256, 512), (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))
TAPS = (2, 7, 14, 21, 28)
POOL_AFTER = (2, 7, 14, 21)
WIDTHS = (64, 128, 256, 512, 512)
_SLICE_OF = {n: 1 + sum(n >= lo for lo in (4, 9, 16, 23)) for n, _, _ in CONVS}
CONV_LIMIT = 1 << 30            # mmh_conv2d_fprop: fewer elements than this per (padded) buffer


def _is_path(x):
    return isinstance(x, (str, bytes)) or hasattr(x, "__fspath__")


def map_keys(sd):
    """a state dict in one of the accepted layouts -> {"features.N.weight" / ".bias": tensor} for the keys that name a
    convolution of a VGG `features` stack; everything else is dropped"""
    out = {}
    for k, v in hpe.strip_module(sd).items():
        m = re.fullmatch(r"net\.slice(\d+)\.(\d+)\.(weight|bias)", k)
        if m:
            if _SLICE_OF.get(int(m.group(2))) != int(m.group(1)):
                raise ValueError(f"Vgg16Lpips: {k}: index {m.group(2)} is no VGG-16 convolution of slice {m.group(1)}")
            k = f"features.{m.group(2)}.{m.group(3)}"
        if re.fullmatch(r"features\.\d+\.(weight|bias)", k):
            out[k] = v
    return out


def load_lin(src):
    """"uniform" | a path | a dict -> five fp32 [C] tensors (host), C = 64, 128, 256, 512, 512"""
    if isinstance(src, str) and src == "uniform":
        return [torch.ones(c, dtype=torch.float32) for c in WIDTHS]
    sd = torch.load(src, map_location="cpu") if _is_path(src) else src
    sd = hpe.strip_module(sd)
    out = []
    for l, c in enumerate(WIDTHS):
        key = f"lin{l}.model.1.weight"
        w = sd.get(key, sd.get(f"lins.{l}.model.1.weight"))
        if w is None:
            raise KeyError(f"load_lin: the file lacks {key}")
        if tuple(w.shape) != (1, c, 1, 1):
            raise ValueError(f"load_lin: {key} is {tuple(w.shape)}, [1, {c}, 1, 1] expected (the VGG heads)")
        out.append(w.detach().to(torch.float32).reshape(c).contiguous())
    return out


class Vgg16Lpips:
    """the trunk of LPIPS(net="vgg") up to relu5_3.  forward_taps(x fp32 [B,H,W,4], ops.lpips_preprocess's output) -> the five
    tap tensors fp32 [B,H/2^l,W/2^l,C_l]"""

    def __init__(self, device=None):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.convs = None

    def load_state_dict(self, sd):
        sd = map_keys(sd)
        known = {n for n, _, _ in CONVS}
        extra = sorted({int(k.split(".")[1]) for k in sd} - known)
        if extra:
            raise ValueError(f"Vgg16Lpips: convolutions at features.{extra}: not a VGG-16 (a 19-layer file has them at 16, 23, "
                             "25, 30, 32, 34)")
        convs = {}
        for n, cin, cout in CONVS:
            for p in ("weight", "bias"):
                if f"features.{n}.{p}" not in sd:
                    raise KeyError(f"Vgg16Lpips: the state dict lacks features.{n}.{p}")
            w, b = sd[f"features.{n}.weight"], sd[f"features.{n}.bias"]
            if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
                raise ValueError(f"Vgg16Lpips: features.{n}.weight is {tuple(w.shape)}, {(cout, cin, 3, 3)} expected")
            convs[n] = tuple(t.to(self.device) for t in hpe.relay_conv(w, b))
        self.convs = convs
        return self

    def _stages(self, x):
        """yields the five taps in order; the caller holds hpe.direct_two_level() open around the iteration"""
        assert self.convs is not None, "load_state_dict first"
        ops._chk(x, "x")
        B, H, W_, cx = x.shape
        if cx != 4 or H % 16 or W_ % 16:
            raise ValueError(f"Vgg16Lpips: expected [B,H,W,4] with H and W multiples of 16, got {tuple(x.shape)}")
        for n, _, cout in CONVS:
            w, b = self.convs[n]
            y = ops._empty((B, H, W_, cout), x)
            hpe._conv(x, 0, x.shape[3], w, b, y, 0, cout, B, H, W_, L.ACT_RELU)
            x = y
            del y
            if n in TAPS:
                yield x
            if n in POOL_AFTER:
                y = ops._empty((B, H // 2, W_ // 2, cout), x)
                L.call("mmh_maxpool2x2_fwd", ops._ptr(x), B, H, W_, cout, ops._ptr(y), ops._stream())
                x, H, W_ = y, H // 2, W_ // 2
                del y

    @torch.no_grad()
    def forward_taps(self, x):
        with hpe.direct_two_level():
            return list(self._stages(x))


def _hw(images, layout):
    return (images.shape[2], images.shape[3]) if layout == "nchw" else (images.shape[1], images.shape[2])


class LpipsScorer:
    """LPIPS of image pairs, batch by batch.  feed() enqueues preprocess -> trunk -> the five layer distances for both sides
    and keeps the per-image, per-layer values (float64 [B,5]) on the device; rows() / results() read them back.
    backbone: a Vgg16Lpips, a VGG-16 state dict or a path to one; lin: "uniform", a path, a dict (see load_lin) or five [C]
    tensors."""

    def __init__(self, backbone, lin, device=None):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if not isinstance(backbone, Vgg16Lpips):
            sd = torch.load(backbone, map_location="cpu") if _is_path(backbone) else backbone
            backbone = Vgg16Lpips(self.device).load_state_dict(sd)
        self.net = backbone
        self.lin_name = lin if isinstance(lin, str) else ("file" if _is_path(lin) else "custom")
        heads = load_lin(lin) if (_is_path(lin) or isinstance(lin, dict)) else list(lin)
        if [tuple(w.shape) for w in heads] != [(c,) for c in WIDTHS]:
            raise ValueError(f"LpipsScorer: linear heads of widths {[tuple(w.shape) for w in heads]}, {WIDTHS} expected")
        self.lin = [w.detach().to(self.device, torch.float32).contiguous() for w in heads]
        self._batches = []

    @staticmethod
    def chunk_size(H, W_):
        """images per trunk pass: the widest buffer per image is the first tap's 64 lanes over the padded image"""
        return max(1, (CONV_LIMIT - 1) // ((H + 2) * (W_ + 2) * 64))

    @torch.no_grad()
    def distances(self, pred, pred_layout, target, target_layout):
        """-> float64 [B,5] on the device: every pair's five layer scores"""
        H, W_ = _hw(pred, pred_layout)
        if (H, W_) != _hw(target, target_layout) or pred.shape[0] != target.shape[0]:
            raise ValueError(f"LpipsScorer: pred {tuple(pred.shape)} ({pred_layout}) and target {tuple(target.shape)} "
                             f"({target_layout}) are not the same number of images of one size")
        if H % 16 or W_ % 16:
            raise ValueError(f"LpipsScorer: {H} x {W_} images: the VGG-16 trunk pools four times, H and W must be multiples of 16")
        B, n = pred.shape[0], self.chunk_size(H, W_)
        out = torch.empty((B, 5), dtype=torch.float64, device=self.device)
        with hpe.direct_two_level():
            for i in range(0, B, n):
                xa = ops.lpips_preprocess(pred[i:i + n], pred_layout)
                xb = ops.lpips_preprocess(target[i:i + n], target_layout)
                col = torch.empty((5, xa.shape[0]), dtype=torch.float64, device=self.device)
                sa, sb = self.net._stages(xa), self.net._stages(xb)
                del xa, xb
                for l in range(5):      # a tap's buffers are dropped as soon as its score is enqueued and the pool has read them
                    ta, tb = next(sa), next(sb)
                    ops.lpips_layer(ta, tb, self.lin[l], out=col[l])
                    del ta, tb
                for s in (sa, sb):
                    with contextlib.suppress(StopIteration):
                        next(s)
                out[i:i + n] = col.t()
        return out

    def feed(self, pred, pred_layout, target, target_layout, paths=None):
        """pred / target: one batch each (see ops.lpips_preprocess); paths: None or one dict per image, copied into its row"""
        B = pred.shape[0]
        if paths is not None and len(paths) != B:
            raise ValueError(f"feed: {B} images, {len(paths)} paths")
        self._batches.append((self.distances(pred, pred_layout, target, target_layout), paths))

    def layers(self):
        """float64 [n,5] on the host"""
        return np.concatenate([v.cpu().numpy() for v, _ in self._batches]) if self._batches else np.zeros((0, 5))

    @staticmethod
    def total(v):
        """the five layer scores of each row added in tap order"""
        return (((v[:, 0] + v[:, 1]) + v[:, 2]) + v[:, 3]) + v[:, 4]

    def rows(self):
        tot = self.total(self.layers())
        paths = [dict(ps[i]) if ps is not None else {} for v, ps in self._batches for i in range(v.shape[0])]
        return [dict(p, lpips=float(t)) for p, t in zip(paths, tot)]

    def results(self):
        v = self.layers()
        if not len(v):
            return {"LPIPS_avg": None, "LPIPS_layers": [None] * 5, "lpips_lin": self.lin_name, "n": 0}
        return {"LPIPS_avg": float(np.mean(self.total(v))), "LPIPS_layers": [float(x) for x in v.mean(0)],
                "lpips_lin": self.lin_name, "n": int(v.shape[0])}
