"""The reference Evaluator's Inception score on the device (baselines/quantitative_on_benchmarks/utils.py:12-112,196-232 and
inception.py): torchvision's Inception-v3, inference only, and the score of its logits.

`InceptionV3` loads torchvision's `inception_v3_google` state dict (what the reference's inception_v3(True, ...) loads; a leading
"module." is stripped, AuxLogits.* is accepted and ignored) and re-lays it once:

* every BasicConv2d's BatchNorm (eps 0.001) is folded into its conv in float64 on the host - w' = w * gamma / sqrt(var + eps),
  b' = beta - mean * gamma / sqrt(var + eps) - and rounded once to fp32;
* conv weights [Cout,Cin,kh,kw] -> RSCK [kh,kw,Cin',Cout] fp32 (hpe.relay_conv), the image's 3 channels padded to 4;
* fc.weight [1000,2048] stored transposed for mmh_linear_fprop.

The forward is transform_input=False, eval mode, no dropout, no aux head.  Every block has ONE output buffer: each branch's
last conv, and the max-pool branches of Mixed_6a and Mixed_7a, write their lanes of it through the conv's / pool's y_cs and an
offset pointer - there is no torch.cat.  All channel counts are multiples of 4, so every offset is 16-byte aligned.  Square
kernels go through mmh_conv2d_fprop, the 1x7 / 7x1 / 1x3 / 3x1 ones through mmh_conv2d_fprop_rect; ReLU is fused; conv_levels
is hpe.DIRECT_LEVELS for the duration of the call (hpe.direct_two_level).  Any input from 75 x 75 up works (the smallest that
leaves a 1 x 1 grid).

Two departures from the reference, both stated in DESIGN 4.5h: images become bytes by the [0, 1] mapping `aug` and SSIM use
(the reference's ToPILImage wraps the negative half of a [-1, 1] tensor), and the score is float64 from the logits on (the
reference rounds the softmax to fp32 first).

No Inception weights exist in this repository or the reference's: a score means what its weight file means."""

import numpy as np
import torch

from . import lib as L
from . import ops
from .hpe import direct_two_level, relay_conv, relay_fc, strip_module

BN_EPS = 0.001
SIZE = 299
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
PIL_BITS = 22


# ------------------------------------------------------------------------------------------------- the graph
def _a(name, cin, pool):
    return [(f"{name}.branch1x1", cin, 64, 1, 1, 1, 0, 0), (f"{name}.branch5x5_1", cin, 48, 1, 1, 1, 0, 0),
            (f"{name}.branch5x5_2", 48, 64, 5, 5, 1, 2, 2), (f"{name}.branch3x3dbl_1", cin, 64, 1, 1, 1, 0, 0),
            (f"{name}.branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1), (f"{name}.branch3x3dbl_3", 96, 96, 3, 3, 1, 1, 1),
            (f"{name}.branch_pool", cin, pool, 1, 1, 1, 0, 0)]


def _c(name, c7):
    return [(f"{name}.branch1x1", 768, 192, 1, 1, 1, 0, 0), (f"{name}.branch7x7_1", 768, c7, 1, 1, 1, 0, 0),
            (f"{name}.branch7x7_2", c7, c7, 1, 7, 1, 0, 3), (f"{name}.branch7x7_3", c7, 192, 7, 1, 1, 3, 0),
            (f"{name}.branch7x7dbl_1", 768, c7, 1, 1, 1, 0, 0), (f"{name}.branch7x7dbl_2", c7, c7, 7, 1, 1, 3, 0),
            (f"{name}.branch7x7dbl_3", c7, c7, 1, 7, 1, 0, 3), (f"{name}.branch7x7dbl_4", c7, c7, 7, 1, 1, 3, 0),
            (f"{name}.branch7x7dbl_5", c7, 192, 1, 7, 1, 0, 3), (f"{name}.branch_pool", 768, 192, 1, 1, 1, 0, 0)]


def _e(name, cin):
    return [(f"{name}.branch1x1", cin, 320, 1, 1, 1, 0, 0), (f"{name}.branch3x3_1", cin, 384, 1, 1, 1, 0, 0),
            (f"{name}.branch3x3_2a", 384, 384, 1, 3, 1, 0, 1), (f"{name}.branch3x3_2b", 384, 384, 3, 1, 1, 1, 0),
            (f"{name}.branch3x3dbl_1", cin, 448, 1, 1, 1, 0, 0), (f"{name}.branch3x3dbl_2", 448, 384, 3, 3, 1, 1, 1),
            (f"{name}.branch3x3dbl_3a", 384, 384, 1, 3, 1, 0, 1), (f"{name}.branch3x3dbl_3b", 384, 384, 3, 1, 1, 1, 0),
            (f"{name}.branch_pool", cin, 192, 1, 1, 1, 0, 0)]


# (name, Cin, Cout, kh, kw, stride, pad_h, pad_w) of the 94 BasicConv2d of inception.py:82-99, in its order
CONVS = ([("Conv2d_1a_3x3", 3, 32, 3, 3, 2, 0, 0), ("Conv2d_2a_3x3", 32, 32, 3, 3, 1, 0, 0), ("Conv2d_2b_3x3", 32, 64, 3, 3, 1, 1, 1),
          ("Conv2d_3b_1x1", 64, 80, 1, 1, 1, 0, 0), ("Conv2d_4a_3x3", 80, 192, 3, 3, 1, 0, 0)]
         + _a("Mixed_5b", 192, 32) + _a("Mixed_5c", 256, 64) + _a("Mixed_5d", 288, 64)
         + [("Mixed_6a.branch3x3", 288, 384, 3, 3, 2, 0, 0), ("Mixed_6a.branch3x3dbl_1", 288, 64, 1, 1, 1, 0, 0),
            ("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1), ("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 3, 2, 0, 0)]
         + _c("Mixed_6b", 128) + _c("Mixed_6c", 160) + _c("Mixed_6d", 160) + _c("Mixed_6e", 192)
         + [("Mixed_7a.branch3x3_1", 768, 192, 1, 1, 1, 0, 0), ("Mixed_7a.branch3x3_2", 192, 320, 3, 3, 2, 0, 0),
            ("Mixed_7a.branch7x7x3_1", 768, 192, 1, 1, 1, 0, 0), ("Mixed_7a.branch7x7x3_2", 192, 192, 1, 7, 1, 0, 3),
            ("Mixed_7a.branch7x7x3_3", 192, 192, 7, 1, 1, 3, 0), ("Mixed_7a.branch7x7x3_4", 192, 192, 3, 3, 2, 0, 0)]
         + _e("Mixed_7b", 1280) + _e("Mixed_7c", 2048))
CONV_SPEC = {c[0]: c[1:] for c in CONVS}
BN_KEYS = ("weight", "bias", "running_mean", "running_var")
MIN_INPUT = 75


def expected_keys():
    """the keys the forward needs (num_batches_tracked and AuxLogits.* are not among them)"""
    keys = []
    for n in CONV_SPEC:
        keys.append(f"{n}.conv.weight")
        keys += [f"{n}.bn.{k}" for k in BN_KEYS]
    return keys + ["fc.weight", "fc.bias"]


def fold_bn(w, gamma, beta, mean, var, eps=BN_EPS):
    """conv weight [Cout,Cin,kh,kw] and its BatchNorm's four vectors -> (w', b') in float64: bn(conv(x, w)) == conv(x, w') + b'"""
    w, gamma, beta, mean, var = (t.detach().to(torch.float64).cpu() for t in (w, gamma, beta, mean, var))
    scale = gamma / torch.sqrt(var + eps)
    return w * scale[:, None, None, None], beta - mean * scale


# ------------------------------------------------------------------------------------------------- preprocess tables
def resize_size(H, W_, size=SIZE):
    """transforms.Resize(size) on an H x W image (utils.py:24): the short side to `size`, the long one int(size * long / short)"""
    if W_ <= H:
        return int(size * H / W_), size
    return size, int(size * W_ / H)


def crop_offset(n, size=SIZE):
    """transforms.CenterCrop(size) along an axis of n >= size pixels (utils.py:25): int(round((n - size) / 2))"""
    return int(round((n - size) / 2.0))


def pil_bilinear_tables(n_in, n_out):
    """PIL's ImagingResample coefficients of a BILINEAR resize of n_in pixels to n_out along one axis, for 8-bit images:
    (bounds int32 [n_out,2] = (first input pixel, taps), coef int32 [n_out,ksize] in 22-bit fixed point).  float64 as PIL's
    doubles: scale = n_in / n_out, support = max(scale, 1), centre = (j + 0.5) scale, first = max(int(centre - support + 0.5), 0),
    last = min(int(centre + support + 0.5), n_in), weight t = triangle((t + first - centre + 0.5) / max(scale, 1)), divided by
    their sum taken in tap order, then int(0.5 + w 2^22) (int(-0.5 + ...) for a negative weight)."""
    scale = float(n_in) / float(n_out)
    fscale = max(scale, 1.0)
    support = 1.0 * fscale
    ksize = int(np.ceil(support)) * 2 + 1
    j = np.arange(n_out, dtype=np.float64)
    center = (j + 0.5) * scale
    first = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    last = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in)
    taps = last - first
    ss = 1.0 / fscale
    w = np.zeros((n_out, ksize), dtype=np.float64)
    total = np.zeros(n_out, dtype=np.float64)
    for t in range(ksize):
        a = np.abs((t + first - center + 0.5) * ss)
        v = np.where((a < 1.0) & (t < taps), 1.0 - a, 0.0)
        w[:, t] = v
        total = total + v
    w = np.where(total[:, None] != 0.0, w / np.where(total == 0.0, 1.0, total)[:, None], w)
    fixed = np.where(w < 0, np.trunc(-0.5 + w * (1 << PIL_BITS)), np.trunc(0.5 + w * (1 << PIL_BITS))).astype(np.int32)
    return np.stack([first, taps], 1).astype(np.int32), fixed


VARIANTS = ("torchvision", "fid")


def normalize_lut(variant="torchvision"):
    """fp32 [3,256]: ToTensor and Normalize (utils.py:26-27) of every byte, evaluated by torch on the CPU exactly as the
    transforms do - u8.float().div(255).sub(mean).div(std) - so a lookup is bit-identical to them by construction.
    variant "fid": pytorch-fid's 2 * (b / 255) - 1 (its ToTensor, then normalize_input), the same for the three channels"""
    u = torch.arange(256, dtype=torch.int32).to(torch.uint8).to(torch.float32).div(255)
    if variant == "fid":
        return (2 * u - 1)[None, :].repeat(3, 1).contiguous()
    mean, std = torch.tensor(MEAN, dtype=torch.float32), torch.tensor(STD, dtype=torch.float32)
    return u[None, :].repeat(3, 1).sub(mean[:, None]).div(std[:, None]).contiguous()


class PreprocessTables:
    """everything mmh_inception_preprocess needs for H x W images: the two passes' tables, the crop window, the lookup table"""

    def __init__(self, H, W_, size=SIZE, device=None, variant="torchvision"):
        self.H, self.W, self.size = int(H), int(W_), int(size)
        self.rh, self.rw = resize_size(self.H, self.W, size)
        self.oh = self.ow = int(size)
        self.crop_y, self.crop_x = crop_offset(self.rh, size), crop_offset(self.rw, size)
        hb, hk = pil_bilinear_tables(self.W, self.rw)
        vb, vk = pil_bilinear_tables(self.H, self.rh)
        self.hks, self.vks = int(hk.shape[1]), int(vk.shape[1])
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)     # noqa: E731
        self.hbounds, self.hcoef, self.vbounds, self.vcoef = put(hb), put(hk), put(vb), put(vk)
        self.lut = normalize_lut(variant).to(device)


# ------------------------------------------------------------------------------------------------- the network
class InceptionV3:
    """inception.py:61-176 (Inception3, eval, transform_input=False).  forward(x fp32 [B,H,W,4], H, W >= 75; lanes 0..2 the
    normalised R, G, B, lane 3 zero) -> logits fp32 [B,1000].

    variant "fid": pytorch-fid's graph for its pt_inception-2015-12-05 weights (FIDInceptionA / C / E_1 / E_2): the average
    pools of the A, C and E blocks divide by the number of in-image pixels, Mixed_7c's pool branch is a 3x3 stride-1 max pool,
    fc may be [1008,2048] and is not used - features() only.  The default variant's launches and bits are what they were."""

    def __init__(self, device=None, variant="torchvision"):
        if variant not in VARIANTS:
            raise ValueError(f"InceptionV3: variant {variant!r}: {' | '.join(VARIANTS)}")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.variant = variant
        self._avg = "avg_valid" if variant == "fid" else "avg"
        self.convs = None

    def load_state_dict(self, sd):
        sd = strip_module(sd)
        fid = self.variant == "fid"
        missing = [k for k in expected_keys() if k not in sd and not (fid and k.startswith("fc."))]
        if missing:
            raise KeyError(f"InceptionV3: checkpoint lacks {missing[:4]}{' ...' if len(missing) > 4 else ''}")
        convs = {}
        for n, (cin, cout, kh, kw, _, _, _) in CONV_SPEC.items():
            if tuple(sd[f"{n}.conv.weight"].shape) != (cout, cin, kh, kw):
                raise ValueError(f"InceptionV3: {n}.conv.weight is {tuple(sd[f'{n}.conv.weight'].shape)}, expected {(cout, cin, kh, kw)}")
            w, b = fold_bn(sd[f"{n}.conv.weight"], *(sd[f"{n}.bn.{k}"] for k in BN_KEYS))
            convs[n] = tuple(t.to(self.device) for t in relay_conv(w, b, cin_p=ops.pad4(cin)))
        if fid:
            self.fc = None
        else:
            if tuple(sd["fc.weight"].shape) != (1000, 2048):
                raise ValueError(f"InceptionV3: fc.weight is {tuple(sd['fc.weight'].shape)}, expected (1000, 2048)")
            self.fc = tuple(t.to(self.device) for t in relay_fc(sd["fc.weight"], sd["fc.bias"]))
        self.convs = convs
        return self

    # ---- one conv: src lanes [x_off, x_off + Cin) of x -> lanes [y_off, y_off + Cout) of out (a new tensor if None)
    def _conv(self, name, x, x_off=0, out=None, y_off=0):
        _, _, kh, kw, stride, ph, pw = CONV_SPEC[name]
        w, b = self.convs[name]
        return ops.conv_fprop_direct(x, w, b, ph, pw, stride, L.ACT_RELU, x_off, out, y_off, rect=kh != kw)

    def _chain(self, names, x, out, y_off):
        for n in names[:-1]:
            x = self._conv(n, x)
        return self._conv(names[-1], x, 0, out, y_off)

    def _block_a(self, p, x, pool):
        B, H, W_, _ = x.shape
        out = ops._empty((B, H, W_, 224 + pool), x)
        self._conv(f"{p}.branch1x1", x, 0, out, 0)
        self._chain([f"{p}.branch5x5_1", f"{p}.branch5x5_2"], x, out, 64)
        self._chain([f"{p}.branch3x3dbl_1", f"{p}.branch3x3dbl_2", f"{p}.branch3x3dbl_3"], x, out, 128)
        self._conv(f"{p}.branch_pool", ops.pool3x3(x, self._avg), 0, out, 224)
        return out

    def _block_b(self, p, x):
        B, H, W_, cin = x.shape
        out = ops._empty((B, (H - 3) // 2 + 1, (W_ - 3) // 2 + 1, 480 + cin), x)
        self._conv(f"{p}.branch3x3", x, 0, out, 0)
        self._chain([f"{p}.branch3x3dbl_1", f"{p}.branch3x3dbl_2", f"{p}.branch3x3dbl_3"], x, out, 384)
        ops.pool3x3(x, "max", out=out, y_off=480)
        return out

    def _block_c(self, p, x):
        B, H, W_, _ = x.shape
        out = ops._empty((B, H, W_, 768), x)
        self._conv(f"{p}.branch1x1", x, 0, out, 0)
        self._chain([f"{p}.branch7x7_{i}" for i in (1, 2, 3)], x, out, 192)
        self._chain([f"{p}.branch7x7dbl_{i}" for i in (1, 2, 3, 4, 5)], x, out, 384)
        self._conv(f"{p}.branch_pool", ops.pool3x3(x, self._avg), 0, out, 576)
        return out

    def _block_d(self, p, x):
        B, H, W_, cin = x.shape
        out = ops._empty((B, (H - 3) // 2 + 1, (W_ - 3) // 2 + 1, 512 + cin), x)
        self._chain([f"{p}.branch3x3_1", f"{p}.branch3x3_2"], x, out, 0)
        self._chain([f"{p}.branch7x7x3_{i}" for i in (1, 2, 3, 4)], x, out, 320)
        ops.pool3x3(x, "max", out=out, y_off=512)
        return out

    def _block_e(self, p, x, pool=None):
        B, H, W_, _ = x.shape
        out = ops._empty((B, H, W_, 2048), x)
        self._conv(f"{p}.branch1x1", x, 0, out, 0)
        t = self._conv(f"{p}.branch3x3_1", x)
        self._conv(f"{p}.branch3x3_2a", t, 0, out, 320)
        self._conv(f"{p}.branch3x3_2b", t, 0, out, 704)
        t = self._conv(f"{p}.branch3x3dbl_2", self._conv(f"{p}.branch3x3dbl_1", x))
        self._conv(f"{p}.branch3x3dbl_3a", t, 0, out, 1088)
        self._conv(f"{p}.branch3x3dbl_3b", t, 0, out, 1472)
        self._conv(f"{p}.branch_pool", ops.pool3x3(x, pool or self._avg), 0, out, 1856)
        return out

    @torch.no_grad()
    def features(self, x):
        """-> the pooled 2048 features fp32 [B,2048] (the input of fc)"""
        assert self.convs is not None, "load_state_dict first"
        ops._chk(x, "x")
        if x.dim() != 4 or x.shape[3] != 4 or x.shape[1] < MIN_INPUT or x.shape[2] < MIN_INPUT:
            raise ValueError(f"InceptionV3: expected fp32 [B,H,W,4] with H, W >= {MIN_INPUT}, got {tuple(x.shape)}")
        with direct_two_level():
            for n in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
                x = self._conv(n, x)
            x = ops.pool3x3(x, "max")
            x = self._conv("Conv2d_4a_3x3", self._conv("Conv2d_3b_1x1", x))
            x = ops.pool3x3(x, "max")
            x = self._block_a("Mixed_5b", x, 32)
            x = self._block_a("Mixed_5c", x, 64)
            x = self._block_a("Mixed_5d", x, 64)
            x = self._block_b("Mixed_6a", x)
            for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
                x = self._block_c(n, x)
            x = self._block_d("Mixed_7a", x)
            x = self._block_e("Mixed_7b", x)
            x = self._block_e("Mixed_7c", x, "max_s1" if self.variant == "fid" else None)
        return ops.global_avgpool(x)

    @torch.no_grad()
    def forward(self, x):
        return self.logits_of(self.features(x))

    @torch.no_grad()
    def logits_of(self, f):
        """features() -> logits: the fc layer alone (one forward serves the Inception score and FID)"""
        if self.fc is None:
            raise RuntimeError("InceptionV3: the 'fid' variant has no classifier - features() only")
        wt, b = self.fc
        B = f.shape[0]
        return torch.cat([ops.linear(f[i:i + 64], wt, b) for i in range(0, B, 64)]) if B > 64 else ops.linear(f, wt, b)

    __call__ = forward


# ------------------------------------------------------------------------------------------------- the score
def group_bounds(n, group):
    """consecutive groups of `group` images and a non-empty tail on its own (Evaluator.evaluate() forces it, utils.py:64-65)"""
    if group < 1:
        raise ValueError(f"group {group}: at least one image per group")
    return [(i, min(i + group, n)) for i in range(0, n, group)]


class InceptionScorer:
    """Evaluator._get_IS_score / inception_score(splits=1) (utils.py:81-98,196-232) for batches: feed() enqueues preprocess ->
    InceptionV3 and keeps the logits on the device; results() scores them group by group with mmh_inception_score."""

    def __init__(self, net, group=64, device=None, size=SIZE):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if not isinstance(net, InceptionV3):
            is_path = isinstance(net, (str, bytes)) or hasattr(net, "__fspath__")
            net = InceptionV3(self.device).load_state_dict(torch.load(net, map_location="cpu") if is_path else net)
        group_bounds(0, group)
        self.net, self.group, self.size = net, int(group), int(size)
        self._tables, self._logits, self._rows = {}, [], []

    def tables(self, H, W_):
        key = (int(H), int(W_))
        if key not in self._tables:
            self._tables[key] = PreprocessTables(H, W_, self.size, self.device)
        return self._tables[key]

    @torch.no_grad()
    def logits(self, images, layout="nchw"):
        H, W_ = (images.shape[2], images.shape[3]) if layout == "nchw" else (images.shape[1], images.shape[2])
        return self.net(ops.inception_preprocess(images, layout, self.tables(H, W_)))

    def feed(self, images, layout="nchw", paths=None):
        """images: one batch (see ops.inception_preprocess); paths: None or one dict per image, copied into its row"""
        B = images.shape[0]
        if paths is not None and len(paths) != B:
            raise ValueError(f"feed: {B} images, {len(paths)} paths")
        self._logits.append(self.logits(images, layout))
        self._rows += [dict(r) for r in paths] if paths is not None else [{} for _ in range(B)]

    def feed_features(self, features, paths=None):
        """feed() for a batch whose pooled features another consumer of the same network already computed (mmhand_amd.fid):
        only the fc layer runs; the logits are those of feed() on the same images, bit for bit"""
        B = features.shape[0]
        if paths is not None and len(paths) != B:
            raise ValueError(f"feed_features: {B} rows, {len(paths)} paths")
        self._logits.append(self.net.logits_of(features))
        self._rows += [dict(r) for r in paths] if paths is not None else [{} for _ in range(B)]

    def results(self):
        """{"IS_avg", "IS_std": np.mean / np.std over the groups' scores (the reference's keys, utils.py:67-68), "IS_all": one
        group over every image, "n_groups", "kl": per image, against its own group's py, "rows": per-image dicts with is_kl}"""
        if not self._logits:
            return {"IS_avg": None, "IS_std": None, "IS_all": None, "n_groups": 0, "kl": [], "rows": []}
        lg = torch.cat(self._logits).contiguous()
        scores, kls = [], []
        for lo, hi in group_bounds(lg.shape[0], self.group):
            kl = ops.inception_score(lg[lo:hi])[0].cpu().numpy()
            kls.append(kl)
            scores.append(float(np.exp(np.mean(kl))))
        kl_all = np.concatenate(kls)
        is_all = float(np.exp(np.mean(ops.inception_score(lg)[0].cpu().numpy())))
        rows = [dict(r, is_kl=float(k)) for r, k in zip(self._rows, kl_all)]
        return {"IS_avg": float(np.mean(scores)), "IS_std": float(np.std(scores)), "IS_all": is_all, "n_groups": len(scores),
                "kl": kl_all.tolist(), "rows": rows}
