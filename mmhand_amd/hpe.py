"""The reference Evaluator's pose metric on the device: PCK / AUC / end-point error of a 2D hand-pose machine and its 3D lift
(baselines/quantitative_on_benchmarks/hpe_estimator.py:7-143, networks/net_hpm2d.py, networks/net_hpm3d.py).

`Hpm2d` and `Hpm3d` are inference-only.  They load the reference's checkpoints (keys conv1_1.weight ... stage6.conv7.bias,
depth.*, depth_fc_*; a leading "module." is stripped), read every width from the tensors' shapes and re-lay the weights once:

* conv weights [Cout,Cin,k,k] -> RSCK [k,k,Cin',Cout'] fp32, Cin' / Cout' zero-padded to multiples of 4 (the 21 joints to 24);
* the reference's cat((heat, out_0), 1) is one buffer [B,h,w,24 + C0']: conv5_3_CPM writes lanes 24.., conv6_2_CPM and every
  stage's conv7 write lanes 0..23 through the conv's y_cs, and each stage's conv1 has zero rows for lanes 21..23;
* depth_fc_1's columns go from the reference's (c, y, x) flatten order to (y, x, c') with zero rows for c' >= 21, the three
  Linear weights are stored transposed [K,N], the last one's 21 outputs padded to 24.

The forward is mmh_conv2d_fprop (fp32 direct kernels, zero padding, fused ReLU; conv_levels = DIRECT_LEVELS for the duration
of the call and put back, whatever ops.set_winograd_mode says), mmh_maxpool2x2_fwd, and the three passes of csrc/hpe.hip:
ops.hpe_normalize, ops.heatmap_upsample_argmax, ops.linear.  No pretrained estimator weights exist in this repository or the
reference's: every number produced with generated weights says nothing about a generator."""
import contextlib
import ctypes as C
import math

import numpy as np
import torch

from . import lib as L
from . import ops

JOINTS, JLANES = 21, 24
TRUNK = ("conv1_1", "conv1_2", "pool", "conv2_1", "conv2_2", "pool", "conv3_1", "conv3_2", "conv3_3", "conv3_4", "pool",
         "conv4_1", "conv4_2", "conv4_3", "conv4_4", "conv5_1", "conv5_2")
REPEAT = ("conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7")
# ground-truth z in pixel units: RHD_dataset.py:123 (depth * 700) with hpe_estimator.py:122 (/ 700 * 256) = depth * 256;
# STB_dataset.py:164 hands the label's depth over as it is, so hpe_estimator.py:122 leaves depth / 700 * 256
Z_SCALE = {"rhd": 256.0, "stb": 256.0 / 700.0}


def strip_module(sd):
    """hpe_estimator.py:145-156: DataParallel checkpoints carry a leading 'module.'"""
    return type(sd)((k[len("module."):] if k.startswith("module.") else k, v) for k, v in sd.items())


def relay_conv(w, b, rows=None, cin_p=None):
    """nn.Conv2d weight [Cout,Cin,k,k] + bias -> (RSCK fp32 [k,k,cin_p,pad4(Cout)], bias [pad4(Cout)]); rows[i] = the lane of
    the physical input that the reference's input channel i reads (default i); every other row and column is zero."""
    w = w.detach().to(torch.float32).cpu()
    cout, cin, kh, kw = w.shape
    rows = torch.arange(cin) if rows is None else torch.as_tensor(rows, dtype=torch.long)
    cin_p = ops.pad4(int(rows.max()) + 1) if cin_p is None else cin_p
    out = torch.zeros((kh, kw, cin_p, ops.pad4(cout)), dtype=torch.float32)
    out[:, :, rows, :cout] = w.permute(2, 3, 1, 0)
    bias = torch.zeros(ops.pad4(cout), dtype=torch.float32)
    if b is not None:
        bias[:cout] = b.detach().to(torch.float32).cpu()
    return out.contiguous(), bias


def relay_fc1(w, b, hs, ws):
    """depth_fc_1.weight [N, 21*hs*ws] over the reference's (c, y, x) flatten -> wt [hs*ws*24, pad4(N)] over (y, x, c')"""
    w = w.detach().to(torch.float32).cpu()
    n = w.shape[0]
    assert w.shape[1] == JOINTS * hs * ws, (tuple(w.shape), hs, ws)
    wt = torch.zeros((hs, ws, JLANES, ops.pad4(n)), dtype=torch.float32)
    wt[:, :, :JOINTS, :n] = w.reshape(n, JOINTS, hs, ws).permute(2, 3, 1, 0)
    return wt.reshape(hs * ws * JLANES, ops.pad4(n)).contiguous(), _pad_vec(b, ops.pad4(n))


def relay_fc(w, b, k_p=None):
    """nn.Linear weight [N,K] -> wt [k_p, pad4(N)] (zero rows / columns beyond K / N)"""
    w = w.detach().to(torch.float32).cpu()
    n, k = w.shape
    wt = torch.zeros((k_p or k, ops.pad4(n)), dtype=torch.float32)
    wt[:k, :n] = w.t()
    return wt.contiguous(), _pad_vec(b, ops.pad4(n))


def _pad_vec(b, n):
    out = torch.zeros(n, dtype=torch.float32)
    out[:b.shape[0]] = b.detach().to(torch.float32).cpu()
    return out


# summation levels of the direct fp32 fprop during an estimator forward (mmh_set_option("conv_levels")).  Two levels exist for
# convs with more than 64 output channels on the chunk-major k order: here conv2_1 .. conv5_3_CPM, conv6_1_CPM and every
# stage's conv1 .. conv6 at full width.  The 64-channel convs and the 24-lane heat-map convs (conv6_2_CPM, each conv7) have
# one level under either value.  DESIGN 4.5g gives the measured distances of both settings.
DIRECT_LEVELS = 2


@contextlib.contextmanager
def direct_two_level():
    """conv_levels = DIRECT_LEVELS for the duration of the block, so that the forward is the same whatever
    ops.set_winograd_mode left behind; the process-wide option is put back.  The option is a global of the library: a second
    thread launching convolutions during the block would see it (nothing in this package does that)."""
    old = L.get_option("conv_levels")
    L.call("mmh_set_option", b"conv_levels", DIRECT_LEVELS)
    try:
        yield
    finally:
        L.call("mmh_set_option", b"conv_levels", old)


def _conv(x, x_off, x_cs, w, bias, y, y_off, y_cs, B, H, W_, act):
    """one mmh_conv2d_fprop: x / y are NHWC buffers read / written from lane x_off / y_off with pixel strides x_cs / y_cs"""
    k, _, cin, cout = w.shape
    d = ops.conv_desc(B, H, W_, cin, cout, k, 1, k // 2, False, x_cs=x_cs, y_cs=y_cs)
    L.call("mmh_conv2d_fprop", C.byref(d), C.c_void_p(x.data_ptr() + 4 * x_off), ops._ptr(w), ops._ptr(bias),
           C.c_void_p(y.data_ptr() + 4 * y_off), act, ops._stream())


class _PoseMachine:
    """the layers Hpm2d and Hpm3d share: the VGG-style trunk, the CPM head and `stages` Repeat blocks on the cat buffer"""

    STAGES = ()

    def __init__(self, device=None):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.convs = None

    # ---- checkpoint -> device weights
    def _put(self, name, pair):
        self.convs[name] = tuple(t.to(self.device) for t in pair)

    def load_state_dict(self, sd):
        sd = strip_module(sd)
        missing = [k for k in self.expected_keys() if k not in sd]
        if missing:
            raise KeyError(f"{type(self).__name__}: checkpoint lacks {missing[:4]}{' ...' if len(missing) > 4 else ''}")
        if sd["conv6_2_CPM.weight"].shape[0] != JOINTS:
            raise ValueError(f"{type(self).__name__}: {sd['conv6_2_CPM.weight'].shape[0]} joints in the checkpoint, 21 expected")
        self.convs = {}
        self.in_nc = int(sd["conv1_1.weight"].shape[1])
        for n in (t for t in TRUNK if t != "pool"):
            self._put(n, relay_conv(sd[n + ".weight"], sd[n + ".bias"]))
        for n in ("conv5_3_CPM", "conv6_1_CPM", "conv6_2_CPM"):
            self._put(n, relay_conv(sd[n + ".weight"], sd[n + ".bias"]))
        self.c0 = int(sd["conv5_3_CPM.weight"].shape[0])
        self.cat = JLANES + ops.pad4(self.c0)
        rows = list(range(JOINTS)) + [JLANES + i for i in range(self.c0)]       # cat((heat, out_0)): heat first
        for s in self.STAGES:
            if sd[f"{s}.conv1.weight"].shape[1] != JOINTS + self.c0:
                raise ValueError(f"{s}.conv1 reads {sd[f'{s}.conv1.weight'].shape[1]} channels, {JOINTS + self.c0} expected")
            self._put(f"{s}.conv1", relay_conv(sd[f"{s}.conv1.weight"], sd[f"{s}.conv1.bias"], rows=rows, cin_p=self.cat))
            for c in REPEAT[1:]:
                self._put(f"{s}.{c}", relay_conv(sd[f"{s}.{c}.weight"], sd[f"{s}.{c}.bias"]))
        self._load_head(sd)
        return self

    def expected_keys(self):
        names = [t for t in TRUNK if t != "pool"] + ["conv5_3_CPM", "conv6_1_CPM", "conv6_2_CPM"]
        names += [f"{s}.{c}" for s in self.STAGES for c in REPEAT]
        return [f"{n}.{p}" for n in names + self._head_names() for p in ("weight", "bias")]

    def _head_names(self):
        return []

    def _load_head(self, sd):
        pass

    # ---- forward
    def _run(self, x):
        """x: fp32 [B,H,W,pad4(in_nc)] -> (the cat buffer [B,h,w,24 + C0'] with the CPM head's heat maps in lanes 0..20, zeros in
        21..23 and out_0 from lane 24, (B, h, w))"""
        assert self.convs is not None, "load_state_dict first"
        ops._chk(x, "x")
        B, H, W_, cx = x.shape
        assert H % 8 == 0 and W_ % 8 == 0 and cx == ops.pad4(self.in_nc), (tuple(x.shape), self.in_nc)
        for n in TRUNK:
            if n == "pool":
                y = ops._empty((B, H // 2, W_ // 2, x.shape[3]), x)
                L.call("mmh_maxpool2x2_fwd", ops._ptr(x), B, H, W_, x.shape[3], ops._ptr(y), ops._stream())
                H, W_ = H // 2, W_ // 2
            else:
                w, b = self.convs[n]
                y = ops._empty((B, H, W_, w.shape[3]), x)
                _conv(x, 0, x.shape[3], w, b, y, 0, w.shape[3], B, H, W_, L.ACT_RELU)
            x = y
        cat = ops._empty((B, H, W_, self.cat), x)
        w, b = self.convs["conv5_3_CPM"]
        _conv(x, 0, x.shape[3], w, b, cat, JLANES, self.cat, B, H, W_, L.ACT_RELU)
        w, b = self.convs["conv6_1_CPM"]
        t = ops._empty((B, H, W_, w.shape[3]), x)
        _conv(cat, JLANES, self.cat, w, b, t, 0, w.shape[3], B, H, W_, L.ACT_RELU)
        w, b = self.convs["conv6_2_CPM"]
        _conv(t, 0, t.shape[3], w, b, cat, 0, self.cat, B, H, W_, L.ACT_NONE)
        return cat, (B, H, W_)

    def _repeat(self, s, cat, shape, out, out_cs):
        """one Repeat block reading the cat buffer; its conv7 writes lanes 0..23 of `out` (pixel stride out_cs)"""
        B, H, W_ = shape
        x, x_cs = cat, self.cat
        for c in REPEAT[:-1]:
            w, b = self.convs[f"{s}.{c}"]
            y = ops._empty((B, H, W_, w.shape[3]), cat)
            _conv(x, 0, x_cs, w, b, y, 0, w.shape[3], B, H, W_, L.ACT_RELU)
            x, x_cs = y, w.shape[3]
        w, b = self.convs[f"{s}.conv7"]
        _conv(x, 0, x_cs, w, b, out, 0, out_cs, B, H, W_, L.ACT_NONE)


class Hpm2d(_PoseMachine):
    """networks/net_hpm2d.py:26-119 with input_nc 3.  forward(x fp32 [B,H,W,4]) -> the cat buffer [B,H/8,W/8,24 + C0'] whose
    lanes 0..20 are the last stage's heat maps (what hpe_estimator.py:124 takes, before the upsample)."""

    STAGES = ("stage2", "stage3", "stage4", "stage5", "stage6")

    @torch.no_grad()
    def forward(self, x):
        with direct_two_level():
            cat, shape = self._run(x)
            for s in self.STAGES:
                self._repeat(s, cat, shape, cat, self.cat)
        return cat

    __call__ = forward


class Hpm3d(_PoseMachine):
    """networks/net_hpm3d.py:26-115 with input_nc 21.  forward(up fp32 [B,H,W,24], the upsampled heat maps) -> depths fp32
    [B,24] (lanes 21..23 zero).  stage6's weights are in the checkpoint and unused, as in the reference's forward."""

    STAGES = ("stage2", "stage3", "stage4", "stage5", "depth")

    def _head_names(self):
        return ["stage6." + c for c in REPEAT] + ["depth_fc_1", "depth_fc_2", "depth_fc_3"]

    def _load_head(self, sd):
        k1 = int(sd["depth_fc_1.weight"].shape[1])
        hs = math.isqrt(k1 // JOINTS)
        if hs * hs * JOINTS != k1:
            raise ValueError(f"depth_fc_1 reads {k1} values: not 21 square maps")
        self.head_hw = hs
        self.fc = [tuple(t.to(self.device) for t in relay_fc1(sd["depth_fc_1.weight"], sd["depth_fc_1.bias"], hs, hs))]
        for n in ("depth_fc_2", "depth_fc_3"):
            wt, b = relay_fc(sd[n + ".weight"], sd[n + ".bias"], k_p=self.fc[-1][0].shape[1])
            self.fc.append((wt.to(self.device), b.to(self.device)))

    @torch.no_grad()
    def forward(self, x):
        with direct_two_level():
            cat, shape = self._run(x)
            for s in self.STAGES[:-1]:
                self._repeat(s, cat, shape, cat, self.cat)
            B, H, W_ = shape
            if (H, W_) != (self.head_hw, self.head_hw):
                raise ValueError(f"Hpm3d: depth_fc_1 was trained on {self.head_hw * 8}^2 inputs, got {H * 8} x {W_ * 8}")
            d = ops._empty((B, H, W_, JLANES), cat)
            self._repeat("depth", cat, shape, d, JLANES)
        z = d.view(B, H * W_ * JLANES)
        for wt, b in self.fc:
            z = torch.cat([ops.linear(z[i:i + 64], wt, b) for i in range(0, B, 64)]) if B > 64 else ops.linear(z, wt, b)
        return z

    __call__ = forward


def pck_measures(dist, max_px=30, steps=20):
    """EvalUtil.get_measures(0, max_px, steps) (hpe_estimator.py:55-95) of dist [n_images, n_joints] (every joint visible):
    per joint the mean / median distance, the PCK curve mean(dist <= t) over t = linspace(0, max_px, steps) and its trapezoid
    area over the thresholds' span; then the means over the joints.  float64 on the host."""
    dist = np.asarray(dist, dtype=np.float64)
    thresholds = np.linspace(0, max_px, steps)

    def trapz(y):
        return float(np.sum(np.diff(thresholds) * (y[1:] + y[:-1]) / 2.0))

    norm = trapz(np.ones_like(thresholds))
    if dist.size == 0:
        return {"epe_mean": None, "epe_median": None, "auc": None, "curve": [], "thresholds": thresholds.tolist()}
    means, medians, aucs, curves = [], [], [], []
    for j in range(dist.shape[1]):
        data = dist[:, j]
        means.append(np.mean(data))
        medians.append(np.median(data))
        curve = np.array([np.mean((data <= t).astype("float")) for t in thresholds])
        curves.append(curve)
        aucs.append(trapz(curve) / norm)
    return {"epe_mean": float(np.mean(means)), "epe_median": float(np.mean(medians)), "auc": float(np.mean(aucs)),
            "curve": np.mean(np.array(curves), 0).tolist(), "thresholds": thresholds.tolist()}


class HPEstimator:
    """hpe_estimator.py:97-143 for batches.  feed() enqueues normalise -> Hpm2d -> upsample + arg-max [-> Hpm3d] and keeps the
    predictions (21 pixels and 21 depths per image) on the device; results() reads them back once and does EvalUtil's
    arithmetic on the host in float64.  hpm3d None: only the 2D figures.
    z_scale: ground-truth z = label depth * z_scale (Z_SCALE: "rhd" 256, "stb" 256 / 700); predicted z = output * image height
    (hpe_estimator.py:135).  Every image goes through the min-max normalisation the reference's datasets apply to real images
    (the reference hands generated images over as the generator left them; one input domain for both is this port's choice)."""

    def __init__(self, hpm2d, hpm3d=None, device=None, z_scale=256.0):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.hpm2d = self._net(Hpm2d, hpm2d)
        self.hpm3d = self._net(Hpm3d, hpm3d) if hpm3d is not None else None
        self.z_scale = float(z_scale)
        self._batches = []

    def _net(self, cls, src):
        if isinstance(src, _PoseMachine):
            return src
        is_path = isinstance(src, (str, bytes)) or hasattr(src, "__fspath__")
        return cls(self.device).load_state_dict(torch.load(src, map_location="cpu") if is_path else src)

    @torch.no_grad()
    def predict(self, images, layout="nchw"):
        """-> (xy int32 [B,21,2], z fp32 [B,21] in units of the image height or None), on the device"""
        x = ops.hpe_normalize(images, layout)
        cat = self.hpm2d(x)
        up, xy, _ = ops.heatmap_upsample_argmax(cat)
        z = self.hpm3d(up)[:, :JOINTS] if self.hpm3d is not None else None
        return xy, z

    def feed(self, images, uv, depth=None, paths=None, layout="nchw"):
        """images: one batch (see ops.hpe_normalize); uv [B,21,2]: the target joints in pixels of these images; depth [B,21]:
        the labels' depth (None: no 3D figures for this batch); paths: None or one dict per image, copied into its row"""
        uv = np.asarray(uv, dtype=np.float64).reshape(-1, JOINTS, 2)
        B, H = uv.shape[0], int(images.shape[2] if layout == "nchw" else images.shape[1])
        if images.shape[0] != B or (paths is not None and len(paths) != B):
            raise ValueError(f"feed: {images.shape[0]} images, {B} poses, {None if paths is None else len(paths)} paths")
        depth = None if depth is None else np.asarray(depth, dtype=np.float64).reshape(B, JOINTS)
        xy, z = self.predict(images, layout)
        self._batches.append((xy, z, uv, depth, H, paths))

    def distances(self):
        """(d2 [n,21], d3 [n,21] or None, rows): EvalUtil.feed's Euclidean distances (hpe_estimator.py:27-29), float64"""
        d2, d3, rows = [], [], []
        for xy, z, uv, depth, H, paths in self._batches:
            p = xy.cpu().numpy().astype(np.float64)
            diff = uv - p
            d2.append(np.sqrt(np.sum(np.square(diff), axis=2)))
            if z is not None and depth is not None:
                dz = depth * self.z_scale - z.cpu().numpy().astype(np.float64) * float(H)
                d3.append(np.sqrt(np.sum(np.square(np.concatenate([diff, dz[..., None]], 2)), axis=2)))
            rows += [dict(r) for r in paths] if paths is not None else [{} for _ in range(uv.shape[0])]
        d2 = np.concatenate(d2) if d2 else np.zeros((0, JOINTS))
        d3 = np.concatenate(d3) if d3 and len(d3) == len(self._batches) else None
        return d2, d3, rows

    def results(self, max_px=30, steps=20):
        """{"pck2d": measures, "pck3d": measures or None, "rows": per-image dicts with epe2d [, epe3d]} - the measures are
        pck_measures' (the reference's get_results(30, 20), hpe_estimator.py:140-143)"""
        d2, d3, rows = self.distances()
        for i, r in enumerate(rows):
            r["epe2d"] = float(np.mean(d2[i]))
            if d3 is not None:
                r["epe3d"] = float(np.mean(d3[i]))
        return {"pck2d": pck_measures(d2, max_px, steps), "pck3d": pck_measures(d3, max_px, steps) if d3 is not None else None,
                "rows": rows}
