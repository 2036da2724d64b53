"""Training the 2D hand-pose machine (networks/net_hpm2d.py) on the device: where the weights of `evaluate --pck` come from.

The reference has the network and the data mode that yields (image, 21 Gaussian heat maps at full resolution, sigma 5:
data/RHD_dataset.py:139-147,192-200,245-277) and no training loop in its tree.  The recipe here is this port's: loss =
sum over the six stage outputs of stage_weights[s] * nn.MSELoss()(upsample(out_s), target), Adam (lr 1e-4, betas 0.9 / 0.999).

`Hpm2dTrainer` keeps the padded RSCK layout of hpe.Hpm2d (hpe.relay_conv) as fp32 masters in one flat buffer, with the
gradients and Adam's two moments in three more of the same layout, so that one mmh_adam_step updates every parameter.
forward: the calls of hpe.Hpm2d's inference (mmh_conv2d_fprop with fused ReLU, mmh_maxpool2x2_fwd, under
hpe.direct_two_level()), keeping what the backward reads - except conv1_1, which runs on mmh_conv3x3_c4_fprop_f64 (float64
accumulation, one rounding): its ReLU masks are then those of exact arithmetic, and its gradients, summed over 27 inputs only,
do not hang on a mask that fp32 rounding flips.  Inference overwrites the heat lanes of ONE cat buffer; here every
stage's input cat buffer [B,h,w,24 + C0'] is kept (out_0 is computed densely once and copied into lanes 24.. of each).
backward: an explicit schedule, no autograd -
  mmh_heatmap_mse              the six losses and their gradients on the low-resolution maps, G_1 .. G_6 [B,h,w,24]
  stage6 .. stage2             conv7 .. conv1: mmh_act_bwd (ReLU), mmh_colsum (bias), mmh_conv2d_wgrad, mmh_conv2d_dgrad (fp32,
                               zero padding); conv1's input gradient [B,h,w,24 + C0'] is split by mmh_lane_add: lanes 0..23 onto
                               the previous output's G, lanes 24.. onto d_out0
  conv6_2_CPM, conv6_1_CPM     from G_1; conv6_1_CPM's input gradient is the sixth addend of d_out0
  conv5_3_CPM .. conv1_1       the trunk with mmh_maxpool2x2_bwd; conv1_1 needs no input gradient
Padding rows, columns and lanes stay exactly zero: their inputs, weights or output gradients are zero, so their gradients are
exact zeros and Adam moves a zero parameter with zero moments by zero."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import hpe
from . import lib as L
from . import ops
from .hpe import JLANES, JOINTS, REPEAT, TRUNK

STAGES = hpe.Hpm2d.STAGES
N_OUT = 1 + len(STAGES)
FULL_WIDTHS = dict(c1=64, c2=128, c3=256, c4=512, c0=128, cpm=512, rep=128)


def layer_shapes(widths=FULL_WIDTHS, in_nc=3):
    """[(name, (Cout, Cin, k, k))] of networks/net_hpm2d.py:40-67 in the order of its state dict"""
    w = widths
    chans = [in_nc, w["c1"], w["c1"], w["c2"], w["c2"], w["c3"], w["c3"], w["c3"], w["c3"], w["c4"], w["c4"], w["c4"], w["c4"],
             w["c4"], w["c4"]]
    names = [t for t in TRUNK if t != "pool"]
    out = [(n, (chans[i + 1], chans[i], 3, 3)) for i, n in enumerate(names)]
    out += [("conv5_3_CPM", (w["c0"], w["c4"], 3, 3)), ("conv6_1_CPM", (w["cpm"], w["c0"], 1, 1)),
            ("conv6_2_CPM", (JOINTS, w["cpm"], 1, 1))]
    for s in STAGES:
        out.append((f"{s}.conv1", (w["rep"], w["c0"] + JOINTS, 7, 7)))
        out += [(f"{s}.conv{i}", (w["rep"], w["rep"], 7, 7)) for i in (2, 3, 4, 5)]
        out += [(f"{s}.conv6", (w["rep"], w["rep"], 1, 1)), (f"{s}.conv7", (JOINTS, w["rep"], 1, 1))]
    return out


def init_state_dict(seed, widths=FULL_WIDTHS, in_nc=3):
    """torch's default nn.Conv2d initialisation: the modules themselves, constructed on the host in the state dict's order
    under torch.manual_seed(seed); the caller's random state is put back"""
    sd = OrderedDict()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(seed))
        for name, (cout, cin, k, _) in layer_shapes(widths, in_nc):
            conv = torch.nn.Conv2d(cin, cout, kernel_size=k, padding=k // 2)
            sd[name + ".weight"], sd[name + ".bias"] = conv.weight.detach().clone(), conv.bias.detach().clone()
    return sd


def linear_lr(lr, epoch, niter, niter_decay, epoch_count=1):
    """networks/networks.py:54-58: lr * (1 - max(0, epoch + epoch_count - niter) / (niter_decay + 1)), epoch counted from 0"""
    return lr * (1.0 - max(0, epoch + epoch_count - niter) / float(niter_decay + 1))


class Hpm2dTrainer:
    def __init__(self, device=None, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, sigma=5.0, stage_weights=None):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.lr, self.beta1, self.beta2, self.eps, self.sigma = float(lr), float(beta1), float(beta2), float(eps), float(sigma)
        self.stage_weights = [1.0] * N_OUT if stage_weights is None else [float(v) for v in stage_weights]
        if len(self.stage_weights) != N_OUT:
            raise ValueError(f"stage_weights: {N_OUT} values expected, got {len(self.stage_weights)}")
        self.steps = 0
        self.p = None

    # ---- checkpoint <-> the flat padded buffers
    def load_state_dict(self, sd):
        """the reference's keys (a leading 'module.' is stripped) -> masters; Adam's moments and the step count start at zero"""
        sd = hpe.strip_module(sd)
        probe = hpe.Hpm2d("cpu").load_state_dict(sd)            # its checks and its re-layout: the one definition of both
        self.in_nc, self.c0, self.cat = probe.in_nc, probe.c0, probe.cat
        if self.in_nc != 3 or probe.convs["conv1_1"][0].shape[3] > 256:
            raise ValueError(f"Hpm2dTrainer: conv1_1 reads {self.in_nc} channels and writes {sd['conv1_1.weight'].shape[0]}: the "
                             "training forward's first layer (mmh_conv3x3_c4_fprop_f64) takes 3 and at most 256")
        self.meta, off = OrderedDict(), 0
        for name, (w, b) in probe.convs.items():
            cout, cin = int(sd[name + ".weight"].shape[0]), int(sd[name + ".weight"].shape[1])
            rows = list(range(cin))
            if name.endswith(".conv1") and "." in name:
                rows = list(range(JOINTS)) + [JLANES + i for i in range(self.c0)]
            self.meta[name] = dict(shape=tuple(w.shape), cout=cout, cin=cin, rows=torch.tensor(rows), w_off=off,
                                   b_off=off + w.numel())
            off += w.numel() + b.numel()
        flat = torch.zeros(off, dtype=torch.float32)
        for name, (w, b) in probe.convs.items():
            m = self.meta[name]
            flat[m["w_off"]:m["b_off"]] = w.reshape(-1)
            flat[m["b_off"]:m["b_off"] + b.numel()] = b
        self.p = flat.to(self.device)
        self.g, self.m, self.v = (torch.zeros_like(self.p) for _ in range(3))
        self.steps = 0
        return self

    def _views(self, flat, name):
        m = self.meta[name]
        k, _, cin_p, cout_p = m["shape"]
        return flat[m["w_off"]:m["b_off"]].view(k, k, cin_p, cout_p), flat[m["b_off"]:m["b_off"] + cout_p]

    def state_dict(self):
        """the reference's keys and shapes (networks/net_hpm2d.py) on the host, fp32: what hpe.Hpm2d.load_state_dict and the
        reference module (strict=True) load"""
        assert self.p is not None, "load_state_dict first"
        flat, sd = self.p.cpu(), OrderedDict()
        for name, m in self.meta.items():
            w, b = self._views(flat, name)
            sd[name + ".weight"] = w[:, :, m["rows"], :m["cout"]].permute(3, 2, 0, 1).contiguous()
            sd[name + ".bias"] = b[:m["cout"]].clone()
        return sd

    def padding_mask(self):
        """bool, the flat buffers' layout: True where an element is padding (no element of the reference's tensors)"""
        mask = torch.ones(self.p.numel(), dtype=torch.bool)
        for name, m in self.meta.items():
            w, b = self._views(mask, name)
            w[:, :, m["rows"], :m["cout"]] = False
            b[:m["cout"]] = False
        return mask

    # ---- forward
    def _fprop(self, name, x, x_off, x_cs, y, y_off, y_cs, B, H, W_, act):
        w, b = self._views(self.p, name)
        hpe._conv(x, x_off, x_cs, w, b, y, y_off, y_cs, B, H, W_, act)

    def forward(self, x):
        """x: fp32 [B,H,W,pad4(in_nc)] (ops.hpe_normalize's output) -> the six cat-width buffers whose lanes 0..20 are the stage
        outputs out_1 .. out_6 (lanes 21..23 zero).  Keeps the activations for backward()."""
        assert self.p is not None, "load_state_dict first"
        ops._chk(x, "x")
        B, H, W_, cx = x.shape
        assert H % 8 == 0 and W_ % 8 == 0 and cx == ops.pad4(self.in_nc), (tuple(x.shape), self.in_nc)
        tape = []                                               # (name | "pool", input, output, H, W) of the trunk
        with hpe.direct_two_level():
            for n in TRUNK:
                if n == "pool":
                    y = ops._empty((B, H // 2, W_ // 2, x.shape[3]), x)
                    L.call("mmh_maxpool2x2_fwd", ops._ptr(x), B, H, W_, x.shape[3], ops._ptr(y), ops._stream())
                    tape.append((n, x, y, H, W_))
                    H, W_ = H // 2, W_ // 2
                else:
                    cout_p = self.meta[n]["shape"][3]
                    y = ops._empty((B, H, W_, cout_p), x)
                    if n == "conv1_1":
                        # float64 accumulation: this layer's ReLU masks decide gradients that are summed over 27 inputs only
                        w, b = self._views(self.p, n)
                        L.call("mmh_conv3x3_c4_fprop_f64", ops._ptr(x), ops._ptr(w), ops._ptr(b), ops._ptr(y), B, H, W_, cout_p,
                               cout_p, L.ACT_RELU, ops._stream())
                    else:
                        self._fprop(n, x, 0, x.shape[3], y, 0, cout_p, B, H, W_, L.ACT_RELU)
                    tape.append((n, x, y, H, W_))
                x = y
            out0 = ops._empty((B, H, W_, self.cat - JLANES), x)
            self._fprop("conv5_3_CPM", x, 0, x.shape[3], out0, 0, out0.shape[3], B, H, W_, L.ACT_RELU)
            tape.append(("conv5_3_CPM", x, out0, H, W_))
            t = ops._empty((B, H, W_, self.meta["conv6_1_CPM"]["shape"][3]), x)
            self._fprop("conv6_1_CPM", out0, 0, out0.shape[3], t, 0, t.shape[3], B, H, W_, L.ACT_RELU)
            cats = [torch.zeros((B, H, W_, self.cat), dtype=torch.float32, device=x.device) for _ in range(N_OUT)]
            self._fprop("conv6_2_CPM", t, 0, t.shape[3], cats[0], 0, self.cat, B, H, W_, L.ACT_NONE)
            acts = []
            for i, s in enumerate(STAGES):
                cats[i][..., JLANES:].copy_(out0)               # the reference's cat((out_i, out_0), 1)
                a, xin, x_cs = [], cats[i], self.cat
                for c in REPEAT[:-1]:
                    cout_p = self.meta[f"{s}.{c}"]["shape"][3]
                    y = ops._empty((B, H, W_, cout_p), x)
                    self._fprop(f"{s}.{c}", xin, 0, x_cs, y, 0, cout_p, B, H, W_, L.ACT_RELU)
                    a.append(y)
                    xin, x_cs = y, cout_p
                self._fprop(f"{s}.conv7", xin, 0, x_cs, cats[i + 1], 0, self.cat, B, H, W_, L.ACT_NONE)
                acts.append(a)
        self._kept = dict(tape=tape, out0=out0, t=t, cats=cats, acts=acts, shape=(B, H, W_))
        return cats

    # ---- loss
    def loss(self, uv, with_grad=True):
        """mmh_heatmap_mse on the kept stage outputs -> (loss float64 [6] on the device, the six gradient buffers [B,h,w,24]
        or None).  uv: float64 [B,21,2] in pixels of the input images."""
        k = self._kept
        B, h, w = k["shape"]
        if not torch.is_tensor(uv):
            uv = torch.from_numpy(np.asarray(uv, dtype=np.float64))
        uv = uv.to(self.device, torch.float64).reshape(B, JOINTS, 2).contiguous()
        nbytes = L.load().mmh_heatmap_mse_ws_bytes(N_OUT, B, h, w)
        if nbytes == 0:
            raise ValueError(f"heatmap_mse: shape B={B} h={h} w={w} refused")
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=self.device)
        out = torch.empty(N_OUT, dtype=torch.float64, device=self.device)
        heat = (C.c_void_p * N_OUT)(*[c.data_ptr() for c in k["cats"]])
        G = [ops._empty((B, h, w, JLANES), k["out0"]) for _ in range(N_OUT)] if with_grad else None
        dheat = (C.c_void_p * N_OUT)(*[g.data_ptr() for g in G]) if with_grad else None
        wts = (C.c_double * N_OUT)(*self.stage_weights)
        L.call("mmh_heatmap_mse", heat, N_OUT, B, h, w, self.cat, ops._ptr(uv), self.sigma, wts, ops._ptr(out), dheat, JLANES,
               ops._ptr(ws), nbytes, ops._stream())
        return out, G

    # ---- backward
    def _bwd(self, name, x, x_cs, g, y, H, W_, need_dx=True):
        """the backward of one convolution: g = the gradient on its (post-ReLU, if y is given) dense output; x its input, read
        from lane 0 with pixel stride x_cs.  Writes dw, db into the gradient buffer; -> dx [B,H,W,Cin'] or None"""
        B = g.shape[0]
        k, _, cin_p, cout_p = self.meta[name]["shape"]
        w, _ = self._views(self.p, name)
        dw, db = self._views(self.g, name)
        st = ops._stream()
        if y is not None:
            gy = torch.empty_like(g)
            L.call("mmh_act_bwd", ops._ptr(g), ops._ptr(y), ops._ptr(gy), g.numel(), L.ACT_RELU, st)
            g = gy
        rows = B * H * W_
        cw = ops._ws(L.load().mmh_colsum_ws_bytes(rows, cout_p), g)
        L.call("mmh_colsum", ops._ptr(g), rows, cout_p, cout_p, ops._ptr(db), ops._ptr(cw), cw.numel() * 4, 0, L.F32, st)
        d = ops.conv_desc(B, H, W_, cin_p, cout_p, k, 1, k // 2, False, x_cs=x_cs, y_cs=cout_p)
        ww = ops._ws(L.load().mmh_conv2d_wgrad_ws_bytes(C.byref(d)), g)
        L.call("mmh_conv2d_wgrad", C.byref(d), ops._ptr(x), ops._ptr(g), ops._ptr(dw), ops._ptr(ww), ww.numel() * 4, 0, 0, st)
        if not need_dx:
            return None
        dx = ops._empty((B, H, W_, cin_p), g)
        L.call("mmh_conv2d_dgrad", C.byref(d), ops._ptr(g), ops._ptr(w), ops._ptr(dx), cin_p, st)
        return dx

    @staticmethod
    def _lane_add(x, x_off, y, lanes):
        """y[..., :lanes] += x[..., x_off : x_off + lanes] for NHWC buffers of any widths"""
        pixels = x.numel() // x.shape[-1]
        L.call("mmh_lane_add", C.c_void_p(x.data_ptr() + 4 * x_off), x.shape[-1], ops._ptr(y), y.shape[-1], pixels, lanes,
               ops._stream())

    def backward(self, G):
        """G: the six gradient buffers of loss(); fills the gradient buffer (every element of it is written)"""
        k = self._kept
        B, h, w = k["shape"]
        c0p = self.cat - JLANES
        d_out0 = torch.zeros((B, h, w, c0p), dtype=torch.float32, device=self.device)
        for i in range(len(STAGES) - 1, -1, -1):
            s, a = STAGES[i], k["acts"][i]
            g = self._bwd(f"{s}.conv7", a[5], a[5].shape[3], G[i + 1], None, h, w)
            for c in range(5, 0, -1):                                           # conv6 .. conv2
                g = self._bwd(f"{s}.{REPEAT[c]}", a[c - 1], a[c - 1].shape[3], g, a[c], h, w)
            dcat = self._bwd(f"{s}.conv1", k["cats"][i], self.cat, g, a[0], h, w)
            self._lane_add(dcat, 0, G[i], JLANES)
            self._lane_add(dcat, JLANES, d_out0, c0p)
        g = self._bwd("conv6_2_CPM", k["t"], k["t"].shape[3], G[0], None, h, w)
        g = self._bwd("conv6_1_CPM", k["out0"], c0p, g, k["t"], h, w)
        self._lane_add(g, 0, d_out0, c0p)
        g = d_out0
        for n, x, y, H, W_ in reversed(k["tape"]):
            if n == "pool":
                dx = torch.empty_like(x)
                L.call("mmh_maxpool2x2_bwd", ops._ptr(x), ops._ptr(g), B, H, W_, x.shape[3], ops._ptr(dx), ops._stream())
                g = dx
            else:
                g = self._bwd(n, x, x.shape[3], g, y, H, W_, need_dx=n != "conv1_1")
        self._kept = None

    # ---- one training step
    def step(self, images, uv, layout="nchw", lr=None):
        """normalise -> forward -> loss -> backward -> Adam; -> the six losses, float64 [6] on the device"""
        x = ops.hpe_normalize(images, layout)
        self.forward(x)
        losses, G = self.loss(uv)
        self.backward(G)
        self.steps += 1
        ops.adam_step(self.p, self.g, self.m, self.v, self.lr if lr is None else lr, self.beta1, self.beta2, self.eps, self.steps)
        return losses

    def grads(self):
        """the gradient buffer as a state dict of the reference's shapes (host, fp32)"""
        flat, out = self.g.cpu(), OrderedDict()
        for name, m in self.meta.items():
            w, b = self._views(flat, name)
            out[name + ".weight"] = w[:, :, m["rows"], :m["cout"]].permute(3, 2, 0, 1).contiguous()
            out[name + ".bias"] = b[:m["cout"]].clone()
        return out

    def inference_net(self):
        """an hpe.Hpm2d on the current weights (a copy: later steps do not change it)"""
        return hpe.Hpm2d(self.device).load_state_dict(self.state_dict())
