"""Training the two hand-pose machines (networks/net_hpm2d.py, networks/net_hpm3d.py) on the device: where the weights of
`evaluate --pck` come from.

The reference trains them under hand_pose_estimators/CVPR2020_hpm3d/models/ (hpm2d_model.py, hpm3d_model.py, hpm_model.py):
Hpm2d on (image, 21 Gaussian heat maps at full resolution, sigma 5: data/RHD_dataset.py:139-147,192-200,245-277) with the sum
over the six stage outputs of nn.MSELoss() times 1000 (hpm2d_model.py:143-151), Hpm3d on (those heat maps, the labels' depth)
with nn.SmoothL1Loss() times 10 (hpm3d_model.py:73,91-113), both with Adam(lr 2e-4, betas 0.5 / 0.999) and the linear decay.
`Hpm2dTrainer` has that loss with stage_weights[s] in place of the 1000 and defaults of this port's (weights 1, lr 1e-4,
betas 0.9 / 0.999); `Hpm3dTrainer`'s recipe and defaults are the reference's.

Both keep the padded layout of the inference networks (hpe.relay_conv, hpe.relay_fc1, hpe.relay_fc) as fp32 masters in one flat
buffer, with the gradients and Adam's two moments in three more of the same layout, so that one mmh_adam_step updates every
parameter.
forward: the calls of the inference networks (mmh_conv2d_fprop with fused ReLU, mmh_maxpool2x2_fwd, mmh_linear_fprop, under
hpe.direct_two_level()), keeping what the backward reads.  Hpm2dTrainer's conv1_1 runs on mmh_conv3x3_c4_fprop_f64 (float64
accumulation, one rounding): its ReLU masks are then those of exact arithmetic, and its gradients, summed over 27 inputs only,
do not hang on a mask that fp32 rounding flips.  Inference overwrites the heat lanes of ONE cat buffer; here every
stage's input cat buffer [B,h,w,24 + C0'] is kept (out_0 is computed densely once and copied into lanes 24.. of each).
backward: an explicit schedule, no autograd -
  Hpm2dTrainer
  mmh_heatmap_mse              the six losses and their gradients on the low-resolution maps, G_1 .. G_6 [B,h,w,24]
  stage6 .. stage2             conv7 .. conv1: mmh_act_bwd (ReLU), mmh_colsum (bias), mmh_conv2d_wgrad, mmh_conv2d_dgrad (fp32,
                               zero padding); conv1's input gradient [B,h,w,24 + C0'] is split by mmh_lane_add: lanes 0..23 onto
                               the previous output's G, lanes 24.. onto d_out0
  conv6_2_CPM, conv6_1_CPM     from G_1; conv6_1_CPM's input gradient is the sixth addend of d_out0
  conv5_3_CPM .. conv1_1       the trunk with mmh_maxpool2x2_bwd; conv1_1 needs no input gradient
  Hpm3dTrainer
  mmh_smooth_l1                the loss and its gradient on depth_fc_3's output [B,24]
  depth_fc_3 .. depth_fc_1     mmh_linear_wgrad, mmh_linear_dgrad (no activation lies between them: net_hpm3d.py:112-114);
                               depth_fc_1's input gradient is the gradient on the depth stage's conv7 output
  depth, stage5 .. stage2      as above; only the last block is supervised, so G of an earlier output is lanes 0..23 of the
                               next conv1's input gradient alone.  mmh_conv2d_dgrad runs with two-level summation here
                               (dgrad_two_level below)
  the CPM head and the trunk   as above
Padding rows, columns and lanes stay exactly zero: their inputs, weights or output gradients are zero, so their gradients are
exact zeros and Adam moves a zero parameter with zero moments by zero."""
import contextlib
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
FULL_WIDTHS = dict(c1=64, c2=128, c3=256, c4=512, c0=128, cpm=512, rep=128, fc=512)
FC = ("depth_fc_1", "depth_fc_2", "depth_fc_3")


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
        out += _repeat_shapes(s, w)
    return out


def _repeat_shapes(s, w):
    out = [(f"{s}.conv1", (w["rep"], w["c0"] + JOINTS, 7, 7))]
    out += [(f"{s}.conv{i}", (w["rep"], w["rep"], 7, 7)) for i in (2, 3, 4, 5)]
    return out + [(f"{s}.conv6", (w["rep"], w["rep"], 1, 1)), (f"{s}.conv7", (JOINTS, w["rep"], 1, 1))]


def layer_shapes_3d(widths=FULL_WIDTHS, head_hw=32):
    """[(name, weight shape)] of networks/net_hpm3d.py:29-64 (Hpm3d(21, 21)) in the order of its state dict: the 2D machine's
    layers on 21 input channels, the `depth` block and the three Linear layers, depth_fc_1 for head_hw x head_hw maps"""
    fc = widths.get("fc", FULL_WIDTHS["fc"])
    return (layer_shapes(widths, JOINTS) + _repeat_shapes("depth", widths) +
            [(FC[0], (fc, JOINTS * head_hw * head_hw)), (FC[1], (fc, fc)), (FC[2], (JOINTS, fc))])


def _init(shapes, seed):
    sd = OrderedDict()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(seed))
        for name, shape in shapes:
            mod = (torch.nn.Linear(shape[1], shape[0]) if len(shape) == 2 else
                   torch.nn.Conv2d(shape[1], shape[0], kernel_size=shape[2], padding=shape[2] // 2))
            sd[name + ".weight"], sd[name + ".bias"] = mod.weight.detach().clone(), mod.bias.detach().clone()
    return sd


def init_state_dict(seed, widths=FULL_WIDTHS, in_nc=3):
    """torch's default nn.Conv2d initialisation: the modules themselves, constructed on the host in the state dict's order
    under torch.manual_seed(seed); the caller's random state is put back"""
    return _init(layer_shapes(widths, in_nc), seed)


def init_state_dict_3d(seed, widths=FULL_WIDTHS, head_hw=32):
    """the same for Hpm3d(21, 21): torch's default nn.Conv2d / nn.Linear initialisation in the state dict's order"""
    return _init(layer_shapes_3d(widths, head_hw), seed)


def linear_lr(lr, epoch, niter, niter_decay, epoch_count=1):
    """networks/networks.py:54-58: lr * (1 - max(0, epoch + epoch_count - niter) / (niter_decay + 1)), epoch counted from 0"""
    return lr * (1.0 - max(0, epoch + epoch_count - niter) / float(niter_decay + 1))


class _PoseTrainer:
    """what the two trainers share: the flat padded buffers and their views, and the forward / backward of the layers both
    networks have (the trunk, the CPM head, a Repeat block on a cat buffer)"""

    def __init__(self, device, lr, beta1, beta2, eps, sigma):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.lr, self.beta1, self.beta2, self.eps, self.sigma = float(lr), float(beta1), float(beta2), float(eps), float(sigma)
        self.steps = 0
        self.p = None

    # ---- checkpoint <-> the flat padded buffers
    def _fill(self, sd, probe, pairs):
        """pairs: [(name, (w, b), extra meta)] in the padded layout -> self.meta and the four flat buffers"""
        self.in_nc, self.c0, self.cat = probe.in_nc, probe.c0, probe.cat
        self.meta, off = OrderedDict(), 0
        for name, (w, b), extra in pairs:
            wt = sd[name + ".weight"]
            self.meta[name] = dict(shape=tuple(w.shape), cout=int(wt.shape[0]), cin=int(wt.shape[1]), w_off=off,
                                   b_off=off + w.numel(), **extra)
            off += w.numel() + b.numel()
        flat = torch.zeros(off, dtype=torch.float32)
        for name, (w, b), _ in pairs:
            m = self.meta[name]
            flat[m["w_off"]:m["b_off"]] = w.reshape(-1)
            flat[m["b_off"]:m["b_off"] + b.numel()] = b
        self.p = flat.to(self.device)
        self.g, self.m, self.v = (torch.zeros_like(self.p) for _ in range(3))
        self.steps = 0

    def _conv_pairs(self, probe, sd):
        out = []
        for name, (w, b) in probe.convs.items():
            rows = list(range(int(sd[name + ".weight"].shape[1])))
            if name.endswith(".conv1") and "." in name:
                rows = list(range(JOINTS)) + [JLANES + i for i in range(probe.c0)]
            out.append((name, (w, b), dict(rows=torch.tensor(rows))))
        return out

    def _views(self, flat, name):
        m = self.meta[name]
        return flat[m["w_off"]:m["b_off"]].view(*m["shape"]), flat[m["b_off"]:m["b_off"] + m["shape"][-1]]

    @staticmethod
    def _owned(w, m):
        """the view of a padded Linear weight [K',N'] that holds the reference tensor's elements"""
        if "hs" in m:                                           # depth_fc_1: rows over (y, x, c'), hpe.relay_fc1
            return w.view(m["hs"], m["hs"], JLANES, -1)[:, :, :JOINTS, :m["cout"]]
        return w[:m["cin"], :m["cout"]]                         # hpe.relay_fc

    def _reference(self, flat):
        """a flat buffer as a dict of the reference's names and shapes (host, fp32)"""
        flat, out = flat.cpu(), OrderedDict()
        for name, m in self.meta.items():
            w, b = self._views(flat, name)
            if "rows" in m:                                     # a convolution: RSCK, the reference's input channels at `rows`
                ref = w[:, :, m["rows"], :m["cout"]].permute(3, 2, 0, 1)
            elif "hs" in m:
                ref = self._owned(w, m).permute(3, 2, 0, 1).reshape(m["cout"], -1)
            else:
                ref = self._owned(w, m).t()
            out[name + ".weight"] = ref.contiguous()
            out[name + ".bias"] = b[:m["cout"]].clone()
        return out

    def padding_mask(self):
        """bool, the flat buffers' layout: True where an element is padding (no element of the reference's tensors)"""
        mask = torch.ones(self.p.numel(), dtype=torch.bool)
        for name, m in self.meta.items():
            w, b = self._views(mask, name)
            if "rows" in m:
                w[:, :, m["rows"], :m["cout"]] = False
            else:
                self._owned(w, m)[...] = False
            b[:m["cout"]] = False
        return mask

    def grads(self):
        """the gradient buffer as a state dict of the reference's shapes (host, fp32)"""
        return self._reference(self.g)

    # ---- forward
    def _fprop(self, name, x, x_off, x_cs, y, y_off, y_cs, B, H, W_, act):
        w, b = self._views(self.p, name)
        hpe._conv(x, x_off, x_cs, w, b, y, y_off, y_cs, B, H, W_, act)

    def _first(self, x, y, B, H, W_, cout_p):
        self._fprop("conv1_1", x, 0, x.shape[3], y, 0, cout_p, B, H, W_, L.ACT_RELU)

    def _front(self, x):
        """the trunk and the CPM head; -> (tape, out0, t, x_last, (B, h, w)); the caller runs conv6_2_CPM into its cat buffer"""
        assert self.p is not None, "load_state_dict first"
        ops._chk(x, "x")
        B, H, W_, cx = x.shape
        assert H % 8 == 0 and W_ % 8 == 0 and cx == ops.pad4(self.in_nc), (tuple(x.shape), self.in_nc)
        tape = []                                               # (name | "pool", input, output, H, W) of the trunk
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
                    self._first(x, y, B, H, W_, cout_p)
                else:
                    self._fprop(n, x, 0, x.shape[3], y, 0, cout_p, B, H, W_, L.ACT_RELU)
                tape.append((n, x, y, H, W_))
            x = y
        out0 = ops._empty((B, H, W_, self.cat - JLANES), x)
        self._fprop("conv5_3_CPM", x, 0, x.shape[3], out0, 0, out0.shape[3], B, H, W_, L.ACT_RELU)
        tape.append(("conv5_3_CPM", x, out0, H, W_))
        t = ops._empty((B, H, W_, self.meta["conv6_1_CPM"]["shape"][3]), x)
        self._fprop("conv6_1_CPM", out0, 0, out0.shape[3], t, 0, t.shape[3], B, H, W_, L.ACT_RELU)
        return tape, out0, t, (B, H, W_)

    def _stage(self, s, cat, out0, out, out_cs, shape):
        """one Repeat block: out_0 copied into lanes 24.. of its input cat buffer (the reference's cat((out_i, out_0), 1)), conv1 ..
        conv6 kept, conv7 into lanes 0..23 of `out`; -> the six activations"""
        B, H, W_ = shape
        cat[..., JLANES:].copy_(out0)
        a, xin, x_cs = [], cat, self.cat
        for c in REPEAT[:-1]:
            cout_p = self.meta[f"{s}.{c}"]["shape"][3]
            y = ops._empty((B, H, W_, cout_p), cat)
            self._fprop(f"{s}.{c}", xin, 0, x_cs, y, 0, cout_p, B, H, W_, L.ACT_RELU)
            a.append(y)
            xin, x_cs = y, cout_p
        self._fprop(f"{s}.conv7", xin, 0, x_cs, out, 0, out_cs, B, H, W_, L.ACT_NONE)
        return a

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

    def _stage_bwd(self, s, a, cat, g, g_prev, d_out0, h, w):
        """one Repeat block from g, the gradient on its conv7 output: conv1's input gradient is added onto g_prev (lanes 0..23)
        and d_out0 (lanes 24..)"""
        g = self._bwd(f"{s}.conv7", a[5], a[5].shape[3], g, None, h, w)
        for c in range(5, 0, -1):                                               # conv6 .. conv2
            g = self._bwd(f"{s}.{REPEAT[c]}", a[c - 1], a[c - 1].shape[3], g, a[c], h, w)
        dcat = self._bwd(f"{s}.conv1", cat, self.cat, g, a[0], h, w)
        self._lane_add(dcat, 0, g_prev, JLANES)
        self._lane_add(dcat, JLANES, d_out0, self.cat - JLANES)

    def _front_bwd(self, g0, d_out0):
        """the CPM head from g0, the gradient on conv6_2_CPM's output, then the trunk from the completed d_out0"""
        k = self._kept
        B, h, w = k["shape"]
        c0p = self.cat - JLANES
        g = self._bwd("conv6_2_CPM", k["t"], k["t"].shape[3], g0, None, h, w)
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

    def _adam(self, lr):
        self.steps += 1
        ops.adam_step(self.p, self.g, self.m, self.v, self.lr if lr is None else lr, self.beta1, self.beta2, self.eps, self.steps)


class Hpm2dTrainer(_PoseTrainer):
    def __init__(self, device=None, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, sigma=5.0, stage_weights=None):
        super().__init__(device, lr, beta1, beta2, eps, sigma)
        self.stage_weights = [1.0] * N_OUT if stage_weights is None else [float(v) for v in stage_weights]
        if len(self.stage_weights) != N_OUT:
            raise ValueError(f"stage_weights: {N_OUT} values expected, got {len(self.stage_weights)}")

    def load_state_dict(self, sd):
        """the reference's keys (a leading 'module.' is stripped) -> masters; Adam's moments and the step count start at zero"""
        sd = hpe.strip_module(sd)
        probe = hpe.Hpm2d("cpu").load_state_dict(sd)            # its checks and its re-layout: the one definition of both
        if probe.in_nc != 3 or probe.convs["conv1_1"][0].shape[3] > 256:
            raise ValueError(f"Hpm2dTrainer: conv1_1 reads {probe.in_nc} channels and writes {sd['conv1_1.weight'].shape[0]}: the "
                             "training forward's first layer (mmh_conv3x3_c4_fprop_f64) takes 3 and at most 256")
        self._fill(sd, probe, self._conv_pairs(probe, sd))
        return self

    def state_dict(self):
        """the reference's keys and shapes (networks/net_hpm2d.py) on the host, fp32: what hpe.Hpm2d.load_state_dict and the
        reference module (strict=True) load"""
        assert self.p is not None, "load_state_dict first"
        return self._reference(self.p)

    def _first(self, x, y, B, H, W_, cout_p):
        # float64 accumulation: this layer's ReLU masks decide gradients that are summed over 27 inputs only
        w, b = self._views(self.p, "conv1_1")
        L.call("mmh_conv3x3_c4_fprop_f64", ops._ptr(x), ops._ptr(w), ops._ptr(b), ops._ptr(y), B, H, W_, cout_p, cout_p, L.ACT_RELU,
               ops._stream())

    def forward(self, x):
        """x: fp32 [B,H,W,pad4(in_nc)] (ops.hpe_normalize's output) -> the six cat-width buffers whose lanes 0..20 are the stage
        outputs out_1 .. out_6 (lanes 21..23 zero).  Keeps the activations for backward()."""
        with hpe.direct_two_level():
            tape, out0, t, shape = self._front(x)
            B, H, W_ = shape
            cats = [torch.zeros((B, H, W_, self.cat), dtype=torch.float32, device=x.device) for _ in range(N_OUT)]
            self._fprop("conv6_2_CPM", t, 0, t.shape[3], cats[0], 0, self.cat, B, H, W_, L.ACT_NONE)
            acts = [self._stage(s, cats[i], out0, cats[i + 1], self.cat, shape) for i, s in enumerate(STAGES)]
        self._kept = dict(tape=tape, out0=out0, t=t, cats=cats, acts=acts, shape=shape)
        return cats

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

    def backward(self, G):
        """G: the six gradient buffers of loss(); fills the gradient buffer (every element of it is written)"""
        k = self._kept
        B, h, w = k["shape"]
        d_out0 = torch.zeros((B, h, w, self.cat - JLANES), dtype=torch.float32, device=self.device)
        for i in range(len(STAGES) - 1, -1, -1):
            self._stage_bwd(STAGES[i], k["acts"][i], k["cats"][i], G[i + 1], G[i], d_out0, h, w)
        self._front_bwd(G[0], d_out0)
        self._kept = None

    def step(self, images, uv, layout="nchw", lr=None):
        """normalise -> forward -> loss -> backward -> Adam; -> the six losses, float64 [6] on the device"""
        return self.step_normalized(ops.hpe_normalize(images, layout), uv, lr=lr)

    def step_normalized(self, x, uv, lr=None):
        """step() from the network's input on: x fp32 [B,H,W,4] as ops.hpe_normalize or ops.hpe_augment_normalize leave it, uv
        the joints in pixels of THAT input (after any warp)"""
        self.forward(x)
        losses, G = self.loss(uv)
        self.backward(G)
        self._adam(lr)
        return losses

    def inference_net(self):
        """an hpe.Hpm2d on the current weights (a copy: later steps do not change it)"""
        return hpe.Hpm2d(self.device).load_state_dict(self.state_dict())


@contextlib.contextmanager
def dgrad_two_level():
    """dgrad_levels = 2 for the duration of the block: the convolutions' input gradients with two-level summation.  Only the
    last of Hpm3d's blocks is supervised, so a gradient passes through up to 50 convolutions' dgrad in a row and the rounding of
    a one-level sum over 7 x 7 x 128 terms adds up along the way; Hpm2d's six supervised outputs feed fresh
    gradients in at every block and its trainer stays on the default.  The option is a global of the library, as conv_levels."""
    old = L.get_option("dgrad_levels")
    L.call("mmh_set_option", b"dgrad_levels", 2)
    try:
        yield
    finally:
        L.call("mmh_set_option", b"dgrad_levels", old)


class Hpm3dTrainer(_PoseTrainer):
    """the reference's recipe for Hpm3d(21, 21) (hpm3d_model.py:73,91-113; Adam: models/networks/__init__.py:72; defaults:
    options/train_options.py:31-37): input the 21 ground-truth Gaussian maps, target the labels' depth, loss
    nn.SmoothL1Loss() * 10.  stage6.* is in the checkpoint and not run, in the reference as here: its tensors are kept aside and
    come back from state_dict() bit for bit (torch's Adam skips parameters without a gradient)."""

    STAGES = hpe.Hpm3d.STAGES                                   # stage2 .. stage5, depth

    def __init__(self, device=None, lr=2e-4, beta1=0.5, beta2=0.999, eps=1e-8, sigma=5.0, beta=1.0, scale=10.0):
        super().__init__(device, lr, beta1, beta2, eps, sigma)
        self.beta, self.scale = float(beta), float(scale)
        if not (self.beta > 0 and np.isfinite(self.beta) and np.isfinite(self.scale)):
            raise ValueError(f"Hpm3dTrainer: beta {beta} must be positive and scale {scale} finite")

    def load_state_dict(self, sd):
        """the reference's keys (a leading 'module.' is stripped) -> masters; Adam's moments and the step count start at zero"""
        sd = hpe.strip_module(sd)
        probe = hpe.Hpm3d("cpu").load_state_dict(sd)            # its checks and its re-layout: the one definition of both
        self.head_hw = probe.head_hw
        pairs = self._conv_pairs(probe, sd)
        pairs.append((FC[0], probe.fc[0], dict(hs=probe.head_hw)))
        pairs += [(n, probe.fc[i], {}) for i, n in ((1, FC[1]), (2, FC[2]))]
        self._fill(sd, probe, pairs)
        self._aside = OrderedDict((f"stage6.{c}.{p}", sd[f"stage6.{c}.{p}"].detach().to(torch.float32).cpu().clone())
                                  for c in REPEAT for p in ("weight", "bias"))
        return self

    def state_dict(self):
        """the reference's keys, order and shapes (networks/net_hpm3d.py) on the host, fp32: what hpe.Hpm3d.load_state_dict and
        the reference module (strict=True) load; stage6.* as it came in"""
        assert self.p is not None, "load_state_dict first"
        ref, out = self._reference(self.p), OrderedDict()
        for key in ref:
            if key == "depth.conv1.weight":                     # the reference declares stage6 before depth
                out.update((k, v.clone()) for k, v in self._aside.items())
            out[key] = ref[key]
        return out

    def forward(self, x):
        """x: fp32 [B,H,W,24] (ops.gauss_heatmaps' or ops.heatmap_upsample_argmax's output) -> depth_fc_3's output [B,24] (lanes
        21..23 zero).  Keeps the five cat buffers, the depth stage's dense output and the Linear outputs for backward()."""
        if x.shape[0] > 64:
            raise ValueError(f"Hpm3dTrainer: a batch of {x.shape[0]}: the Linear kernels take 64 rows")
        if (x.shape[1], x.shape[2]) != (self.head_hw * 8, self.head_hw * 8):
            raise ValueError(f"Hpm3dTrainer: depth_fc_1 is sized for {self.head_hw * 8}^2 inputs, got {x.shape[1]} x {x.shape[2]}")
        S = self.STAGES
        with hpe.direct_two_level():
            tape, out0, t, shape = self._front(x)
            B, H, W_ = shape
            cats = [torch.zeros((B, H, W_, self.cat), dtype=torch.float32, device=x.device) for _ in S]
            self._fprop("conv6_2_CPM", t, 0, t.shape[3], cats[0], 0, self.cat, B, H, W_, L.ACT_NONE)
            acts = [self._stage(s, cats[i], out0, cats[i + 1], self.cat, shape) for i, s in enumerate(S[:-1])]
            d = ops._empty((B, H, W_, JLANES), x)
            acts.append(self._stage(S[-1], cats[-1], out0, d, JLANES, shape))
        z = [d.view(B, H * W_ * JLANES)]
        for n in FC:
            wt, b = self._views(self.p, n)
            z.append(ops.linear(z[-1], wt, b))
        self._kept = dict(tape=tape, out0=out0, t=t, cats=cats, acts=acts, d=d, z=z, shape=shape)
        return z[-1]

    def loss(self, depth, with_grad=True):
        """mmh_smooth_l1 on lanes 0..20 of depth_fc_3's kept output -> (loss float64 [1] on the device, its gradient [B,24] or
        None).  depth: [B,21] in the units the network is to predict (image heights: hpe_estimator.py:135)."""
        return ops.smooth_l1(self._kept["z"][-1], depth, JOINTS, self.beta, self.scale, with_grad)

    def backward(self, g):
        """g: the gradient of loss(); fills the gradient buffer (every element of it is written)"""
        k = self._kept
        B, h, w = k["shape"]
        for i in (2, 1, 0):
            wt, _ = self._views(self.p, FC[i])
            dwt, db = self._views(self.g, FC[i])
            ops.linear_wgrad(k["z"][i], g, dwt, db)
            g = ops.linear_dgrad(g, wt)
        g = g.view(B, h, w, JLANES)                             # the gradient on the depth stage's conv7 output
        d_out0 = torch.zeros((B, h, w, self.cat - JLANES), dtype=torch.float32, device=self.device)
        with dgrad_two_level():
            for i in range(len(self.STAGES) - 1, -1, -1):
                g_prev = torch.zeros((B, h, w, JLANES), dtype=torch.float32, device=self.device)
                self._stage_bwd(self.STAGES[i], k["acts"][i], k["cats"][i], g, g_prev, d_out0, h, w)
                g = g_prev
            self._front_bwd(g, d_out0)
        self._kept = None

    def heatmaps(self, uv):
        """the network's training input from the labels: ops.gauss_heatmaps at the size depth_fc_1 is sized for"""
        return ops.gauss_heatmaps(uv, self.head_hw * 8, self.head_hw * 8, self.sigma, device=self.device)

    def step(self, heat_or_uv, depth, lr=None):
        """heat_or_uv: the input itself, fp32 [B,H,W,24] on the device, or uv [B,21,2] from which mmh_gauss_heatmaps renders it;
        forward -> loss -> backward -> Adam; -> the loss, float64 [1] on the device"""
        x = heat_or_uv
        if not (torch.is_tensor(x) and x.dim() == 4):
            x = self.heatmaps(x)
        self.forward(x)
        loss, g = self.loss(depth)
        self.backward(g)
        self._adam(lr)
        return loss

    def inference_net(self):
        """an hpe.Hpm3d on the current weights (a copy: later steps do not change it)"""
        return hpe.Hpm3d(self.device).load_state_dict(self.state_dict())
