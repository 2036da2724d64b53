"""Oracles of the estimator's training (mmhand_amd/hpe_train.py, csrc/hpe_train.hip), next to tests/_hpe_oracle.py:

* `target`, `heatmap_mse`: float64 numpy of mmh_heatmap_mse's definition (include/mmhand_hip.h) - the x8 bilinear upsample of
  tests/_hpe_oracle.upsample rounded to fp32, the Gaussian target of data/RHD_dataset.py:245-277 (gaussian_kernel and the two
  cuts of gen_heatmap), the mean squared error and its gradient on the low-resolution maps, with sum |terms| per element;
* `losses`: the whole training loss as a torch graph in any dtype - the reference's forward (networks/net_hpm2d.py:71-119: six
  outputs, each through F.interpolate(scale_factor=8, bilinear, align_corners=True)) and nn.MSELoss against the target;
* `param_grads`, `adam_trace`: that graph's parameter gradients, and torch.optim.Adam steps on it in float64."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import _hpe_oracle as O

JOINTS = 21
STAGES = ("stage2", "stage3", "stage4", "stage5", "stage6")
CUT_LO, CUT_HI = 0.0099, 1.0


def dist2(uv, Ho, Wo):
    """float64 [B,Ho,Wo,21]: D2 = (gridx - x) ** 2 + (gridy - y) ** 2 (RHD_dataset.py:275-276)"""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, JOINTS, 2)
    gy, gx = np.mgrid[0:Ho, 0:Wo]
    gx, gy = gx.astype(np.float64)[None, :, :, None], gy.astype(np.float64)[None, :, :, None]
    x, y = uv[:, None, None, :, 0], uv[:, None, None, :, 1]
    return (gx - x) ** 2 + (gy - y) ** 2


def gaussian(uv, Ho, Wo, sigma):
    """float64 [B,Ho,Wo,21] before the cuts: exp(-D2 / 2.0 / sigma / sigma) (RHD_dataset.py:277)"""
    return np.exp(-dist2(uv, Ho, Wo) / 2.0 / sigma / sigma)


def target(uv, Ho, Wo, sigma):
    """fp32 [B,Ho,Wo,21]: values above 1 become 1, values below 0.0099 become 0 (RHD_dataset.py:250-251), then .astype(float32)
    (RHD_dataset.py:197)"""
    g = gaussian(uv, Ho, Wo, sigma)
    g[g > CUT_HI] = CUT_HI
    g[g < CUT_LO] = 0.0
    return g.astype(np.float32)


def cut_margin(uv, Ho, Wo, sigma):
    """(the smallest relative distance of any target pixel from either cut, the number of pixels a joint sits on exactly).
    A joint exactly on a pixel has D2 == 0 there and exp(-0.0) == 1.0 in every libm: the value IS the upper cut, which leaves
    it alone (1 > 1 is false).  Those pixels are counted apart and every other one enters the margin."""
    g = gaussian(uv, Ho, Wo, sigma)
    on = dist2(uv, Ho, Wo) == 0.0
    assert (g[on] == 1.0).all()
    off = g[~on]
    return float(min(np.abs(off / CUT_LO - 1.0).min(), np.abs(off / CUT_HI - 1.0).min())), int(on.sum())


def tap_matrix(n_src, n_out):
    """A [n_out, n_src]: the weight with which output o reads source i; both taps added where they are the same index"""
    i0, i1, wgt = O._taps(n_src, n_out)
    A = np.zeros((n_out, n_src), dtype=np.float64)
    o = np.arange(n_out)
    A[o, i0] += 1.0 - wgt
    A[o, i1] += wgt
    return A


def heatmap_mse(heats, uv, sigma, weights):
    """heats: S arrays fp32 [B,h,w,cs >= 21] -> (loss float64 [S], grad float64 [S,B,h,w,21] (not rounded), absterms the same
    shape = sum |terms| of every gradient element)"""
    B, h, w, _ = heats[0].shape
    Ho, Wo = 8 * h, 8 * w
    n = float(B * JOINTS * Ho * Wo)
    t = target(uv, Ho, Wo, sigma).astype(np.float64)
    Ay, Ax = tap_matrix(h, Ho), tap_matrix(w, Wo)
    loss, grad, absterms = [], [], []
    for hm, wt in zip(heats, weights):
        up = O.upsample(np.asarray(hm)[..., :JOINTS]).astype(np.float32)
        d = up.astype(np.float64) - t
        loss.append(np.sum(d * d) / n)
        coef = 2.0 * float(wt) / n
        grad.append(np.einsum("oy,px,bopj->byxj", Ay, Ax, coef * d, optimize=True))
        absterms.append(np.einsum("oy,px,bopj->byxj", Ay, Ax, np.abs(coef * d), optimize=True))
    return np.array(loss), np.stack(grad), np.stack(absterms)


def conv3x3_c4_f64(x, w, bias, relu=True):
    """mmh_conv3x3_c4_fprop_f64's definition: x fp32 [B,H,W,4], w fp32 [3,3,4,Cout], bias fp32 [Cout] -> fp32 [B,H,W,Cout]; the
    products (exact in float64) added to the bias in ascending (kh, kw, c) order, one rounding, then ReLU"""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    B, H, W_, _ = x.shape
    xp = np.zeros((B, H + 2, W_ + 2, 4))
    xp[:, 1:-1, 1:-1] = x
    acc = np.broadcast_to(np.asarray(bias, dtype=np.float64), (B, H, W_, w.shape[3])).copy()
    for kh in range(3):
        for kw in range(3):
            for c in range(4):
                acc = acc + xp[:, kh:kh + H, kw:kw + W_, c, None] * w[kh, kw, c]
    y = acc.astype(np.float32)
    return np.maximum(y, np.float32(0)) if relu else y


# ------------------------------------------------------------------------------------------------- the whole graph
def stage_outputs(sd, x):
    """networks/net_hpm2d.py:71-117: the six low-resolution outputs [B,21,H/8,W/8]"""
    for n in O.TRUNK:
        x = O._conv(sd, n, x)
        if n in O.POOL_AFTER:
            x = F.max_pool2d(x, 2)
    out0 = x
    outs = [O._conv(sd, "conv6_2_CPM", O._conv(sd, "conv6_1_CPM", out0), relu=False)]
    for s in STAGES:
        outs.append(O._repeat(sd, s, torch.cat((outs[-1], out0), 1)))
    return outs


def losses(sd, x, uv, sigma=5.0, tgt=None):
    """the six MSE losses as tensors of sd's graph; x [B,3,H,W] in the dtype of sd; tgt: a stored target [B,21,H,W]"""
    if tgt is None:
        tgt = torch.from_numpy(target(uv, x.shape[2], x.shape[3], sigma)).permute(0, 3, 1, 2)
    tgt = tgt.to(x.dtype)
    ups = [F.interpolate(o, scale_factor=8, mode="bilinear", align_corners=True) for o in stage_outputs(sd, x)]
    return [F.mse_loss(u, tgt) for u in ups]


def param_grads(sd, x, uv, sigma=5.0, weights=None, dtype=torch.float64, tgt=None):
    """(losses [6] float64 numpy, {key: gradient of sum_s weights[s] * loss_s in `dtype`})"""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    ls = losses(p, x.to(dtype), uv, sigma, tgt)
    wts = [1.0] * len(ls) if weights is None else weights
    sum(w * l for w, l in zip(wts, ls)).backward()
    return np.array([float(l.detach()) for l in ls]), {k: v.grad.detach() for k, v in p.items()}


def adam_trace(sd, x, uv, steps=3, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, sigma=5.0):
    """`steps` torch.optim.Adam steps on the sum of the six losses in float64 -> (losses [steps, 6], the final parameters)"""
    p = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.Adam(list(p.values()), lr=lr, betas=(beta1, beta2), eps=eps)
    x = x.double()
    trace = []
    for _ in range(steps):
        opt.zero_grad()
        ls = losses(p, x, uv, sigma)
        sum(ls).backward()
        opt.step()
        trace.append([float(l.detach()) for l in ls])
    return np.array(trace), {k: v.detach() for k, v in p.items()}


# ------------------------------------------------------------------------------------------------- test poses
def poses(B, Ho, Wo, seed=0):
    """uv float64 [B,21,2] on an Ho x Wo grid covering: fractional coordinates inside the image, on the border, exactly on a
    pixel, outside the image (an all-zero map far outside, a clipped one just outside) and two joints at one point.  Fractions
    are multiples of 1/8 plus 1/16, so that no squared distance lands on a cut (tests/test_hpe_train_cpu.py asserts it)."""
    r = O.hashed(8100, B * JOINTS * 2, seed).reshape(B, JOINTS, 2)
    frac = np.floor((r + 1.0) * 4.0 * np.array([Wo, Ho])) / 8.0 + 0.0625       # [0, Wo) x [0, Ho) in eighths, off the grid
    uv = np.where(frac > np.array([Wo - 1.0, Ho - 1.0]), frac - 1.0, frac)      # within the pixel centres' span
    uv[:, 0] = [0.0, Ho - 1.0]                      # on the border, exactly on a pixel: the value 1 at one output
    uv[:, 1] = [Wo - 1.0, 0.0]
    uv[:, 2] = [Wo // 2, Ho // 2]                   # exactly on a pixel
    uv[:, 3] = [-1000.0, -1000.0]                   # far outside: an all-zero target
    uv[:, 4] = [Wo + 3.3125, Ho // 3 + 0.5625]      # just outside: a clipped bump
    uv[:, 5] = [-2.4375, -1.6875]
    uv[:, 7] = uv[:, 6]                             # two joints at one point
    return uv
