"""Oracles of the 3D estimator's training (mmhand_amd/hpe_train.py: Hpm3dTrainer, csrc/hpe3d_train.hip), next to
tests/_hpe_oracle.py and tests/_hpe_train_oracle.py:

* `gauss_heatmaps`, `smooth_l1`, `linear_dgrad`, `linear_wgrad`: float64 numpy of the four kernels' definitions
  (include/mmhand_hip.h); the linear ones also return sum |terms| per element, for the bound of one fma chain;
* `outputs`, `loss`: the whole training graph as torch calls on a state dict in any dtype - the reference's forward
  (networks/net_hpm3d.py:66-115: the trunk, four Repeat blocks, `depth`, three nn.Linear; stage6 is not run) and
  nn.SmoothL1Loss() times a scale (hpm3d_model.py:73,105);
* `param_grads`, `adam_trace`: that graph's parameter gradients, and torch.optim.Adam steps on it in float64;
* `inputs`: the heat maps and depth targets of the fixture and of the whole-network tests."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import _hpe_oracle as O
from tests import _hpe_train_oracle as T

JOINTS, JLANES = 21, 24
STAGES = ("stage2", "stage3", "stage4", "stage5")
FC = ("depth_fc_1", "depth_fc_2", "depth_fc_3")


# ------------------------------------------------------------------------------------------------- the four kernels
def gauss_heatmaps(uv, H, W_, sigma):
    """fp32 [B,H,W,24]: tests/_hpe_train_oracle.target in lanes 0..20, zeros in 21..23"""
    t = T.target(uv, H, W_, sigma)
    out = np.zeros(t.shape[:3] + (JLANES,), dtype=np.float32)
    out[..., :JOINTS] = t
    return out


def smooth_l1(pred, target, n=JOINTS, beta=1.0, scale=1.0):
    """pred fp32 [M,ps >= n], target float64 [M,n] -> (loss float64, dpred float64 [M,24], not rounded).  Every operation in
    float64 and on its own; the terms are added in ascending (m, j) order (np.cumsum adds in order)."""
    p = np.asarray(pred)[:, :n].astype(np.float64)
    M = p.shape[0]
    d = p - np.asarray(target, dtype=np.float64).reshape(M, n)
    a = np.abs(d)
    quad = a < beta
    terms = np.where(quad, 0.5 * d * d / beta, a - 0.5 * beta)
    loss = scale * np.cumsum(terms.reshape(-1))[-1] / float(M * n)
    g = np.zeros((M, JLANES), dtype=np.float64)
    g[:, :n] = (scale / float(M * n)) * np.where(quad, d / beta, np.sign(d))
    return float(loss), g


def linear_dgrad(dy, wt):
    """dy [M,N], wt [K,N] -> (dx float64 [M,K] = dy @ wt.T, sum |terms| [M,K])"""
    dy, wt = np.asarray(dy, dtype=np.float64), np.asarray(wt, dtype=np.float64)
    return dy @ wt.T, np.abs(dy) @ np.abs(wt).T


def linear_wgrad(x, dy):
    """x [M,K], dy [M,N] -> (dwt float64 [K,N] = x.T @ dy, db [N] = dy.sum(0), sum |terms| of dwt, of db)"""
    x, dy = np.asarray(x, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    return x.T @ dy, dy.sum(0), np.abs(x).T @ np.abs(dy), np.abs(dy).sum(0)


def gamma(L):
    """the bound of one fp32 fma chain of length L: |computed - exact| <= gamma_L * sum |terms|"""
    u = L * 2.0 ** -24
    return u / (1.0 - u)


# ------------------------------------------------------------------------------------------------- the whole graph
def outputs(sd, x):
    """networks/net_hpm3d.py:66-115: x [B,21,H,W] -> depth_fc_3's output [B,21] as a tensor of sd's graph"""
    heat, out0 = O._front(sd, x, STAGES)
    d = O._repeat(sd, "depth", torch.cat((heat, out0), 1)).reshape(x.shape[0], -1)
    for n in FC:
        d = F.linear(d, sd[n + ".weight"], sd[n + ".bias"])
    return d


def loss(sd, x, z, beta=1.0, scale=10.0):
    """(hpm3d_model.py:105's loss as a tensor of sd's graph, the outputs)"""
    out = outputs(sd, x)
    return F.smooth_l1_loss(out, z.to(out.dtype), beta=beta) * scale, out


def param_grads(sd, x, z, beta=1.0, scale=10.0, dtype=torch.float64):
    """(loss float, outputs numpy [B,21], {key: gradient in `dtype`} for the keys that have one, the keys that have none)"""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    l, out = loss(p, x.to(dtype), z, beta, scale)
    l.backward()
    return (float(l.detach()), out.detach().numpy(), {k: v.grad.detach() for k, v in p.items() if v.grad is not None},
            [k for k, v in p.items() if v.grad is None])


def adam_trace(sd, x, z, steps=3, lr=2e-4, beta1=0.5, beta2=0.999, eps=1e-8, beta=1.0, scale=10.0):
    """`steps` torch.optim.Adam steps on the loss in float64 -> (losses [steps], the final parameters).  Every parameter is
    handed to the optimiser, stage6's too: torch's Adam skips parameters without a gradient."""
    p = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.Adam(list(p.values()), lr=lr, betas=(beta1, beta2), eps=eps)
    x = x.double()
    trace = []
    for _ in range(steps):
        opt.zero_grad()
        l, _ = loss(p, x, z, beta, scale)
        l.backward()
        opt.step()
        trace.append(float(l.detach()))
    return np.array(trace), {k: v.detach() for k, v in p.items()}


# ------------------------------------------------------------------------------------------------- test inputs
def inputs(seed=0):
    """(heat fp32 [2,32,32,21], z float64 [2,21]): the Gaussian maps of tests/_hpe_train_oracle.poses at sigma 5 and depth
    targets in +-0.8 with two far ones, so that both branches of the loss carry terms (the outputs of the generated weights lie
    in +-0.14)"""
    heat = T.target(T.poses(2, 32, 32, seed), 32, 32, 5.0)
    z = (O.hashed(8200, 2 * JOINTS, seed) * 0.8).reshape(2, JOINTS)
    z[0, 0], z[1, 1] = 1.5, -2.25
    return heat, z


def nchw(heat):
    return torch.from_numpy(np.ascontiguousarray(heat[..., :JOINTS])).permute(0, 3, 1, 2).contiguous()
