"""Measures the 2D estimator's training step (mmhand_amd/hpe_train.py, csrc/hpe_train.hip) on one MI355X and writes
profiles/hpe_train.txt:

* the step (normalise -> forward -> loss -> backward -> Adam) at B = 32, 256 x 256, full width: ms and images/s, and its split
  into forward, loss kernel and backward (each timed alone on the same buffers);
* mmh_heatmap_mse alone against the same loss written with torch ops on the same box - F.interpolate(scale_factor=8, bilinear,
  align_corners=True) of the six outputs, F.mse_loss against a device-resident target, autograd back to the six low-resolution
  maps - interleaved round by round.  The torch path is given its target for nothing (the fused kernel computes it); its
  peak memory above the inputs is recorded next to the fused kernel's.

The weights are generated (tests/_hpe_oracle.py): the rates do not depend on them, and no accuracy is reported.  These are
measurements; nothing here is a bar.

    python tools/bench_hpe_train.py [--batch 32] [--size 256] [--rounds 5] [--out profiles/hpe_train.txt]"""
import argparse
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, runs, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpe_train.txt"))
    a = p.parse_args()
    from mmhand_amd import hpe_train, ops
    from tests import _hpe_oracle as O
    from tests import _hpe_train_oracle as T
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    B, S = a.batch, a.size
    tr = hpe_train.Hpm2dTrainer(dev).load_state_dict(OrderedDict((k, v.float()) for k, v in O.state_dict("2d", O.FULL).items()))
    g = torch.Generator(device=dev).manual_seed(0)
    img = torch.rand((B, 3, S, S), generator=g, device=dev) * 2 - 1
    uv = torch.rand((B, 21, 2), generator=g, device=dev, dtype=torch.float64) * (S - 1)
    x = ops.hpe_normalize(img)

    # the torch form of the loss on the trainer's own stage outputs (NCHW copies of lanes 0..20) and a resident target
    cats = tr.forward(x)
    kept = tr._kept                                 # a step's backward releases what its forward kept: the loss runs on these
    maps = [c[..., :21].permute(0, 3, 1, 2).contiguous().requires_grad_(True) for c in cats]
    tgt = torch.from_numpy(T.target(uv.cpu().numpy(), S, S, tr.sigma)).permute(0, 3, 1, 2).contiguous().to(dev)

    def torch_loss():
        for m in maps:
            m.grad = None
        ls = [F.mse_loss(F.interpolate(m, scale_factor=8, mode="bilinear", align_corners=True), tgt) for m in maps]
        sum(ls).backward()
        return ls

    def fused_loss():
        tr._kept = kept
        return tr.loss(uv)

    # one check that both compute the same thing before anything is timed
    ref = torch.stack([l.detach().double() for l in torch_loss()])
    got, G = fused_loss()
    assert float((got / ref - 1).abs().max()) < 1e-5, (got, ref)
    assert float((G[5][..., :21].permute(0, 3, 1, 2) - maps[5].grad).abs().max()) <= 1e-4 * float(maps[5].grad.abs().max())
    del G

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fused_loss()
    torch.cuda.synchronize()
    fused_peak = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    torch_loss()
    torch.cuda.synchronize()
    torch_peak = torch.cuda.max_memory_allocated() - base

    fused_ms, torch_ms, step_ms = [], [], []
    for _ in range(a.rounds):                       # interleaved: one fused loss, one torch loss, one whole step, per round
        fused_ms += timed(fused_loss, 1)
        torch_ms += timed(torch_loss, 1)
        step_ms += timed(lambda: tr.step(img, uv), 1)

    def backward_only():
        tr.forward(x)
        torch.cuda.synchronize()
        _, G = tr.loss(uv)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.backward(G)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    fwd_ms = timed(lambda: tr.forward(x), a.rounds)
    loss_ms = timed(fused_loss, a.rounds)
    bwd_ms = [backward_only() for _ in range(a.rounds + 1)][1:]
    adam_ms = timed(lambda: ops.adam_step(tr.p, tr.g, tr.m, tr.v, 0.0, 0.9, 0.999, 1e-8, 1), a.rounds)
    med = lambda v: float(np.median(v))        # noqa: E731
    res = {"batch": B, "size": S, "rounds": a.rounds,
           "step_ms": round(med(step_ms), 2), "step_img_s": round(B / med(step_ms) * 1e3, 1),
           "forward_ms": round(med(fwd_ms), 2), "loss_kernel_ms": round(med(loss_ms), 3), "backward_ms": round(med(bwd_ms), 2),
           "adam_ms": round(med(adam_ms), 3),
           "heatmap_mse_ms": round(med(fused_ms), 3), "torch_loss_ms": round(med(torch_ms), 3),
           "heatmap_mse_over_torch": round(med(fused_ms) / med(torch_ms), 4),
           "heatmap_mse_peak_MB": round(fused_peak / 1e6, 1), "torch_loss_peak_MB": round(torch_peak / 1e6, 1),
           "parameters": int((~tr.padding_mask()).sum()),
           "weights": "generated (tests/_hpe_oracle.py)", "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("# tools/bench_hpe_train.py: one training step of the 2D estimator (generated weights) and its loss kernel next to the\n"
                 "# same loss in torch ops (device-resident target), interleaved; times in ms are medians of HIP-event pairs with the\n"
                 "# host enqueue included; *_peak_MB = device memory allocated above the inputs while the loss and its backward run\n"
                 + line + "\n")


if __name__ == "__main__":
    main()
