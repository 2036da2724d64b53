"""Measures the 3D estimator's training step (mmhand_amd/hpe_train.py: Hpm3dTrainer, csrc/hpe3d_train.hip) on one MI355X and
writes profiles/hpe3d_train.txt:

* the step (render the input -> forward -> loss -> backward -> Adam) at B = 32, 256 x 256, full width: ms and images/s, and its
  split into those five parts (each timed alone on the same buffers);
* mmh_gauss_heatmaps next to (a) the float64 numpy target on the host plus its upload - what a loader without the kernel does -
  and (b) the same maps written with torch device ops (float64 distances, exp, the two cuts, a cast and a copy into the 24-lane
  buffer), interleaved round by round;
* mmh_linear_wgrad + mmh_linear_dgrad at depth_fc_1's shape (M = B, K = 32 * 32 * 24, N = 512) next to the two torch.matmul
  calls that compute the same products on the device.

The weights are generated (tests/_hpe_oracle.py): the rates do not depend on them, and no accuracy is reported.  These are
measurements beside one another; nothing here is a bar.  Not measured: a loader's image reads (--heat_source predicted), more
than one GPU, the graph-captured form of the step (there is none).

    python tools/bench_hpe3d_train.py [--batch 32] [--size 256] [--rounds 5] [--out profiles/hpe3d_train.txt]"""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

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
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpe3d_train.txt"))
    a = p.parse_args()
    from mmhand_amd import hpe_train, ops
    from tests import _hpe_oracle as O
    from tests import _hpe_train_oracle as T
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    B, S = a.batch, a.size
    sd = OrderedDict((k, v.float()) for k, v in O.state_dict("3d", O.FULL, head_hw=S // 8).items())
    tr = hpe_train.Hpm3dTrainer(dev).load_state_dict(sd)
    g = torch.Generator(device=dev).manual_seed(0)
    uv = torch.rand((B, 21, 2), generator=g, device=dev, dtype=torch.float64) * (S - 1)
    z = torch.rand((B, 21), generator=g, device=dev, dtype=torch.float64) * 2 - 1
    uv_host = uv.cpu().numpy()
    x = tr.heatmaps(uv)

    # ---- the input render: the kernel, the host's numpy target + upload, torch device ops
    def host_render():
        t = T.target(uv_host, S, S, tr.sigma)
        buf = np.zeros((B, S, S, 24), dtype=np.float32)
        buf[..., :21] = t
        return torch.from_numpy(buf).to(dev)

    gy, gx = torch.meshgrid(torch.arange(S, device=dev, dtype=torch.float64), torch.arange(S, device=dev, dtype=torch.float64),
                            indexing="ij")

    def torch_render():
        d2 = (gx[None, :, :, None] - uv[:, None, None, :, 0]) ** 2 + (gy[None, :, :, None] - uv[:, None, None, :, 1]) ** 2
        v = torch.exp(-d2 / 2.0 / tr.sigma / tr.sigma).clamp_(max=1.0)
        v[v < 0.0099] = 0.0
        out = torch.zeros((B, S, S, 24), dtype=torch.float32, device=dev)
        out[..., :21] = v.float()
        return out

    # one check that all three render the same maps before anything is timed (random joints may put a pixel on a cut, where one
    # unit in the last place of exp decides between 0.0099 and 0: a handful of such pixels is not a difference of the methods)
    for other in (host_render(), torch_render()):
        assert float(((other - x).abs() > 2.0 ** -23).float().mean()) < 1e-6 and not other[..., 21:].any()
    render_ms, torch_render_ms, host_render_ms = [], [], []
    for _ in range(a.rounds):
        render_ms += timed(lambda: tr.heatmaps(uv), 1)
        torch_render_ms += timed(torch_render, 1)
        t0 = time.perf_counter()
        host_render()
        torch.cuda.synchronize()
        host_render_ms.append((time.perf_counter() - t0) * 1e3)

    # ---- the Linear backward at depth_fc_1's shape next to torch.matmul
    K, N = (S // 8) ** 2 * 24, 512
    xs = torch.rand((B, K), generator=g, device=dev) - 0.5
    dy = torch.rand((B, N), generator=g, device=dev) - 0.5
    wt = torch.rand((K, N), generator=g, device=dev) - 0.5
    dwt, db = torch.empty_like(wt), torch.empty(N, device=dev)

    def lin_ours():
        ops.linear_wgrad(xs, dy, dwt, db)
        return ops.linear_dgrad(dy, wt)

    def lin_torch():
        return torch.matmul(xs.t(), dy), dy.sum(0), torch.matmul(dy, wt.t())

    ours_dx, (t_dwt, t_db, t_dx) = lin_ours(), lin_torch()
    assert float((ours_dx - t_dx).abs().max()) <= 1e-4 * float(t_dx.abs().max())
    assert float((dwt - t_dwt).abs().max()) <= 1e-4 * float(t_dwt.abs().max())
    lin_ms, lin_torch_ms = [], []
    for _ in range(a.rounds):
        lin_ms += timed(lin_ours, 1)
        lin_torch_ms += timed(lin_torch, 1)

    # ---- the step and its parts
    step_ms = timed(lambda: tr.step(uv, z), a.rounds)
    fwd_ms = timed(lambda: tr.forward(x), a.rounds)
    loss_ms = timed(lambda: tr.loss(z), a.rounds)

    def backward_only():
        tr.forward(x)
        _, gz = tr.loss(z)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.backward(gz)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    bwd_ms = [backward_only() for _ in range(a.rounds + 1)][1:]
    adam_ms = timed(lambda: ops.adam_step(tr.p, tr.g, tr.m, tr.v, 0.0, 0.5, 0.999, 1e-8, 1), a.rounds)
    med = lambda v: float(np.median(v))        # noqa: E731
    res = {"batch": B, "size": S, "rounds": a.rounds,
           "step_ms": round(med(step_ms), 2), "step_img_s": round(B / med(step_ms) * 1e3, 1),
           "render_ms": round(med(render_ms), 3), "forward_ms": round(med(fwd_ms), 2), "loss_kernel_ms": round(med(loss_ms), 3),
           "backward_ms": round(med(bwd_ms), 2), "adam_ms": round(med(adam_ms), 3),
           "gauss_heatmaps_ms": round(med(render_ms), 3), "torch_render_ms": round(med(torch_render_ms), 3),
           "host_render_upload_ms": round(med(host_render_ms), 1),
           "gauss_heatmaps_over_torch": round(med(render_ms) / med(torch_render_ms), 4),
           "linear_bwd_fc1_ms": round(med(lin_ms), 3), "torch_matmul_fc1_ms": round(med(lin_torch_ms), 3),
           "linear_bwd_over_torch": round(med(lin_ms) / med(lin_torch_ms), 4),
           "parameters": int((~tr.padding_mask()).sum()),
           "weights": "generated (tests/_hpe_oracle.py)", "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("# tools/bench_hpe3d_train.py: one training step of the 3D estimator (generated weights) and its parts; the input render\n"
                 "# next to the host's float64 numpy target + upload (wall clock) and to torch device ops; the Linear backward at\n"
                 "# depth_fc_1's shape next to torch.matmul; times in ms are medians of HIP-event pairs with the host enqueue included\n"
                 + line + "\n")


if __name__ == "__main__":
    main()
