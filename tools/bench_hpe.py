"""Measures the PCK estimators (mmhand_amd/hpe.py, csrc/hpe.hip) on one MI355X and writes profiles/hpe.txt:

* images/s of HPEstimator.predict (normalise -> Hpm2d -> upsample + arg-max -> Hpm3d) at B = 32, 256 x 256, full width,
  interleaved round by round with the Generator's fp32 inference (InferenceGenerator, ngf 64, 9 blocks) on the same box;
* the three new kernels alone at the shapes that pipeline gives them: median of `--runs` HIP-event pairs after warm-up.

The weights are generated (tests/_hpe_oracle.py): the rates do not depend on them, and no accuracy is reported.  These are
measurements; nothing here is a bar.

    python tools/bench_hpe.py [--batch 32] [--size 256] [--rounds 5] [--runs 30] [--out profiles/hpe.txt]"""
import argparse
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, runs, warm=3):
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
    p.add_argument("--runs", type=int, default=30)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpe.txt"))
    a = p.parse_args()
    from mmhand_amd import hpe, ops
    from mmhand_amd.inference import InferenceGenerator
    from mmhand_amd.networks import Generator
    from tests import _hpe_oracle as O
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    B, S = a.batch, a.size
    f32 = lambda sd: OrderedDict((k, v.float()) for k, v in sd.items())        # noqa: E731
    est = hpe.HPEstimator(f32(O.state_dict("2d", O.FULL)), f32(O.state_dict("3d", O.FULL, head_hw=S // 8)), device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    img = torch.rand((B, 3, S, S), generator=g, device=dev) * 2 - 1
    torch.manual_seed(0)
    gen = InferenceGenerator(Generator([3, 42, 6], 3, 64, "batch", True, 9).to(dev).eval(), use_graph=True, bf16=False)
    gin = [img, torch.rand((B, 42, S, S), generator=g, device=dev), torch.rand((B, 6, S, S), generator=g, device=dev) * 2 - 1]

    est_ms, gen_ms = [], []
    for _ in range(a.rounds):                       # interleaved: one estimator batch, one generator batch, per round
        est_ms += timed(lambda: est.predict(img), 1, warm=1)
        gen_ms += timed(lambda: gen(gin), 1, warm=1)
    # the stages of one estimator batch
    x = ops.hpe_normalize(img)
    cat = est.hpm2d(x)
    up, _, _ = ops.heatmap_upsample_argmax(cat)
    flat = torch.rand((min(B, 64), 24 * (S // 8) ** 2), generator=g, device=dev)
    wt, bias = est.hpm3d.fc[0]
    stage = {"hpe_normalize": timed(lambda: ops.hpe_normalize(img), a.runs),
             "heatmap_upsample_argmax": timed(lambda: ops.heatmap_upsample_argmax(cat), a.runs),
             "linear_fc1": timed(lambda: ops.linear(flat, wt, bias), a.runs),
             "hpm2d": timed(lambda: est.hpm2d(x), max(3, a.rounds)), "hpm3d": timed(lambda: est.hpm3d(up), max(3, a.rounds))}
    med = lambda v: float(np.median(v))        # noqa: E731
    res = {"batch": B, "size": S, "rounds": a.rounds,
           "estimator_ms": round(med(est_ms), 2), "estimator_img_s": round(B / med(est_ms) * 1e3, 1),
           "generator_fp32_ms": round(med(gen_ms), 2), "generator_fp32_img_s": round(B / med(gen_ms) * 1e3, 1),
           "stages_ms": {k: round(med(v), 3) for k, v in stage.items()},
           "linear_fc1_GBps": round(wt.numel() * 4 / med(stage["linear_fc1"]) / 1e6, 1),
           "upsample_GBps": round(up.numel() * 4 / med(stage["heatmap_upsample_argmax"]) / 1e6, 1),
           "weights": "generated (tests/_hpe_oracle.py)", "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("# tools/bench_hpe.py: PCK estimators (generated weights) next to the Generator's fp32 inference, interleaved;\n"
                 "# times in ms are medians (HIP events, host enqueue included for the whole-network rows)\n" + line + "\n")


if __name__ == "__main__":
    main()
