"""Measures the Inception score path (mmhand_amd/inception.py, csrc/inception.hip, mmh_conv2d_fprop_rect) on one MI355X and
writes profiles/inception.txt:

* images/s of preprocess -> InceptionV3 -> score at B = 32 from 256 x 256 inputs, interleaved round by round with the
  Generator's fp32 inference (InferenceGenerator, ngf 64, 9 blocks) on the same box;
* the new kernels alone at the shapes that pipeline gives them: median of `--runs` HIP-event pairs after warm-up.

The weights are generated (tests/_inception_oracle.py): the rates do not depend on them, and no score is reported.  No parent
path exists for any of this: these are measurements, nothing here is a bar or a speed-up.

    python tools/bench_inception.py [--batch 32] [--size 256] [--rounds 5] [--runs 30] [--out profiles/inception.txt]"""
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
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "inception.txt"))
    a = p.parse_args()
    from mmhand_amd import inception, lib, ops
    from mmhand_amd.inference import InferenceGenerator
    from mmhand_amd.networks import Generator
    from tests import _inception_oracle as O
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    B, S = a.batch, a.size
    sd = OrderedDict((k, v.float() if v.is_floating_point() else v) for k, v in O.state_dict(0).items())
    scorer = inception.InceptionScorer(sd, group=64, device=dev)
    net = scorer.net
    g = torch.Generator(device=dev).manual_seed(0)
    img = torch.rand((B, 3, S, S), generator=g, device=dev) * 2 - 1
    torch.manual_seed(0)
    gen = InferenceGenerator(Generator([3, 42, 6], 3, 64, "batch", True, 9).to(dev).eval(), use_graph=True, bf16=False)
    gin = [img, torch.rand((B, 42, S, S), generator=g, device=dev), torch.rand((B, 6, S, S), generator=g, device=dev) * 2 - 1]

    def chain():
        return ops.inception_score(scorer.logits(img))

    is_ms, gen_ms = [], []
    for _ in range(a.rounds):                       # interleaved: one scored batch, one generator batch, per round
        is_ms += timed(chain, 1, warm=1)
        gen_ms += timed(lambda: gen(gin), 1, warm=1)
    tables = scorer.tables(S, S)
    x = ops.inception_preprocess(img, "nchw", tables)
    logits = net(x)
    x35 = torch.rand((B, 35, 35, 288), generator=g, device=dev)
    x17 = torch.rand((B, 17, 17, 160), generator=g, device=dev)
    x8 = torch.rand((B, 8, 8, 2048), generator=g, device=dev)
    w17, b17 = net.convs["Mixed_6c.branch7x7_2"]
    w71, b71 = net.convs["Mixed_6c.branch7x7dbl_2"]
    stage = {"inception_preprocess": timed(lambda: ops.inception_preprocess(img, "nchw", tables), a.runs),
             "avg_pool_35x35x288": timed(lambda: ops.pool3x3(x35, "avg"), a.runs),
             "max_pool_35x35x288": timed(lambda: ops.pool3x3(x35, "max"), a.runs),
             "global_avgpool_8x8x2048": timed(lambda: ops.global_avgpool(x8), a.runs),
             "conv_1x7_17x17x160": timed(lambda: ops.conv_fprop_direct(x17, w17, b17, 0, 3, act=lib.ACT_RELU), a.runs),
             "conv_7x1_17x17x160": timed(lambda: ops.conv_fprop_direct(x17, w71, b71, 3, 0, act=lib.ACT_RELU), a.runs),
             "inception_score": timed(lambda: ops.inception_score(logits), a.runs),
             "inception_v3": timed(lambda: net(x), max(3, a.rounds))}
    med = lambda v: float(np.median(v))        # noqa: E731
    flops_17 = 2.0 * B * 17 * 17 * 160 * 160 * 7
    res = {"batch": B, "size": S, "rounds": a.rounds,
           "inception_score_chain_ms": round(med(is_ms), 2), "inception_score_chain_img_s": round(B / med(is_ms) * 1e3, 1),
           "generator_fp32_ms": round(med(gen_ms), 2), "generator_fp32_img_s": round(B / med(gen_ms) * 1e3, 1),
           "stages_ms": {k: round(med(v), 3) for k, v in stage.items()},
           "preprocess_GBps": round((img.numel() * 4 + x.numel() * 4) / med(stage["inception_preprocess"]) / 1e6, 1),
           "avg_pool_GBps": round(2 * x35.numel() * 4 / med(stage["avg_pool_35x35x288"]) / 1e6, 1),
           "conv_1x7_TFLOPs": round(flops_17 / med(stage["conv_1x7_17x17x160"]) / 1e9, 2),
           "conv_7x1_TFLOPs": round(flops_17 / med(stage["conv_7x1_17x17x160"]) / 1e9, 2),
           "weights": "generated (tests/_inception_oracle.py)", "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("# tools/bench_inception.py: Inception score path (generated weights) next to the Generator's fp32 inference,\n"
                 "# interleaved; times in ms are medians (HIP events, host enqueue included for the whole-network rows); a recorded\n"
                 "# measurement of a new path: no bar, no speed-up\n" + line + "\n")


if __name__ == "__main__":
    main()
