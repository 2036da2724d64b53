"""Times the LPIPS path (mmhand_amd/lpips.py, csrc/lpips.hip) on one MI355X with generated weights, at B = 32 pairs of 256 x 256:

* the scorer: LpipsScorer.distances of 32 pairs - both sides' preprocess and VGG-16 trunk and the five layer distances (pairs / s);
* the trunk alone: ops.lpips_preprocess + Vgg16Lpips.forward_taps of one side;
* each of the five mmh_lpips_layer launches (the layer kernel and its finishing launch) on that forward's taps, with the bytes it
  must read - both maps once, 2 B H W C 4 bytes - over its time as achieved GB/s;
* the same five distances built from torch device operations on the same tensors, in fp32 as the `lpips` package computes them:
  sqrt(sum(x ** 2)), x / (norm + eps) for both maps, the squared difference, times w, the two sums.

Device time: HIP events around `--reps` back-to-back calls (the layer launches are tens of microseconds at the deep taps), one call
enqueued ahead so that the stream is busy when the first event fires; `--warmup` calls first, then the median [min .. max] of
`--runs` event pairs, per call.  The wrappers' allocations are inside (torch's caching allocator serves them from its pool after
warm-up).  The parent commit has no such path, so there is no bar and no speed-up claim; the share of the achievable HBM rate
uses the 6.3 TB/s of the microarchitecture notes this project works from.  The deep taps (33 MB and less per side) fit the
256 MiB Infinity Cache, so their rates are cache rates, not HBM rates.

    python tools/bench_lpips.py [--runs 15] [--warmup 3] [--reps 10] [--batch 32] [--size 256] [--out profiles/lpips.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE_GBS = 6300.0
EPS = 1e-10


def timed(fn, runs, warmup, reps):
    """-> ms per call [runs]"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()                    # keeps the stream busy while e0 and the timed calls are enqueued
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out


def torch_layer(a, b, w):
    """the package's arithmetic on NHWC tensors: normalize_tensor, squared difference, the 1x1 head, the spatial mean; fp32"""
    na = torch.sqrt(torch.sum(a ** 2, dim=3, keepdim=True))
    nb = torch.sqrt(torch.sum(b ** 2, dim=3, keepdim=True))
    d = (a / (na + EPS) - b / (nb + EPS)) ** 2
    return (d * w).sum(3).mean((1, 2))


def spread(ms):
    return f"{float(np.median(ms)):>9.3f} {'[%.3f .. %.3f]' % (min(ms), max(ms)):>22}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 5 and a.warmup >= 1 and a.reps >= 1 and a.size % 16 == 0
    assert torch.cuda.is_available(), "bench_lpips.py measures on the GPU; there is no fallback"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    from mmhand_amd import lpips, ops
    from tests import _lpips_oracle as O

    B, S = a.batch, a.size
    net = lpips.Vgg16Lpips(dev).load_state_dict(O.vgg16_state_dict(0))
    sc = lpips.LpipsScorer(net, O.lin_state_dict(1), device=dev)
    g = torch.Generator().manual_seed(3)
    pred = (torch.rand((B, 3, S, S), generator=g) * 2 - 1).to(dev)
    target = (torch.rand((B, 3, S, S), generator=g) * 2 - 1).to(dev)
    lines = [f"LPIPS path (VGG-16, generated weights), B = {B} pairs of {S} x {S}, HIP events around {a.reps} back-to-back calls, {a.warmup} "
             f"warm-up calls, median [min .. max] of {a.runs} event pairs, ms per call.  Recorded measurements: the parent has no such "
             f"path, no bar."]

    ms = timed(lambda: sc.distances(pred, "nchw", target, "nchw"), a.runs, a.warmup, 1)
    med = float(np.median(ms))
    lines.append(f"scorer: LpipsScorer.distances (2 x preprocess, 2 x trunk, 5 layer distances): {spread(ms)} ms = {B * 1e3 / med:.0f} pairs / s")
    print(lines[-1], flush=True)
    ms = timed(lambda: net.forward_taps(ops.lpips_preprocess(pred, "nchw")), a.runs, a.warmup, 1)
    lines.append(f"trunk:  ops.lpips_preprocess + Vgg16Lpips.forward_taps of one side ({B} images):    {spread(ms)} ms")
    print(lines[-1], flush=True)

    ta = net.forward_taps(ops.lpips_preprocess(pred, "nchw"))
    tb = net.forward_taps(ops.lpips_preprocess(target, "nchw"))
    lines.append("per tap: mmh_lpips_layer (kernel) against the torch fp32 formulation on the same tensors")
    lines.append(f"{'tap':<28} {'MB read':>9} {'kernel ms':>9} {'[min .. max]':>22} {'GB/s':>8} {'of 6300':>8} "
                 f"{'torch ms':>9} {'[min .. max]':>22} {'torch/kernel':>12} {'|kernel - torch| / |w| scale':>28}")
    tot_k = tot_t = 0.0
    for l in range(5):
        fa, fb, w = ta[l], tb[l], sc.lin[l]
        nbytes = 2.0 * fa.numel() * 4
        got = ops.lpips_layer(fa, fb, w)
        ref = torch_layer(fa, fb, w).double()
        scale = torch_layer(fa, fb, w.abs()).double()
        err = float(((got - ref).abs() / scale).max())
        k_ms = timed(lambda: ops.lpips_layer(fa, fb, w), a.runs, a.warmup, a.reps)
        t_ms = timed(lambda: torch_layer(fa, fb, w), a.runs, a.warmup, max(1, a.reps // 5))
        km, tm = float(np.median(k_ms)), float(np.median(t_ms))
        tot_k, tot_t = tot_k + km, tot_t + tm
        gbs = nbytes / km / 1e6
        lines.append(f"{'%d: [%d,%d,%d,%d]' % (l, *fa.shape):<28} {nbytes / 1e6:>9.1f} {spread(k_ms)} {gbs:>8.0f} {100 * gbs / HBM_ACHIEVABLE_GBS:>7.1f}% "
                     f"{spread(t_ms)} {tm / km:>11.1f}x {err:>28.1e}")
        print(lines[-1], flush=True)
    lines.append(f"five taps: mmh_lpips_layer {tot_k:.3f} ms, torch device ops {tot_t:.3f} ms ({tot_t / tot_k:.1f}x)")
    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
