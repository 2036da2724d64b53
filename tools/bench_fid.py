"""Times the FID / KID path (mmhand_amd/fid.py, csrc/fid.hip) on one MI355X with generated weights:

* the feature pass: ops.inception_preprocess + InceptionV3.features of 32 images of 256 x 256 (features / s);
* ops.feature_moments (mmh_feature_moments) at N = 2048 / 8192 / 32768 rows of d = 2048;
* ops.poly_mmd_sums (mmh_poly_mmd_sums) at S = 100 subsets of M = 1000 out of 4096 rows, and at S = 1 over N = 8192 rows.

Device time: HIP events around one call (its launches and the wrapper's allocations, which torch's caching allocator serves from
its pool after warm-up), one call enqueued ahead so that the stream is busy when the first event fires; `--warmup` calls first,
then the median [min .. max] of `--runs` (>= 10) calls.

The parent commit has no such path, so there is no bar and no speed-up claim: next to each kernel stands the float64 numpy
formulation on the same box's threads (OMP_NUM_THREADS, 16 here) - np.mean + np.cov(rowvar=False), and blocked `A @ B.T`
(1024-row blocks), t = dot / d + 1, (t t) t, the three sums - wall clock, its runs interleaved with the device's (one numpy run
after every fifth device run), median of `--cpu_runs`.  TFLOP/s counts what the MFMA multiplies: d (d + 64) N for the upper
tiles of the covariance, 2 d (Ma^2 / 2 + Mb^2 / 2 + Ma Mb) per subset up to tile rounding.  The microarchitecture guide this
project works from lists no fp64 MFMA peak; the figure used is the MI355X data sheet's 78.6 TFLOP/s of fp64 matrix throughput.

    python tools/bench_fid.py [--runs 15] [--warmup 3] [--cpu_runs 3] [--out profiles/fid.txt]"""
import argparse
import os
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_MATRIX_PEAK_TF = 78.6
D = 2048


def timed(fn, cpu_fn, runs, warmup, cpu_runs):
    """-> (device ms [runs], numpy ms [cpu_runs]); the numpy runs sit between the device runs"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    dev_ms, cpu_ms = [], []
    for i in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()                    # keeps the stream busy while e0 and the timed call are enqueued
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
        if cpu_fn is not None and i % 5 == 4 and len(cpu_ms) < cpu_runs:
            t0 = time.perf_counter()
            cpu_fn()
            cpu_ms.append((time.perf_counter() - t0) * 1e3)
    return dev_ms, cpu_ms


def numpy_moments(X64):
    return X64.mean(0), np.cov(X64, rowvar=False)


def numpy_mmd_sums(A, B, ia, ib, block=1024):
    d = A.shape[1]
    out = np.zeros((len(ia), 3))

    def total(x, y, skip_diag):
        s = 0.0
        for i in range(0, len(x), block):
            t = x[i:i + block] @ y.T / d + 1.0
            k = (t * t) * t
            s += k.sum()
            if skip_diag:
                s -= np.trace(k[:, i:i + block])
        return s

    for s in range(len(ia)):
        a, b = A[ia[s]], B[ib[s]]
        out[s] = [total(a, a, True), total(b, b, True), total(a, b, False)]
    return out


def fmt(name, dev_ms, cpu_ms, flop):
    med = float(np.median(dev_ms))
    tf = flop / med / 1e9
    cpu = float(np.median(cpu_ms)) if cpu_ms else float("nan")
    return (f"{name:<44} {med:>10.3f} {'[%.3f .. %.3f]' % (min(dev_ms), max(dev_ms)):>24} {tf:>9.2f} {100 * tf / FP64_MATRIX_PEAK_TF:>7.1f}% "
            f"{cpu:>11.1f} {len(cpu_ms):>4} {cpu / med:>9.1f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu_runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 10 and a.warmup >= 1 and 1 <= a.cpu_runs <= a.runs // 5
    assert torch.cuda.is_available(), "bench_fid.py measures on the GPU; there is no fallback"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    from mmhand_amd import fid, inception, ops
    from tests import _inception_oracle as O

    lines = [f"FID / KID path, HIP events, {a.warmup} warm-up calls, median [min .. max] of {a.runs} calls; beside each kernel the float64 "
             f"numpy formulation (np.mean + np.cov; blocked A @ B.T), OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}, wall clock, "
             f"median of {a.cpu_runs} runs interleaved with the device's.  Recorded measurements: the parent has no such path, no bar."]

    # ---- the feature pass
    sd = OrderedDict((k, v.float() if v.is_floating_point() else v) for k, v in O.state_dict(0).items())
    net = inception.InceptionV3(dev).load_state_dict(sd)
    sc = fid.FidScorer(net, device=dev)
    images = torch.from_numpy(np.concatenate([O.images(8, 256, 256, s) for s in range(4)])).to(dev)
    ms, _ = timed(lambda: sc.features(images, "nchw"), None, a.runs, a.warmup, 0)
    med = float(np.median(ms))
    lines.append(f"features: preprocess + InceptionV3.features, B = 32 from 256 x 256 (generated weights): {med:.2f} ms "
                 f"[{min(ms):.2f} .. {max(ms):.2f}] = {32e3 / med:.0f} images / s")
    print(lines[-1], flush=True)
    del net, sc, images
    torch.cuda.empty_cache()

    lines.append(f"{'kernel':<44} {'device ms':>10} {'[min .. max]':>24} {'TFLOP/s':>9} {'of 78.6':>8} {'numpy ms':>11} {'runs':>4} {'numpy/dev':>10}")
    rs = np.random.RandomState(0)
    # ---- moments
    for n in (2048, 8192, 32768):
        X = np.abs(rs.randn(n, D)).astype(np.float32)
        X64 = X.astype(np.float64)
        Xd = torch.from_numpy(X).to(dev)
        mean, cov = ops.feature_moments(Xd)
        want = np.cov(X64, rowvar=False)
        err = float(np.abs(cov.cpu().numpy() - want).max() / np.abs(want).max())
        dev_ms, cpu_ms = timed(lambda: ops.feature_moments(Xd), lambda: numpy_moments(X64), a.runs, a.warmup, a.cpu_runs)
        lines.append(fmt(f"feature_moments N = {n}, d = {D}", dev_ms, cpu_ms, float(D) * (D + 64) * n) + f"   max |cov - np.cov| / max |cov| = {err:.1e}")
        print(lines[-1], flush=True)
        del Xd, X64
    # ---- kernel sums
    for name, na, S, M in (("S = 100, M = 1000 of 4096", 4096, 100, 1000), ("S = 1, all N = 8192", 8192, 1, 8192)):
        A = np.abs(rs.randn(na, D)).astype(np.float32)
        B = np.abs(rs.randn(na, D) + 0.1).astype(np.float32)
        ia, ib = (np.arange(na, dtype=np.int32)[None], np.arange(na, dtype=np.int32)[None]) if S == 1 else fid.draw_subsets(na, na, S, M, 0)
        Ad, Bd = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
        A64, B64 = A.astype(np.float64), B.astype(np.float64)
        got = ops.poly_mmd_sums(Ad, Bd, ia, ib).cpu().numpy()
        want = numpy_mmd_sums(A64, B64, ia[:2], ib[:2])
        err = float(np.abs(got[:len(want)] / want - 1.0).max())
        dev_ms, cpu_ms = timed(lambda: ops.poly_mmd_sums(Ad, Bd, ia, ib), lambda: numpy_mmd_sums(A64, B64, ia, ib), a.runs, a.warmup, a.cpu_runs)
        lines.append(fmt(f"poly_mmd_sums {name}, d = {D}", dev_ms, cpu_ms, 2.0 * D * S * 2.0 * M * M) + f"   max rel. difference to numpy = {err:.1e}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
