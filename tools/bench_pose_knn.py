"""Times the pose-distance search (csrc/pose_knn.hip) through its Python surface: ops.pose_features + ops.pose_knn of N poses
against themselves (every pose excludes itself: the loader's `--pairing nearest --match_pool self`), N = 4096, 16384 and 41258
(the RHD training set), k = 1 and k = 16.

Device time: HIP events around features + kNN (three launches and the wrappers' allocations, which torch's caching allocator
serves from its pool after warm-up), one call enqueued ahead so that the stream is busy when the first event fires; `--warmup`
calls first, then the median [min .. max] of `--runs` (>= 10) calls.  GFLOP/s = 2 N^2 64 over that time: the products alone,
what the MFMA does - the selection epilogue is not counted as work, it is what the rest of the time goes to.

Yardstick: the parent commit has no such path, so it is a float64 numpy formulation on the same box - the same features, then
blocks of 1024 queries: `F[block] @ F.T` (BLAS, the threads OMP_NUM_THREADS gives it; 16 here), the diagonal masked,
`argpartition` for the k best and a sort of those.  Wall clock, best of `--cpu_runs` (1 at the two larger sizes by default: a
run takes seconds).  The two results are compared: the share of queries whose k indices agree exactly is printed (cosines that
differ in the last bits can swap two neighbours; the tests assert exactness on inputs with a checked gap).

    python tools/bench_pose_knn.py [--runs 15] [--warmup 3] [--out profiles/pose_knn.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (4096, 16384, 41258)
KS = (1, 16)


def draw_poses(n, seed=7, size=256):
    rs = np.random.RandomState(seed)
    uv = rs.uniform(0, size, size=(n, 21, 2))
    z = rs.uniform(100, 690, size=(n, 21, 1)) / 700.0 * 255
    return np.concatenate([uv, z], axis=-1)


def cpu_knn(poses, k, block=1024):
    d = (poses[:, 1:] - poses[:, :-1]).reshape(len(poses), 60)
    f = d / np.linalg.norm(d, axis=1, keepdims=True)
    n = len(f)
    idx = np.empty((n, k), dtype=np.int64)
    for b in range(0, n, block):
        cos = f[b:b + block] @ f.T
        rows = np.arange(cos.shape[0])
        cos[rows, b + rows] = -np.inf
        if k < n - 1:
            part = np.argpartition(-cos, k - 1, axis=1)[:, :k]
        else:
            part = np.tile(np.arange(n), (cos.shape[0], 1))[:, :k]
        order = np.argsort(-np.take_along_axis(cos, part, 1), axis=1, kind="stable")
        idx[b:b + block] = np.take_along_axis(part, order, 1)
    return idx


def device_knn(poses_dev, exclude, k):
    from mmhand_amd import ops
    f = ops.pose_features(poses_dev)
    return ops.pose_knn(f, f, k, exclude=exclude)


def bench(n, k, runs, warmup, cpu_runs):
    dev = torch.device("cuda", 0)
    poses = draw_poses(n)
    poses_dev = torch.from_numpy(poses).to(dev)
    exclude = torch.arange(n, dtype=torch.int32, device=dev)
    for _ in range(warmup):
        idx, _ = device_knn(poses_dev, exclude, k)
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        device_knn(poses_dev, exclude, k)          # keeps the stream busy while e0 and the timed call are enqueued
        e0.record()
        idx, _ = device_knn(poses_dev, exclude, k)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    cpu_times = []
    for _ in range(cpu_runs):
        t0 = time.perf_counter()
        want = cpu_knn(poses, k)
        cpu_times.append((time.perf_counter() - t0) * 1e3)
    agree = float((idx.cpu().numpy() == want).all(1).mean())
    med = float(np.median(times))
    return dict(n=n, k=k, med=med, lo=float(np.min(times)), hi=float(np.max(times)), gflops=2.0 * n * n * 64 / med / 1e6,
                cpu=float(np.min(cpu_times)), cpu_runs=cpu_runs, agree=agree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu_runs", type=int, default=0, help="0: 3 at N = 4096, 1 at the larger sizes")
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 10 and a.warmup >= 1
    assert torch.cuda.is_available(), "bench_pose_knn.py measures on the GPU; there is no fallback"
    torch.cuda.set_device(0)
    lines = [f"pose_features + pose_knn of N poses against themselves (self excluded), HIP events, {a.warmup} warm-up calls, median "
             f"[min .. max] of {a.runs} calls; yardstick: float64 numpy (blocked F @ F.T + argpartition), "
             f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}, wall clock, best of its runs",
             f"{'N':>6} {'k':>3} {'device ms':>10} {'[min .. max]':>22} {'GFLOP/s (products)':>19} {'numpy ms':>10} {'runs':>4} "
             f"{'numpy / device':>14} {'queries agreeing':>16}"]
    for n in a.sizes:
        for k in KS:
            r = bench(n, k, a.runs, a.warmup, a.cpu_runs or (3 if n <= 4096 else 1))
            lines.append(f"{r['n']:>6} {r['k']:>3} {r['med']:>10.3f} {'[%.3f .. %.3f]' % (r['lo'], r['hi']):>22} {r['gflops']:>19.0f} "
                         f"{r['cpu']:>10.1f} {r['cpu_runs']:>4} {r['cpu'] / r['med']:>13.1f}x {100 * r['agree']:>15.3f}%")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
