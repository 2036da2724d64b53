"""Times mmh_image_metrics (csrc/metrics.hip) on B=64 pairs of 3x256x256 fp32 NCHW images: median of >= 20 launches
timed with HIP events after warm-up (the C entry point alone, ten launches per event pair), in us, effective GB/s
(both images read once) and as a fraction of the fp32 VALU bound; then evaluate.py's images/s in directory mode and in
generator mode on a synthetic prepared directory, next to aug.py's rate on the same directory.  Prints one JSON line.

    python tools/bench_metrics.py [--runs 50] [--images 64] [--size 64] [--skip_eval]"""
import argparse
import json
import os
import random
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# MI355X: 256 CUs x 128 fp32 FMA per CU and clock (157.3 TFLOP/s fp32 vector, packed) at 2.4 GHz
FMA_PER_S = 256 * 128 * 2.4e9


def valu_ops_per_pixel(window):
    """fp32 VALU operations per output pixel of the tile kernel as written: horizontal pass (halo rows / 32 per output
    row; per 2 output columns 2 (w + 1) shifts, 3 (w + 1) products, 10 w FMAs) + vertical pass (per group of 4 rows
    (w + 3) rows of 2 shifts and 12 re-centring operations, 20 w FMAs) + ~25 for the SSIM combine"""
    rows = (32 + window - 1) / 32.0
    horiz = rows * (5 * (window + 1) + 10 * window) / 2.0
    vert = ((window + 3) * 14 + 20 * window) / 4.0
    return horiz + vert + 25


def bench_kernel(runs, B=64, C=3, H=256, W=256, window=11, per_event=10):
    """mmh_image_metrics alone: workspace, output, descriptors and taps prepared once, the C entry point called
    directly; `per_event` launches back to back between one event pair (one launch enqueued ahead, so the stream is busy
    when the first event fires and host enqueue time is not counted), the median over `runs` pairs, per launch"""
    import ctypes as C_
    from mmhand_amd import lib as L
    from mmhand_amd.metrics import C1, C2, _src, gaussian_taps
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    a = torch.rand((B, C, H, W), generator=g, device=dev) * 2 - 1
    b = (a + 0.1 * torch.randn((B, C, H, W), generator=g, device=dev)).clamp(-1, 1)
    lib = L.load()
    sa, _ = _src(a, "pm1")
    sb, _ = _src(b, "pm1")
    nbytes = lib.mmh_image_metrics_ws_bytes(B, C, H, W, window)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((B, 3), dtype=torch.float64, device=dev)
    taps = gaussian_taps(window)
    args = (C_.byref(sa), C_.byref(sb), B, C, H, W, window, taps.ctypes.data_as(C_.c_void_p), C1, C2,
            C_.c_void_p(ws.data_ptr()), nbytes, C_.c_void_p(out.data_ptr()),
            C_.c_void_p(torch.cuda.current_stream().cuda_stream))

    def launch():
        L.check(lib.mmh_image_metrics(*args), "mmh_image_metrics")

    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        launch()                                   # keeps the stream busy while e0 and the timed launches are enqueued
        e0.record()
        for _ in range(per_event):
            launch()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / per_event)
    med = float(np.median(times))
    nbytes = 2 * a.numel() * 4
    ops = valu_ops_per_pixel(window) * a.numel()
    return {"shape": [B, C, H, W], "window": window, "runs": runs, "launches_per_event_pair": per_event,
            "median_us": round(med, 2), "min_us": round(float(np.min(times)), 2), "GBps": round(nbytes / med / 1e3, 1),
            "valu_bound_us": round(ops / FMA_PER_S * 1e6, 2), "valu_fraction": round(ops / FMA_PER_S * 1e6 / med, 3)}


def bench_eval(n_images, size, batch):
    """images/s of evaluate (generator and directory modes) and aug.py on one synthetic prepared directory (ngf 64,
    9 blocks, batch norm: aug.py's hard-coded generator, random weights)"""
    from tests._dataset_fixture import write_rhd
    from mmhand_amd import aug, evaluate
    from mmhand_amd.networks import Generator
    work = tempfile.mkdtemp(prefix="mmh_bm_")
    cwd = os.getcwd()
    try:
        root = os.path.join(work, "rhd")
        write_rhd(root, n=2 * n_images, size=size)
        os.chdir(work)
        os.makedirs(os.path.join("checkpoints", "bm"))
        torch.manual_seed(0)
        torch.save(Generator([3, 42, 6], 3, 64, "batch", True, 9).state_dict(),
                   os.path.join("checkpoints", "bm", "latest_net_netG.pth"))
        out = {}
        base = ["--dataroot", root, "--dataset", "rhd", "--augmentation_ratio", "0.5", "--batchSize", str(batch)]
        for key, argv in (("evaluate_generator", ["--name", "bm"] + base), ):
            evaluate.main(argv + ["--results_json", "w.json"])                  # warm-up: capture, first reads
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            evaluate.main(argv + ["--results_json", "r.json"])
            out[key + "_img_s"] = round(n_images / (time.perf_counter() - t0), 1)
        random.seed(0)
        aug.main(["bm", root, "gen", "rhd", "0.5", "0"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        aug.main(["bm", root, "gen", "rhd", "0.5", "0"])
        out["aug_img_s"] = round(n_images / (time.perf_counter() - t0), 1)
        argv = ["--generated", "gen"] + base
        evaluate.main(argv)
        t0 = time.perf_counter()
        evaluate.main(argv)
        out["evaluate_directory_img_s"] = round(n_images / (time.perf_counter() - t0), 1)
        out.update(images=n_images, size=size, batchSize=batch)
        return out
    finally:
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=50)
    p.add_argument("--images", type=int, default=64)
    p.add_argument("--size", type=int, default=64)
    p.add_argument("--batchSize", type=int, default=16)
    p.add_argument("--skip_eval", action="store_true")
    args = p.parse_args()
    assert args.runs >= 20
    torch.cuda.set_device(0)
    res = {"kernel": bench_kernel(args.runs)}
    if not args.skip_eval:
        res["pipeline"] = bench_eval(args.images, args.size, args.batchSize)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
