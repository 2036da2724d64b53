"""Loader-only throughput of HandFolderLoader on a temporary prepared directory of 256 x 256 PNGs: today's PIL path against
--device_png, at nThreads 4 and 16, interleaved in one process (alternating visits; medians and spread over the visits), plus
the decode kernel's own time per batch of 128 images from HIP events.

    python tools/bench_loader.py [--pairs 128] [--batch 32] [--visits 5] [--out profiles/loader_png_ab.txt]

The images are photo-like (smooth shading plus sensor-like noise), written by PIL at its default settings and at
compress_level=1.  Iterate, to_device, synchronise per batch; no model."""
import argparse
import os
import pickle
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_dir(root, n, size, level, seed=1):
    from PIL import Image
    rs = np.random.RandomState(seed)
    ann = {"color": {}, "depth": {}}
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float32) / size
    for folder in ann:
        os.makedirs(os.path.join(root, folder), exist_ok=True)
    for i in range(n):
        name = f"{i:05d}.png"
        lab = {"uv_coord": rs.uniform(20, size - 20, size=(21, 2)).tolist(), "depth": rs.uniform(100, 690, size=21).tolist()}
        for folder in ann:
            ann[folder][name] = lab
            f = rs.uniform(1, 4, size=3)
            base = np.stack([np.sin(f[c] * 3 * xx + i) * np.cos(f[c] * 2 * yy) for c in range(3)], -1) * 90 + 128
            img = np.clip(base + rs.normal(0, 4, size=base.shape), 0, 255).astype(np.uint8)
            kw = {} if level is None else {"compress_level": level}
            Image.fromarray(img).save(os.path.join(root, folder, name), **kw)
    with open(os.path.join(root, "annotation.pickle"), "wb") as fh:
        pickle.dump(ann, fh)
    return sum(os.path.getsize(os.path.join(root, "color", f)) for f in os.listdir(os.path.join(root, "color"))) / n


def one_pass(loader):
    t0 = time.perf_counter()
    n = 0
    for b in loader:
        torch.cuda.synchronize()
        n += b["img1"].shape[0]
    return n / (time.perf_counter() - t0)


def kernel_time(root, dev, reps=5):
    """ms per mmh_png_decode_batch of 128 images (32 pairs x 4 files), HIP events around the launch alone"""
    import ctypes as C
    from mmhand_amd import lib as L
    from mmhand_amd.png import PngBatchDecoder
    files = []
    for folder in ("color", "depth"):
        for f in sorted(os.listdir(os.path.join(root, folder)))[:64]:
            with open(os.path.join(root, folder, f), "rb") as fh:
                files.append(fh.read())
    dec = PngBatchDecoder(dev)
    plan = dec.pack(files)
    dec.launch(plan)
    n, h, w, nbytes = plan[:4]
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        L.call("mmh_png_decode_batch", C.c_void_p(dec.stream_d.data_ptr()), nbytes, C.c_void_p(dec.off_d.data_ptr()), n, h, w,
               C.c_void_p(dec.scratch.data_ptr()), C.c_void_p(dec.out.data_ptr()), C.c_void_p(dec.st_d.data_ptr()), 1,
               C.c_void_p(torch.cuda.current_stream().cuda_stream))
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    assert int(dec.st_d[:n].abs().sum()) == 0
    return n, statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--visits", type=int, default=5)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from mmhand_amd.data import HandFolderLoader
    from mmhand_amd.options import default_train_opt
    dev = torch.device("cuda", 0)
    lines = [f"loader-only images/s (pairs/s x 1; each pair = 4 PNG files), {args.size}x{args.size}, batch {args.batch}, "
             f"{args.pairs} pairs per pass, {args.visits} interleaved visits: median [min .. max]"]
    for tag, level in (("PIL default", None), ("compress_level=1", 1)):
        root = tempfile.mkdtemp(prefix="mmh_loader_")
        try:
            mean = write_dir(root, args.pairs, args.size, level)
            variants = [(f"{name} nThreads={t}", dict(device_png=png, threads=t)) for t in (4, 16)
                        for name, png in (("(a) PIL", False), ("(b) device_png", True))]
            loaders = {}
            for name, kw in variants:
                opt = default_train_opt(batchSize=args.batch, dataroot=root, dataset="rhd", augmentation_ratio=1.0)
                loaders[name] = HandFolderLoader(opt, device=dev, **kw)
                one_pass(loaders[name])                              # warm: page cache, pinned buffers, first launch
            rates = {name: [] for name, _ in variants}
            for _ in range(args.visits):
                for name, _ in variants:
                    rates[name].append(one_pass(loaders[name]))
            lines.append(f"--- files written with {tag}: mean colour file {mean / 1024:.1f} KiB")
            for name, _ in variants:
                r = rates[name]
                lines.append(f"{name:28s} {statistics.median(r):8.1f} pairs/s  [{min(r):8.1f} .. {max(r):8.1f}]")
            n, med, lo, hi = kernel_time(root, dev)
            lines.append(f"mmh_png_decode_batch, {n} images in one launch: {med:.3f} ms  [{lo:.3f} .. {hi:.3f}]")
        finally:
            shutil.rmtree(root, ignore_errors=True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
