"""Loader-only throughput of HandFolderLoader on a temporary prepared directory of 256 x 256 PNGs: today's PIL path against
--device_png, at nThreads 4 and 16, and against (c) --resident_dataset in its epochs >= 2 (the store filled by the warm-up
pass), interleaved in one process (alternating visits; medians and spread over the visits), plus the PNG decode kernel's own
time per batch of 128 images from HIP events.

    python tools/bench_loader.py [--pairs 128] [--batch 32] [--visits 5] [--out profiles/loader_resident_ab.txt]

The images are photo-like (smooth shading plus sensor-like noise), written by PIL at its default settings and at
compress_level=1.  Iterate, to_device, synchronise per batch; no model.  Two forms: the RAW form (uint8 batches as
MMHandModel.set_input takes them; a resident batch in this form is a dictionary and no device work, so (c) measures the
host loop alone) and the DECODED form (decoded=True: every batch ends in the decode pass - mmh_decode_inputs for (a) and (b),
mmh_decode_inputs_indexed for (c) - i.e. up to the tensors the networks read; the figure to compare).  Last, the event-timed
cost of mmh_decode_inputs_indexed next to mmh_decode_inputs (and mmh_decode_inputs_resized at the identity size, the
batch-fed kernel with the indexed one's lane layout) at B = 32, 256 x 256, interleaved, as tools/bench_decode_resize.py
times them."""
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
        n += len(b["H1_path"])
    return n / (time.perf_counter() - t0)


def decode_kernel_times(dev, B=32, size=256, runs=30, per_event=10):
    """us per launch of the three decode entry points on the same 4 x B images, interleaved run by run: median [min .. max]
    over `runs` event pairs of `per_event` back-to-back launches (one more enqueued ahead, so host enqueue time is not
    counted).  All three read 4 B size^2 3 bytes and write 240 bytes per pixel."""
    import ctypes as C
    from mmhand_amd import lib as L
    g = torch.Generator(device=dev).manual_seed(0)
    raw = [torch.randint(0, 256, (B, size, size, 3), generator=g, device=dev, dtype=torch.uint8) for _ in range(4)]
    uv = [torch.rand((B, 21, 2), generator=g, device=dev, dtype=torch.float64) * (size - 40) + 20 for _ in range(2)]
    outs = [torch.empty((B, size, size, c), dtype=torch.float32, device=dev) for c in (4, 4, 44, 8)]
    store = torch.cat(raw).contiguous()                         # slot j * B + b = image b of source j
    table = torch.cat(uv + uv).contiguous()
    idx = (torch.arange(B, device=dev, dtype=torch.int32)[:, None] + torch.arange(4, device=dev, dtype=torch.int32)[None] * B).contiguous()
    lib = L.load()
    p = lambda t: C.c_void_p(t.data_ptr())                        # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = [p(t) for t in outs]
    cases = {
        "mmh_decode_inputs": [p(t) for t in raw + uv] + [B, size, size, 6.0] + o + [stream],
        "mmh_decode_inputs_resized": [p(t) for t in raw + uv] + [B, size, size, size, size, 6.0] + o + [stream],
        "mmh_decode_inputs_indexed": [p(store), 4 * B, size, size, p(idx), p(table), B, size, size, 6.0] + o + [None, stream],
    }
    ref = None
    for name, args in cases.items():                              # warm, and the three write the same bits
        for _ in range(3):
            L.check(getattr(lib, name)(*args), name)
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        ref = ref or got
        assert all(torch.equal(a, b) for a, b in zip(ref, got)), name
    times = {name: [] for name in cases}
    for _ in range(runs):
        for name, args in cases.items():
            fn = getattr(lib, name)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            L.check(fn(*args), name)
            e0.record()
            for _ in range(per_event):
                L.check(fn(*args), name)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / per_event)
    nbytes = B * size * size * 240 + 4 * B * size * size * 3
    return [f"{name:28s} {statistics.median(t):8.1f} us  [{min(t):8.1f} .. {max(t):8.1f}]  {nbytes / statistics.median(t) / 1e3:6.0f} GB/s"
            for name, t in times.items()]


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
            variants.append(("(c) resident, epochs >= 2", dict(resident=True, threads=16)))
            variants += [(f"decoded: {name}", dict(decoded=True, threads=16, **kw)) for name, kw in
                         (("(a) PIL nThreads=16", dict(device_png=False)), ("(b) device_png nThreads=16", dict(device_png=True)),
                          ("(c) resident, epochs >= 2", dict(resident=True)))]
            loaders = {}
            for name, kw in variants:
                opt = default_train_opt(batchSize=args.batch, dataroot=root, dataset="rhd", augmentation_ratio=1.0)
                loaders[name] = HandFolderLoader(opt, device=dev, **kw)
                one_pass(loaders[name])                              # warm: page cache, pinned buffers, first launch
                if kw.get("resident"):                               # ... and for (c) the fill epoch: every visit is resident
                    assert loaders[name].resident_state.startswith("on"), loaders[name].resident_state
                    assert all(loaders[name]._batch_is_resident(g) for g in range(loaders[name].n_batches()))
            rates = {name: [] for name, _ in variants}
            for _ in range(args.visits):
                for name, _ in variants:
                    rates[name].append(one_pass(loaders[name]))
            lines.append(f"--- files written with {tag}: mean colour file {mean / 1024:.1f} KiB")
            for name, _ in variants:
                r = rates[name]
                lines.append(f"{name:38s} {statistics.median(r):9.1f} pairs/s  [{min(r):9.1f} .. {max(r):9.1f}]")
            n, med, lo, hi = kernel_time(root, dev)
            lines.append(f"mmh_png_decode_batch, {n} images in one launch: {med:.3f} ms  [{lo:.3f} .. {hi:.3f}]")
        finally:
            shutil.rmtree(root, ignore_errors=True)
    lines.append(f"--- decode pass alone, B = {args.batch}, {args.size} x {args.size}, HIP events, 30 interleaved runs of 10 launches: "
                 "median [min .. max]")
    lines += decode_kernel_times(dev, B=args.batch, size=args.size)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
