"""What --augment_geom costs: the slot-fed decode pass with a sampling matrix per image (mmh_decode_inputs_indexed_affine)
next to the pass it stands beside (mmh_decode_inputs_indexed), and the resident loader's delivery with and without the flag.

    python tools/bench_decode_affine.py [--pairs 128] [--batch 32] [--visits 5] [--out profiles/decode_affine.txt]

Part 1, the kernels alone at B = 32, 256 x 256, HIP events, interleaved run by run in one process as
tools/bench_loader.py times the decode entry points: (a) mmh_decode_inputs_indexed, (b) the new kernel with identity
matrices (same taps, same bytes: what the matrix arithmetic and the per-sample joints cost), (c) the new kernel with matrices
drawn from the default ranges (rotate 15, scale 0.1, shift 0.05: rotated gathers).  (b) must write (a)'s bits.

Part 2, the resident loader in its epochs >= 2 on a temporary directory of 256 x 256 PNGs, decoded form (every batch ends in
the decode pass), with and without the flag, alternating visits; every visit of the flagged loader is a new epoch number, so
its host-side table build and upload are inside the figure.  The last line sets the flagged rate against what the bf16 step
consumes (README, `bf16_path`): the loader has to out-deliver it by 2x at least for the step never to wait."""
import argparse
import ctypes as C
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BF16_STEP_IMAGES_PER_S = (333.8, 349.3)         # README, `bf16_path`: the range over four boxes


def kernel_times(dev, B=32, size=256, runs=30, per_event=10):
    from mmhand_amd import lib as L
    from mmhand_amd.data import affine_forward, affine_inverse, affine_joints, augment_draws
    from mmhand_amd.options import default_train_opt
    g = torch.Generator(device=dev).manual_seed(0)
    store = torch.randint(0, 256, (4 * B, size, size, 3), generator=g, device=dev, dtype=torch.uint8)
    idx = (torch.arange(B, device=dev, dtype=torch.int32)[:, None] + torch.arange(4, device=dev, dtype=torch.int32)[None] * B).contiguous()
    rs = np.random.RandomState(0)
    uv0 = rs.uniform(20, size - 20, size=(B, 2, 21, 2))
    table = np.zeros((4 * B, 21, 2))
    table[:B], table[B:2 * B] = uv0[:, 0], uv0[:, 1]
    d = augment_draws(B, 0, default_train_opt(augment_geom=True, aug_pair="independent", dataroot="-"))
    fwd = affine_forward(d[..., 0], d[..., 1], d[..., 2], d[..., 3], d[..., 4], (size, size))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)         # noqa: E731
    ident = t(np.tile([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], (B, 2, 1)))
    drawn, uv_drawn = t(affine_inverse(fwd, (size, size)).reshape(B, 2, 6)), t(affine_joints(uv0, fwd, (size, size)))
    uv_id, table = t(uv0), t(table)
    outs = [torch.empty((B, size, size, c), dtype=torch.float32, device=dev) for c in (4, 4, 44, 8)]
    lib = L.load()
    p = lambda a: C.c_void_p(a.data_ptr())                        # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = [p(a) for a in outs]
    head = [p(store), 4 * B, size, size, p(idx)]
    cases = {
        "(a) mmh_decode_inputs_indexed": ("mmh_decode_inputs_indexed", head + [p(table), B, size, size, 6.0] + o + [None, stream]),
        "(b) _indexed_affine, identity": ("mmh_decode_inputs_indexed_affine", head + [p(uv_id), p(ident), B, size, size, 6.0] + o + [None, stream]),
        "(c) _indexed_affine, default ranges": ("mmh_decode_inputs_indexed_affine", head + [p(uv_drawn), p(drawn), B, size, size, 6.0] + o + [None, stream]),
    }
    kept = {}
    for name, (fn, args) in cases.items():
        for _ in range(3):
            L.check(getattr(lib, fn)(*args), fn)
        torch.cuda.synchronize()
        kept[name] = [a.clone() for a in outs]
    a, b, c = kept.values()
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "identity matrices do not write the indexed pass's bits"
    assert not torch.equal(a[0], c[0])
    times = {name: [] for name in cases}
    for _ in range(runs):
        for name, (fn, args) in cases.items():
            f = getattr(lib, fn)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            L.check(f(*args), fn)
            e0.record()
            for _ in range(per_event):
                L.check(f(*args), fn)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / per_event)
    nbytes = B * size * size * 240 + 4 * B * size * size * 3
    base = statistics.median(times["(a) mmh_decode_inputs_indexed"])
    return [f"{name:38s} {statistics.median(v):8.1f} us  [{min(v):8.1f} .. {max(v):8.1f}]  {nbytes / statistics.median(v) / 1e3:6.0f} GB/s"
            f"  {statistics.median(v) / base:5.2f} x (a)" for name, v in times.items()]


def one_pass(loader, epoch):
    loader.set_epoch(epoch)
    t0 = time.perf_counter()
    n = 0
    for b in loader:
        torch.cuda.synchronize()
        n += len(b["H1_path"])
    return n / (time.perf_counter() - t0)


def loader_rates(dev, pairs, batch, size, visits):
    from bench_loader import write_dir
    from mmhand_amd.data import HandFolderLoader
    from mmhand_amd.options import default_train_opt
    root = tempfile.mkdtemp(prefix="mmh_affine_")
    try:
        write_dir(root, pairs, size, 1)
        loaders = {}
        for name, flag in (("resident, epochs >= 2", False), ("resident, epochs >= 2, --augment_geom", True)):
            opt = default_train_opt(batchSize=batch, dataroot=root, dataset="rhd", augmentation_ratio=1.0, augment_geom=flag)
            ld = HandFolderLoader(opt, device=dev, decoded=True, resident=True, threads=16)
            one_pass(ld, 0)                                          # the fill epoch
            assert ld.resident_state.startswith("on") and all(ld._batch_is_resident(g) for g in range(ld.n_batches()))
            one_pass(ld, 1)
            loaders[name] = ld
        rates = {name: [] for name in loaders}
        for v in range(visits):
            for name, ld in loaders.items():
                rates[name].append(one_pass(ld, 2 + v))
        return rates
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--visits", type=int, default=5)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"--- decode pass alone, B = {args.batch}, {args.size} x {args.size}, HIP events, 30 interleaved runs of 10 launches: "
             "median [min .. max]"]
    lines += kernel_times(dev, B=args.batch, size=args.size)
    rates = loader_rates(dev, args.pairs, args.batch, args.size, args.visits)
    lines.append(f"--- resident loader, decoded form, {args.size} x {args.size}, batch {args.batch}, {args.pairs} pairs per pass, "
                 f"{args.visits} interleaved visits (a new epoch number each): median [min .. max]")
    for name, r in rates.items():
        lines.append(f"{name:38s} {statistics.median(r):9.1f} pairs/s  [{min(r):9.1f} .. {max(r):9.1f}]")
    worst = min(rates["resident, epochs >= 2, --augment_geom"])
    lines.append(f"with the flag, slowest visit {worst:.1f} pairs/s = {worst / BF16_STEP_IMAGES_PER_S[1]:.1f} x the bf16 step's "
                 f"consumption ({BF16_STEP_IMAGES_PER_S[0]} - {BF16_STEP_IMAGES_PER_S[1]} images/s, README `bf16_path`; the upper end "
                 f"taken); the condition is >= 2 x: {'met' if worst >= 2 * BF16_STEP_IMAGES_PER_S[1] else 'NOT met'}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
