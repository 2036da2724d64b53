"""What --depth_source joints costs and saves: the depth render (mmh_render_pose_depth) behind the decode pass, and the loaders
with two PNGs per pair instead of four.

    python tools/bench_render_depth.py [--pairs 128] [--batch 32] [--visits 5] [--out profiles/render_depth.txt]

Part 1, the kernels alone at B = 32, 256 x 256, HIP events, interleaved run by run in one process as
tools/bench_decode_affine.py times the decode entry points: (a) mmh_decode_inputs_indexed, (b) the same followed by the render
of both sides into its x_d, (c) the render alone.  Joints as the loaders' fixtures draw them (uniform over the image's inner
part), radius 5, bg 255.

Part 2, the file-fed loader (PIL) on a temporary directory of 256 x 256 PNGs, decoded form, at nThreads 4 and 16, with
`files` and with `joints`, alternating visits.

Part 3, the resident loader in its epochs >= 2, both modes, alternating visits, with the store's byte count in each.  The last
line sets the joints-mode rate against what the bf16 step consumes (README, `bf16_path`): the loader has to out-deliver it by
2x at least for the step never to wait."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
BF16_STEP_IMAGES_PER_S = (333.8, 349.3)         # README, `bf16_path`: the range over four boxes


def kernel_times(dev, B=32, size=256, runs=30, per_event=10):
    from mmhand_amd import lib as L
    g = torch.Generator(device=dev).manual_seed(0)
    store = torch.randint(0, 256, (4 * B, size, size, 3), generator=g, device=dev, dtype=torch.uint8)
    idx = (torch.arange(B, device=dev, dtype=torch.int32)[:, None] + torch.arange(4, device=dev, dtype=torch.int32)[None] * B).contiguous()
    rs = np.random.RandomState(0)
    xyz = np.concatenate([rs.uniform(20, size - 20, size=(2, B, 21, 2)), rs.uniform(100, 690, size=(2, B, 21, 1)) / 700.0 * 255], -1)
    table = np.zeros((4 * B, 21, 2))
    table[:B], table[B:2 * B] = xyz[0, :, :, :2], xyz[1, :, :, :2]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)         # noqa: E731
    c1, c2, table = t(xyz[0]), t(xyz[1]), t(table)
    outs = [torch.empty((B, size, size, c), dtype=torch.float32, device=dev) for c in (4, 4, 44, 8)]
    lib = L.load()
    p = lambda a: C.c_void_p(a.data_ptr())                        # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    decode = ("mmh_decode_inputs_indexed", [p(store), 4 * B, size, size, p(idx), p(table), B, size, size, 6.0] + [p(a) for a in outs] + [None, stream])
    render = ("mmh_render_pose_depth", [p(c1), p(c2), B, size, size, 5.0, 255.0, p(outs[3]), 8, stream])
    cases = {"(a) mmh_decode_inputs_indexed": [decode], "(b) (a) + mmh_render_pose_depth, both sides": [decode, render],
             "(c) mmh_render_pose_depth alone": [render]}

    def run(calls):
        for fn, args in calls:
            L.check(getattr(lib, fn)(*args), fn)
    for calls in cases.values():
        for _ in range(3):
            run(calls)
    torch.cuda.synchronize()
    covered = float((outs[3][..., 0] < 1.0).float().mean())
    times = {name: [] for name in cases}
    for _ in range(runs):
        for name, calls in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            run(calls)
            e0.record()
            for _ in range(per_event):
                run(calls)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / per_event)
    base = statistics.median(times["(a) mmh_decode_inputs_indexed"])
    lines = [f"{name:46s} {statistics.median(v):8.1f} us  [{min(v):8.1f} .. {max(v):8.1f}]  {statistics.median(v) / base:5.2f} x (a)"
             for name, v in times.items()]
    r = statistics.median(times["(c) mmh_render_pose_depth alone"])
    lines.append(f"the render writes {B * size * size * 32 / 1e6:.1f} MB of x_d: {B * size * size * 32 / r / 1e3:.0f} GB/s; "
                 f"{covered:.2f} of side 0's pixels are covered by a bone")
    return lines


def one_pass(loader, epoch=0):
    loader.set_epoch(epoch)
    t0 = time.perf_counter()
    n = 0
    for b in loader:
        torch.cuda.synchronize()
        n += len(b["H1_path"])
    return n / (time.perf_counter() - t0)


def _opt(root, batch, mode):
    from mmhand_amd.options import default_train_opt
    return default_train_opt(batchSize=batch, dataroot=root, dataset="rhd", augmentation_ratio=1.0, depth_source=mode)


def file_rates(dev, root, batch, visits):
    from mmhand_amd.data import HandFolderLoader
    loaders = {(th, mode): HandFolderLoader(_opt(root, batch, mode), device=dev, decoded=True, threads=th)
               for th in (4, 16) for mode in ("files", "joints")}
    for ld in loaders.values():
        one_pass(ld)                                            # page cache and allocator warm
    rates = {k: [] for k in loaders}
    for _ in range(visits):
        for k, ld in loaders.items():
            rates[k].append(one_pass(ld))
    return rates


def resident_rates(dev, root, batch, visits):
    from mmhand_amd.data import HandFolderLoader
    loaders = {}
    for mode in ("files", "joints"):
        ld = HandFolderLoader(_opt(root, batch, mode), device=dev, decoded=True, resident=True, threads=16)
        one_pass(ld, 0)                                          # the fill epoch
        assert ld.resident_state.startswith("on") and all(ld._batch_is_resident(g) for g in range(ld.n_batches()))
        one_pass(ld, 1)
        loaders[mode] = ld
    rates = {k: [] for k in loaders}
    for v in range(visits):
        for k, ld in loaders.items():
            rates[k].append(one_pass(ld, 2 + v))
    return rates, {k: ld.resident_state for k, ld in loaders.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--visits", type=int, default=5)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    from bench_loader import write_dir
    lines = [f"--- decode pass and depth render, B = {args.batch}, {args.size} x {args.size}, HIP events, 30 interleaved runs of 10 "
             "launches: median [min .. max]"]
    lines += kernel_times(dev, B=args.batch, size=args.size)
    root = tempfile.mkdtemp(prefix="mmh_render_")
    try:
        write_dir(root, args.pairs, args.size, 1)
        fr = file_rates(dev, root, args.batch, args.visits)
        rr, states = resident_rates(dev, root, args.batch, args.visits)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    fmt = lambda r: f"{statistics.median(r):9.1f} pairs/s  [{min(r):9.1f} .. {max(r):9.1f}]"     # noqa: E731
    lines.append(f"--- file-fed loader (PIL), decoded form, {args.size} x {args.size}, batch {args.batch}, {args.pairs} pairs per pass, "
                 f"{args.visits} interleaved visits: median [min .. max]")
    for (th, mode), r in fr.items():
        lines.append(f"nThreads {th:2d}, --depth_source {mode:6s} ({4 if mode == 'files' else 2} PNGs per pair)  {fmt(r)}")
    lines.append(f"--- resident loader, epochs >= 2, decoded form, batch {args.batch}, {args.visits} interleaved visits: median [min .. max]")
    for mode, r in rr.items():
        lines.append(f"--depth_source {mode:6s}  {fmt(r)}   store {states[mode]}")
    worst = min(rr["joints"])
    lines.append(f"joints mode, slowest visit {worst:.1f} pairs/s = {worst / BF16_STEP_IMAGES_PER_S[1]:.1f} x the bf16 step's "
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
