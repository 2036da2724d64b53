"""The write side of `python -m mmhand_amd.aug` on a temporary prepared directory of 256 x 256 PNGs: today's inline PIL save,
PIL on 16 writer threads, and --device_png (mmh_png_encode_batch + a writer pool), at batch 1 and 64.

    python tools/bench_aug_write.py [--images 256] [--visits 3] [--out profiles/aug_png_ab.txt]

Two measurements per method and batch size, images/s, median [min .. max] over interleaved visits:
  write half   a uint8 [B,256,256,3] device batch - the output of a random-init Generator (ngf 64, 9 blocks) on the first
               pairs of the directory, held fixed - goes to files again and again: .cpu() + Image.save, or encode + write
  whole loop   loader -> Generator forward (BN folded, hipGraph) -> files, over the whole directory, the loop alone (model
               load, BN fold and graph capture happen before the timer): aug's own --device_png loop; aug.main's inline loop
               restated here; and that loop with the saves handed to 16 threads, which is not an `aug` mode
The directory is photo-like (tools/bench_loader.write_dir: smooth shading plus sensor-like noise).  The generated images of a
random-init Generator are NOT photo-like: they are smooth enough that zlib's matches halve the file, so the mean file sizes
the table prints show the Huffman-only encoder at its worst against PIL; the same images go through every row."""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

METHODS = ("PIL inline (today)", "PIL x 16 threads", "--device_png")


def pil_save(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)


def write_half(method, batch, paths, pool, enc):
    """one pass over `paths` in chunks of batch.shape[0]; returns images/s"""
    from mmhand_amd.aug import _write_file
    B = batch.shape[0]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    jobs = []
    for k in range(0, len(paths), B):
        chunk = paths[k:k + B]
        if method == METHODS[2]:
            files, _ = enc.encode(batch[:len(chunk)])
            jobs += [pool.submit(_write_file, p, f) for p, f in zip(chunk, files)]
        else:
            arr = batch[:len(chunk)].cpu().numpy()
            if method == METHODS[0]:
                for p, a in zip(chunk, arr):
                    pil_save(p, a)
            else:
                jobs += [pool.submit(pil_save, p, a) for p, a in zip(chunk, arr)]
    for j in jobs:
        j.result()
    return len(paths) / (time.perf_counter() - t0)


def make_gen(dev):
    from mmhand_amd.inference import InferenceGenerator
    from mmhand_amd.networks import Generator
    model = Generator(input_nc=[3, 42, 6], output_nc=3, ngf=64, norm_layer="batch", use_dropout=True, n_blocks=9)
    model.load_state_dict(torch.load(os.path.join("checkpoints", "bench", "latest_net_netG.pth"), map_location="cpu"))
    return InferenceGenerator(model.to(dev).eval(), use_graph=True)


def make_loader(root, batch, dev):
    from mmhand_amd.data import HandFolderLoader
    from mmhand_amd.options import default_train_opt
    opt = default_train_opt(batchSize=batch, local_rank=0, isTrain=False)
    opt.dataroot, opt.dataset, opt.augmentation_ratio, opt.distributed = root, "rhd", 0.0, False
    return HandFolderLoader(opt, device=dev, decoded=True)


def whole_loop(method, gen, loader, dst, dev, pool):
    """one pass of aug's generation loop over the directory, the loop alone: the generator (weights loaded, BN folded, graph
    captured by the warm-up visit) and the loader are built outside the timer.  --device_png runs aug._generate_device_png
    itself; the inline row is aug.main's loop restated (main keeps it inline), the pooled row the same with the saves handed
    to the pool."""
    from mmhand_amd import aug
    shutil.rmtree(dst, ignore_errors=True)
    os.makedirs(dst)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if method == METHODS[2]:
        n = len(aug._generate_device_png(loader, gen, dst, dev, threads=16))
    else:
        jobs, n = [], 0
        for sample in loader:
            fake = gen([sample["H1"], torch.cat((sample["P1"], sample["P2"]), 1), torch.cat((sample["D1"], sample["D2"]), 1)])
            arr = ((fake.permute(0, 2, 3, 1) * 0.5 + 0.5) * 255.0).round().clamp(0, 255).to(torch.uint8).cpu().numpy()
            for j in range(arr.shape[0]):
                path = aug._target_path(dst, sample["H2_path"][j])
                if method == METHODS[0]:
                    pil_save(path, arr[j])
                else:
                    jobs.append(pool.submit(pil_save, path, arr[j]))
                n += 1
        for j in jobs:
            j.result()
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--visits", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from bench_loader import write_dir
    from mmhand_amd.data import HandFolderLoader
    from mmhand_amd.inference import InferenceGenerator
    from mmhand_amd.networks import Generator
    from mmhand_amd.options import default_train_opt
    from mmhand_amd.png import PngBatchEncoder
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    work = tempfile.mkdtemp(prefix="mmh_augw_")
    lines = []
    try:
        os.chdir(work)
        root = os.path.join(work, "rhd")
        write_dir(root, args.images, 256, None)
        os.makedirs(os.path.join("checkpoints", "bench"))
        model = Generator(input_nc=[3, 42, 6], output_nc=3, ngf=64, norm_layer="batch", use_dropout=True, n_blocks=9)
        torch.save(model.init_weights("normal", seed=7).state_dict(), os.path.join("checkpoints", "bench", "latest_net_netG.pth"))
        # the fixed batch of the write half: 64 generated images
        gen = InferenceGenerator(model.to(dev).eval(), use_graph=False)
        opt = default_train_opt(batchSize=64, local_rank=0, isTrain=False)
        opt.dataroot, opt.dataset, opt.augmentation_ratio, opt.distributed = root, "rhd", 0.0, False
        sample = next(iter(HandFolderLoader(opt, device=dev, decoded=True)))
        fake = gen([sample["H1"], torch.cat((sample["P1"], sample["P2"]), 1), torch.cat((sample["D1"], sample["D2"]), 1)])
        fixed = ((fake.permute(0, 2, 3, 1) * 0.5 + 0.5) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
        del gen, model
        enc, sizes = PngBatchEncoder(dev), {}
        files, _ = enc.encode(fixed[:8])
        sizes["device"] = sum(map(len, files)) / 8
        import io
        from PIL import Image
        tot = 0
        for a in fixed[:8].cpu().numpy():
            b = io.BytesIO()
            Image.fromarray(a).save(b, format="PNG")
            tot += len(b.getvalue())
        sizes["pil"] = tot / 8
        out_dir = os.path.join(work, "w")
        os.makedirs(out_dir)
        paths = [os.path.join(out_dir, f"{i:05d}.png") for i in range(args.images)]
        res, gens = {}, {}
        with ThreadPoolExecutor(max_workers=16) as pool:
            for what in ("write half", "whole loop"):
                for visit in range(args.visits + 1):              # visit 0 warms up (graph capture, buffers, page cache)
                    for B in (1, 64):
                        for m in METHODS:
                            if what == "write half":
                                v = write_half(m, fixed[:B], paths, pool, enc)
                            else:
                                if B not in gens:
                                    gens[B] = make_gen(dev)
                                v = whole_loop(m, gens[B], make_loader(root, B, dev), os.path.join(work, "gen"), dev, pool)
                            if visit:
                                res.setdefault((what, B, m), []).append(v)
        lines.append(f"aug write side, images/s, 256x256, {args.images} images per pass, {args.visits} interleaved visits after one "
                     f"warm-up: median [min .. max]; 16 writer threads at most")
        lines.append(f"mean file of the generated (random-init Generator) images: device encoder {sizes['device'] / 1024:.1f} KiB, "
                     f"PIL default {sizes['pil'] / 1024:.1f} KiB (ratio {sizes['device'] / sizes['pil']:.4f})")
        for what in ("write half", "whole loop"):
            lines.append(f"--- {what}")
            for B in (1, 64):
                for m in METHODS:
                    v = res[(what, B, m)]
                    lines.append(f"batch {B:<3d} {m:<22s} {statistics.median(v):9.1f}  [{min(v):9.1f} .. {max(v):9.1f}]")
    finally:
        os.chdir(ROOT)
        shutil.rmtree(work, ignore_errors=True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
