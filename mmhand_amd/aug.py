"""Generation driver — counterpart of the reference's aug.py:14-71.

    python -m mmhand_amd.aug <checkpoint_name> <dataroot> <dst_dir> <rhd|stb> <ratio> <device>     (the reference's argv, aug.py:16)
    python -m mmhand_amd.aug <checkpoint_name> <dst_dir> [n_batches] [batch] [device]              (synthetic batches)

`--resize_inputs N` (an addition, anywhere on the first form's command line): the pairs reach the generator at N x N whatever
size the files hold - the resize is part of the device's decode pass - and the PNGs are written at that size.
`--batch N` (an addition, first form): the loader's batch size; the default 1 is the reference's.
`--device_png` (an addition, first form, opt-in): the uint8 batch stays on the device, `png.PngBatchEncoder` produces the files'
bytes (row filters + Huffman-only DEFLATE in csrc/png_encode.hip), a pool of at most 16 threads writes them, and the next
batch's forward is enqueued before the previous batch's bytes are fetched.  Same file names, same pixels, other bytes than
PIL's.  MMH_DEVICE_PNG (the loader's switch for the input side) does not turn it on.
`--pairing random|curriculum|nearest`, `--match_pool self|train` (additions, first form): how a target gets its source image
(data.HandFolderLoader): `nearest` is the paper's inference with nearest-neighbour match - the source whose 3D pose is closest
to the target's, out of the generation split itself or of the training share.  The file names do not change: one PNG per target.

The first form reads the reference's prepared directory (data.HandFolderLoader: annotation.pickle + colour / depth PNGs,
the generation side of the augmentation_ratio split, batch size 1, decoded on the device) and writes each generated image
to <dst>/<folder of the TARGET image>/<its file name> (aug.py:66-71).

Loads checkpoints/<name>/latest_net_netG.pth (reference format), builds
Generator([3,42,6],3,64,BatchNorm,use_dropout=True,n_blocks=9).eval(), folds BN into the convs,
captures the forward in a hipGraph and writes the generated images ((x*0.5+0.5)*255, RGB->BGR
then cv2.imwrite) as PNG files via PIL (cv2 is absent here; cv2.imwrite of a BGR float array
rounds to nearest uint8 and stores RGB-ordered PNG pixels, which is what PIL is given) or, without
PIL, as .npy arrays."""
import argparse
import os
import sys

import numpy as np
import torch

from .data import MATCH_POOLS, PAIRINGS, HandFolderLoader, SyntheticHandLoader
from .inference import InferenceGenerator
from .networks import Generator
from .options import check_resize_inputs, default_train_opt


def _target_path(dst, h2_path):
    # aug.py:66-71: <dst>/<folder of the target image>/<its file name>
    *_, folder, name = h2_path.split("/")
    os.makedirs(os.path.join(dst, folder), exist_ok=True)
    return os.path.join(dst, folder, name)


def _write_file(path, data):
    with open(path, "wb") as f:
        f.write(data)


def _generate_device_png(loader, gen, dst, dev, threads):
    """the --device_png loop: forward i is enqueued, then batch i - 1's bytes are fetched and handed to the writer pool, then
    batch i's encode is enqueued behind its forward (one encoder: its buffers are free again once i - 1 is fetched)"""
    from concurrent.futures import ThreadPoolExecutor

    from .png import PngBatchEncoder
    enc = PngBatchEncoder(dev)
    written, jobs, pending = [], [], None
    with ThreadPoolExecutor(max_workers=max(1, min(16, threads))) as pool:
        def drain(plan, paths):
            files, _ = enc.fetch(plan)
            while jobs and jobs[0].done():
                jobs.pop(0).result()                                # a failed write raises here, a batch later at most
            for path, data in zip(paths, files):
                jobs.append(pool.submit(_write_file, path, data))
                written.append(path)
        for sample in loader:
            fake = gen([sample["H1"], torch.cat((sample["P1"], sample["P2"]), 1),
                        torch.cat((sample["D1"], sample["D2"]), 1)])
            img = ((fake.permute(0, 2, 3, 1) * 0.5 + 0.5) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
            paths = [_target_path(dst, p) for p in sample["H2_path"][:img.shape[0]]]
            if pending is not None:
                drain(*pending)
            pending = (enc.launch(img), paths)
        if pending is not None:
            drain(*pending)
        for j in jobs:
            j.result()
    return written


def main(argv, ngf=64, n_blocks=9, size=None, resize_inputs=0):
    """argv as the reference's aug.py; ngf / n_blocks / size are the reference's hard-coded 64 / 9 / 256 (aug.py:31-39),
    keyword-overridable so that a test can drive the whole path on a small checkpoint.  resize_inputs = N, or
    `--resize_inputs N` in argv: the prepared directory's pairs are decoded to N x N (options.check_resize_inputs)."""
    argv = list(argv)
    if "--resize_inputs" in argv:
        i = argv.index("--resize_inputs")
        if i + 1 >= len(argv) or not argv[i + 1].lstrip("-").isdigit():
            raise ValueError("--resize_inputs: expected an integer")
        resize_inputs = int(argv[i + 1])
        del argv[i:i + 2]
    check_resize_inputs(argparse.Namespace(resize_inputs=resize_inputs))
    batch_flag, device_png = 1, False
    if "--batch" in argv:
        i = argv.index("--batch")
        if i + 1 >= len(argv) or not argv[i + 1].isdigit() or int(argv[i + 1]) < 1:
            raise ValueError("--batch: expected a positive integer")
        batch_flag = int(argv[i + 1])
        del argv[i:i + 2]
    if "--device_png" in argv:
        argv.remove("--device_png")
        device_png = True
    pair_flags = {}
    for flag, allowed in (("--pairing", PAIRINGS), ("--match_pool", MATCH_POOLS)):
        if flag in argv:
            i = argv.index(flag)
            if i + 1 >= len(argv) or argv[i + 1] not in allowed:
                raise ValueError(f"{flag}: expected one of {' | '.join(allowed)}")
            pair_flags[flag[2:]] = argv[i + 1]
            del argv[i:i + 2]
    ckp = argv[0]
    real = len(argv) == 6 and argv[3] in ("rhd", "stb")        # _, ckp, dataroot, DST, dataset, ratio, device = sys.argv
    if real:
        dataroot, dst, dataset, ratio, device = argv[1], argv[2], argv[3], float(argv[4]), int(argv[5])
        n_batches, batch = None, batch_flag
    else:
        if device_png or batch_flag != 1:
            raise ValueError("--device_png / --batch belong to the prepared-directory form of the command line")
        if pair_flags:
            raise ValueError("--pairing / --match_pool belong to the prepared-directory form of the command line")
        dst = argv[1]
        n_batches = int(argv[2]) if len(argv) > 2 else 4
        batch = int(argv[3]) if len(argv) > 3 else 1
        device = int(argv[4]) if len(argv) > 4 else 0
    torch.cuda.set_device(device)
    dev = torch.device("cuda", device)
    weights = torch.load(os.path.join("checkpoints", ckp, "latest_net_netG.pth"), map_location="cpu")
    model = Generator(input_nc=[3, 42, 6], output_nc=3, ngf=ngf, norm_layer="batch", use_dropout=True,
                      n_blocks=n_blocks)
    model.load_state_dict(weights)
    gen = InferenceGenerator(model.to(dev).eval(), use_graph=True)
    opt = default_train_opt(batchSize=batch, local_rank=device, isTrain=False, resize_inputs=resize_inputs)
    if real:
        # aug.py:18-26: isTrain False, batchSize 1, not distributed; the loader hands decoded NCHW views
        opt.dataroot, opt.dataset, opt.augmentation_ratio, opt.distributed = dataroot, dataset, ratio, False
        for name, value in pair_flags.items():
            setattr(opt, name, value)
        loader = HandFolderLoader(opt, device=dev, decoded=True)
    else:
        loader = SyntheticHandLoader(opt, n_batches * batch, size=size)
    os.makedirs(dst, exist_ok=True)
    if device_png:
        return _generate_device_png(loader, gen, dst, dev, threads=16)
    written = []
    for i, sample in enumerate(loader):
        fake = gen([sample["H1"], torch.cat((sample["P1"], sample["P2"]), 1),
                    torch.cat((sample["D1"], sample["D2"]), 1)])
        img = ((fake.permute(0, 2, 3, 1) * 0.5 + 0.5) * 255.0).round().clamp(0, 255).to(torch.uint8)
        arr = img.cpu().numpy()                                     # RGB, what the PNG stores
        for j in range(arr.shape[0]):
            # aug.py:66-71: <dst>/<folder of the target image>/<its file name>
            *_, folder, name = sample["H2_path"][j].split("/")
            os.makedirs(os.path.join(dst, folder), exist_ok=True)
            path = os.path.join(dst, folder, name)
            try:
                from PIL import Image
                Image.fromarray(arr[j]).save(path)
            except ImportError:
                path = os.path.splitext(path)[0] + ".npy"
                np.save(path, arr[j])
            written.append(path)
    return written


if __name__ == "__main__":
    main(sys.argv[1:])
