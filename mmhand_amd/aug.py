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

`--depth_source files|joints [--render_radius R] [--render_bg Z]` (additions, first form): `joints` renders the depth conditions
D1 / D2 from the 3D joints on the device (ops.render_pose_depth) instead of reading depth PNGs - a prepared directory without
depth files works.
`--novel K [--novel_alpha A]` (additions, first form; K in 1 .. 15, A in (0, 1], default 0.5): images for poses that are NOT in
the dataset.  Every target t of the generation split is blended with each of its K nearest poses of the pool (`--match_pool
self|train`; ops.pose_knn, t excluded): uv = (1 - A) uv_t + A uv_nb, depth likewise (novel.py).  The source side H1 / P1 / D1 is
t's own image, pose and depth (D1 follows --depth_source); P2 is the pose maps of the new joints and D2 is ALWAYS rendered from
them, whatever --depth_source says - no file can exist for a new pose - so a checkpoint trained with `--depth_source files`
sees a rendered D2 it was not trained on.  The output is a prepared RHD directory: <dst>/color/<number>.png (consecutive,
five digits at least), <dst>/annotation.pickle with the new labels (uv_coord on the written image's grid, depth raw) and
<dst>/novel_index.json = [{file, target, neighbour, rank, alpha, pose_distance}]; `train --dataroot <dst> --dataset rhd
--depth_source joints` consumes it.  A target with fewer than K neighbours yields fewer images.  Composes with --batch,
--device_png and --resize_inputs; --pairing does not apply (the source is the target itself).

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

from . import novel, ops
from .data import MATCH_POOLS, PAIRINGS, HandFolderLoader, SyntheticHandLoader, png_size
from .inference import InferenceGenerator
from .networks import Generator
from .options import DEPTH_SOURCES, check_depth_source, check_resize_inputs, default_train_opt


def _target_path(dst, h2_path):
    # aug.py:66-71: <dst>/<folder of the target image>/<its file name>
    *_, folder, name = h2_path.split("/")
    os.makedirs(os.path.join(dst, folder), exist_ok=True)
    return os.path.join(dst, folder, name)


def _write_file(path, data):
    with open(path, "wb") as f:
        f.write(data)


def _paths_of_targets(dst):
    return lambda sample, first, n: [_target_path(dst, p) for p in sample["H2_path"][:n]]


def _novel_setup(loader, k, alpha, match_pool, dev):
    """plan the new poses (novel.plan on ops.pose_knn's neighbours) and point the loader at them: one position per record,
    source = target = the record's target image, in record order -> records"""
    pool = loader.match_pool_paths(match_pool)
    own = pool is loader.image_target
    with torch.cuda.device(dev):
        q = loader._features(loader.image_target)
        c = q if own else loader._features(pool)
        exclude = torch.arange(len(pool), dtype=torch.int32, device=dev) if own else None
        idx, dist = ops.pose_knn(q, c, k, exclude=exclude)
        idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    records, fallbacks = novel.plan(loader.image_target, pool, loader.get_labels, idx, dist, k, alpha)
    loader.novel_fallbacks = fallbacks
    loader.image_source = [r["target"] for r in records]
    loader.image_target = list(loader.image_source)
    loader.aug_item = np.arange(len(records), dtype=np.int64)
    loader._pair_distance = None
    return records


def _novel_samples(loader, records, dst, render, dev):
    """the loader's batches with the target side replaced by the new poses: P2 = their pose maps, D2 = their render, both on the
    batch's own grid; -> (samples, paths_of, sizes) where sizes collects (files' size, written size) of every record"""
    radius, bg = render
    sizes = []
    os.makedirs(os.path.join(dst, "color"), exist_ok=True)

    def samples():
        first = 0
        for sample in loader:
            n, (Ho, Wo) = sample["H1"].shape[0], sample["H1"].shape[2:]
            xyz = np.empty((n, 21, 3), np.float64)
            for j, r in enumerate(records[first:first + n]):
                src = png_size(r["target"]) or (Ho, Wo)
                sizes.append((src, (int(Ho), int(Wo))))
                xyz[j, :, :2] = novel.resize_uv(r["uv"], src, (int(Ho), int(Wo)))
                xyz[j, :, 2] = r["depth"] / 700.0 * 255
            xyz = torch.from_numpy(xyz).to(dev)
            sample = dict(sample)
            sample["P2"] = ops.pose_heatmaps(xyz[:, :, :2].reshape(n * 21, 2).contiguous(), int(Ho), int(Wo)).view(n, 21, Ho, Wo)
            sample["D2"] = ops.nhwc_to_nchw_view(ops.render_pose_depth(xyz, size=(int(Ho), int(Wo)), radius=radius, bg=bg), 3)
            sample["C2"] = xyz
            sample["_first"] = first
            first += n
            yield sample

    def paths_of(sample, first, n):
        return [os.path.join(dst, "color", r["file"]) for r in records[first:first + n]]
    return samples, paths_of, sizes


def _generate_device_png(loader, gen, dst, dev, threads, paths_of=None):
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
        paths_of = paths_of or _paths_of_targets(dst)
        for sample in loader:
            fake = gen([sample["H1"], torch.cat((sample["P1"], sample["P2"]), 1),
                        torch.cat((sample["D1"], sample["D2"]), 1)])
            img = ((fake.permute(0, 2, 3, 1) * 0.5 + 0.5) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
            paths = paths_of(sample, sample.get("_first", 0), img.shape[0])
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
    valued = {}
    for flag, conv in (("--depth_source", str), ("--render_radius", float), ("--render_bg", float), ("--novel", int),
                       ("--novel_alpha", float)):
        if flag in argv:
            i = argv.index(flag)
            try:
                valued[flag[2:]] = conv(argv[i + 1])
            except (IndexError, ValueError):
                raise ValueError(f"{flag}: expected {'a number' if conv is not str else 'a value'}") from None
            del argv[i:i + 2]
    if valued.get("depth_source", "files") not in DEPTH_SOURCES:
        raise ValueError(f"--depth_source: expected one of {' | '.join(DEPTH_SOURCES)}")
    if "novel_alpha" in valued and "novel" not in valued:
        raise ValueError("--novel_alpha belongs to --novel K")
    novel_k = novel_alpha = None
    if "novel" in valued:
        novel_k, novel_alpha = novel.check_novel(valued.pop("novel"), valued.pop("novel_alpha", 0.5))
    pair_flags = {}
    for flag, allowed in (("--pairing", PAIRINGS), ("--match_pool", MATCH_POOLS)):
        if flag in argv:
            i = argv.index(flag)
            if i + 1 >= len(argv) or argv[i + 1] not in allowed:
                raise ValueError(f"{flag}: expected one of {' | '.join(allowed)}")
            pair_flags[flag[2:]] = argv[i + 1]
            del argv[i:i + 2]
    if novel_k is not None and "pairing" in pair_flags:
        raise ValueError("--novel: the source of a new pose is its target's own image, --pairing does not apply "
                         "(--match_pool chooses the neighbours' pool)")
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
        if valued or novel_k is not None:
            raise ValueError("--depth_source / --render_radius / --render_bg / --novel belong to the prepared-directory form of "
                             "the command line")
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
        for name, value in list(pair_flags.items()) + list(valued.items()):
            if novel_k is None or name != "match_pool":     # --novel: the pool of the neighbours, not of a pairing
                setattr(opt, name, value)
        loader = HandFolderLoader(opt, device=dev, decoded=True)
    else:
        loader = SyntheticHandLoader(opt, n_batches * batch, size=size)
    os.makedirs(dst, exist_ok=True)
    paths_of, batches, finish = _paths_of_targets(dst), loader, None
    if novel_k is not None:
        records = _novel_setup(loader, novel_k, novel_alpha, pair_flags.get("match_pool", "self"), dev)
        # D2 is rendered whatever --depth_source says; --render_radius / --render_bg are validated either way
        check_depth_source(opt)
        render = (float(getattr(opt, "render_radius", 5.0)), float(getattr(opt, "render_bg", 255.0)))
        samples, paths_of, sizes = _novel_samples(loader, records, dst, render, dev)
        batches = samples()

        def finish():
            src, out = sizes[0] if sizes else (None, None)
            if any(s != sizes[0] for s in sizes):
                raise ValueError("--novel: the targets' files differ in size; the annotation has one grid")
            novel.write_annotation(dst, records, src, out)
            novel.write_index(dst, records, root=dataroot)
    if device_png:
        written = _generate_device_png(batches, gen, dst, dev, threads=16, paths_of=paths_of)
        if finish:
            finish()
        return written
    written = []
    for i, sample in enumerate(batches):
        fake = gen([sample["H1"], torch.cat((sample["P1"], sample["P2"]), 1),
                    torch.cat((sample["D1"], sample["D2"]), 1)])
        img = ((fake.permute(0, 2, 3, 1) * 0.5 + 0.5) * 255.0).round().clamp(0, 255).to(torch.uint8)
        arr = img.cpu().numpy()                                     # RGB, what the PNG stores
        out_paths = paths_of(sample, sample.get("_first", 0), arr.shape[0])
        for j in range(arr.shape[0]):
            path = out_paths[j]                                     # aug.py:66-71: <dst>/<folder of the target image>/<its file name>
            try:
                from PIL import Image
                Image.fromarray(arr[j]).save(path)
            except ImportError:
                path = os.path.splitext(path)[0] + ".npy"
                np.save(path, arr[j])
            written.append(path)
    if finish:
        finish()
    return written


if __name__ == "__main__":
    main(sys.argv[1:])
