"""Train the 2D hand-pose machine (the reference's Hpm2d, networks/net_hpm2d.py) on prepared directories, on the device.

    python -m mmhand_amd.train_hpe --dataroot DIR --dataset rhd|stb [--extra_dataroot DIR ...] --name NAME
        [--checkpoints_dir ./checkpoints] [--batchSize 32] [--niter 100] [--niter_decay 100] [--lr 1e-4] [--beta1 0.9]
        [--sigma 5] [--stage_weights 1 1 1 1 1 1] [--init_from PTH | --init_seed N] [--val_dataroot DIR] [--save_epoch_freq 5]

`--extra_dataroot` (repeatable) adds prepared directories such as `aug --novel` output to the training list: the paper's
"real + generated" mix.  Images are read as `evaluate --pck_images` reads them (data._read_bgr, here on loader threads), go to
the device as bytes and through mmh_hpe_normalize; the labels are the directories' annotations.  The reference has the network
and the heat-map data mode (data/RHD_dataset.py:139-147,245-277) and no estimator training loop in its tree: the loss (the sum
over the six stage outputs of MSE against the sigma-5 Gaussian target), Adam and the defaults above are this port's recipe; the
learning rate follows the reference's linear rule (networks/networks.py:54-58).  `--val_dataroot` scores the current weights
after every epoch with hpe.HPEstimator (the 2D PCK figures of `evaluate --pck_images`).  Writes
<checkpoints_dir>/<name>/latest_net_Hpm2d.pth after every epoch and <epoch>_net_Hpm2d.pth every --save_epoch_freq epochs, in
the reference's keys: what `evaluate --pck --hpm2d` loads."""
import argparse
import json
import os
import random
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import hpe_train

# the widths --init_seed builds (the reference's: networks/net_hpm2d.py:40-67); tests narrow them
INIT_WIDTHS = hpe_train.FULL_WIDTHS


def build_parser():
    p = argparse.ArgumentParser(prog="python -m mmhand_amd.train_hpe", description=__doc__.split("\n\n")[0])
    p.add_argument("--dataroot", required=True, help="prepared RHD / STB directory (annotation.pickle + PNGs)")
    p.add_argument("--dataset", required=True, choices=["rhd", "stb"])
    p.add_argument("--extra_dataroot", action="append", default=[], metavar="DIR",
                   help="a further prepared directory of the same --dataset kind (repeatable), e.g. aug --novel output")
    p.add_argument("--name", required=True, help="experiment name: checkpoints go to <checkpoints_dir>/<name>")
    p.add_argument("--checkpoints_dir", default="./checkpoints")
    p.add_argument("--batchSize", type=int, default=32)
    p.add_argument("--niter", type=int, default=100, help="epochs at the initial learning rate")
    p.add_argument("--niter_decay", type=int, default=100, help="epochs over which the rate falls linearly to zero")
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--beta1", type=float, default=0.9)
    p.add_argument("--sigma", type=float, default=5.0, help="the target Gaussian's sigma in pixels (RHD_dataset.py:143)")
    p.add_argument("--stage_weights", type=float, nargs=hpe_train.N_OUT, default=[1.0] * hpe_train.N_OUT,
                   help="the weight of each of the six stage outputs' loss")
    p.add_argument("--init_from", default=None, help="start from this Hpm2d checkpoint")
    p.add_argument("--init_seed", type=int, default=None, help="start from torch's default nn.Conv2d initialisation under "
                                                               "this seed (default 0 when --init_from is not given)")
    p.add_argument("--val_dataroot", default=None, help="prepared directory scored with the current weights after every epoch")
    p.add_argument("--save_epoch_freq", type=int, default=5)
    p.add_argument("--seed", type=int, default=0, help="the seed of the epochs' shuffles")
    p.add_argument("--threads", type=int, default=8, help="image-reading threads")
    p.add_argument("--gpu", type=int, default=0)
    return p


def check_args(parser, a):
    if a.init_from is not None and a.init_seed is not None:
        parser.error("--init_from and --init_seed contradict each other: a run starts from a checkpoint or from a seed")
    if a.niter < 1 or a.niter_decay < 0:
        parser.error("--niter must be >= 1 and --niter_decay >= 0")
    if a.batchSize < 1 or a.save_epoch_freq < 1 or a.threads < 1:
        parser.error("--batchSize, --save_epoch_freq and --threads must be >= 1")
    if not (a.lr > 0 and 0 <= a.beta1 < 1 and a.sigma > 0):
        parser.error("--lr and --sigma must be positive and --beta1 in [0, 1)")
    if any(w < 0 for w in a.stage_weights) or not any(a.stage_weights):
        parser.error("--stage_weights: non-negative values, not all zero")
    roots = [a.dataroot] + a.extra_dataroot
    if len({os.path.abspath(r) for r in roots}) != len(roots):
        parser.error("--dataroot / --extra_dataroot name the same directory twice")
    if a.val_dataroot and os.path.abspath(a.val_dataroot) in {os.path.abspath(r) for r in roots}:
        parser.error("--val_dataroot is one of the training directories")


def _loader(root, a, dev):
    from .data import HandFolderLoader
    from .evaluate import _opt
    ns = types.SimpleNamespace(batchSize=a.batchSize, gpu=a.gpu, dataroot=root, dataset=a.dataset, augmentation_ratio=0.0)
    return HandFolderLoader(_opt(ns), device=dev)


def labelled_images(roots, a, dev):
    """[(path, uv float64 [21,2])] of every colour image the prepared directories list, in the loaders' order"""
    out = []
    for root in roots:
        loader = _loader(root, a, dev)
        out += [(p, np.asarray(loader.get_labels(p)["uv_coord"], dtype=np.float64).reshape(21, 2)) for p in loader._all_images]
    return out


def batches(items, batch, pool, dev):
    """-> (images uint8 [B,H,W,3] BGR on the device, uv [B,21,2]) per batch, the next batch's files being read meanwhile"""
    from .data import _read_bgr
    chunks = [items[i:i + batch] for i in range(0, len(items), batch)]
    pending = [pool.submit(_read_bgr, p) for p, _ in chunks[0]] if chunks else []
    for i, chunk in enumerate(chunks):
        imgs = [f.result() for f in pending]
        pending = [pool.submit(_read_bgr, p) for p, _ in chunks[i + 1]] if i + 1 < len(chunks) else []
        if any(im.shape != imgs[0].shape for im in imgs):
            raise SystemExit(f"train_hpe: images of different sizes in one batch ({chunk[0][0]} ...)")
        yield torch.from_numpy(np.stack(imgs)).to(dev), np.stack([uv for _, uv in chunk])


def validate(trainer, items, a, pool, dev):
    from .hpe import HPEstimator
    est = HPEstimator(trainer.inference_net(), None, device=dev)
    for images, uv in batches(items, a.batchSize, pool, dev):
        est.feed(images, uv, layout="bgr_hwc")
    m = est.results()["pck2d"]
    return {"pck2d_auc": m["auc"], "epe2d_mean": m["epe_mean"], "epe2d_median": m["epe_median"]}


def main(argv=None):
    parser = build_parser()
    a = parser.parse_args(argv)
    check_args(parser, a)
    torch.cuda.set_device(a.gpu)
    dev = torch.device("cuda", a.gpu)
    train = labelled_images([a.dataroot] + a.extra_dataroot, a, dev)
    if not train:
        raise SystemExit("train_hpe: no images")
    val = labelled_images([a.val_dataroot], a, dev) if a.val_dataroot else None
    trainer = hpe_train.Hpm2dTrainer(dev, lr=a.lr, beta1=a.beta1, sigma=a.sigma, stage_weights=a.stage_weights)
    if a.init_from is not None:
        trainer.load_state_dict(torch.load(a.init_from, map_location="cpu"))
    else:
        trainer.load_state_dict(hpe_train.init_state_dict(a.init_seed or 0, INIT_WIDTHS))
    out_dir = os.path.join(a.checkpoints_dir, a.name)
    os.makedirs(out_dir, exist_ok=True)
    rng, log = random.Random(a.seed), []
    with ThreadPoolExecutor(a.threads) as pool:
        for epoch in range(1, a.niter + a.niter_decay + 1):
            lr = hpe_train.linear_lr(a.lr, epoch - 1, a.niter, a.niter_decay)
            order = list(train)
            rng.shuffle(order)
            sums, n = torch.zeros(hpe_train.N_OUT, dtype=torch.float64, device=dev), 0
            for images, uv in batches(order, a.batchSize, pool, dev):
                sums += trainer.step(images, uv, layout="bgr_hwc", lr=lr) * images.shape[0]
                n += images.shape[0]
            row = {"epoch": epoch, "lr": lr, "images": n, "loss": (sums / n).tolist()}
            if val is not None:
                row.update(validate(trainer, val, a, pool, dev))
            print(json.dumps(row), flush=True)
            log.append(row)
            sd = trainer.state_dict()
            torch.save(sd, os.path.join(out_dir, "latest_net_Hpm2d.pth"))
            if epoch % a.save_epoch_freq == 0:
                torch.save(sd, os.path.join(out_dir, f"{epoch}_net_Hpm2d.pth"))
    with open(os.path.join(out_dir, "train_hpe_log.json"), "w") as fh:
        json.dump({"options": vars(a), "epochs": log}, fh, indent=1)
    return log


if __name__ == "__main__":
    main()
