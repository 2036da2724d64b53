"""Train a hand-pose machine (the reference's Hpm2d, networks/net_hpm2d.py, or Hpm3d, networks/net_hpm3d.py) on prepared
directories, on the device.

    python -m mmhand_amd.train_hpe --dataroot DIR --dataset rhd|stb [--extra_dataroot DIR ...] --name NAME [--net hpm2d|hpm3d]
        [--checkpoints_dir ./checkpoints] [--batchSize 32] [--niter 100] [--niter_decay 100] [--lr 1e-4] [--beta1 0.9]
        [--sigma 5] [--stage_weights 1 1 1 1 1 1] [--init_from PTH | --init_seed N] [--val_dataroot DIR] [--save_epoch_freq 5]
        [--smooth_l1_beta 1.0] [--loss_scale 10] [--heat_source target|predicted] [--hpm2d PTH]
        [--augment_geom [--aug_rotate 15] [--aug_scale 0.1] [--aug_shift 0.05] [--aug_flip 0]] [--aug_seed 0]
        [--augment_color [--aug_saturation 0.3] [--aug_hue 10] [--aug_gain 0.1] [--aug_gamma 0.2]]

`--extra_dataroot` (repeatable) adds prepared directories such as `aug --novel` output to the training list: the paper's
"real + generated" mix.  The labels are the directories' annotations; the learning rate follows the reference's linear rule
(networks/networks.py:54-58).  The reference trains both networks under hand_pose_estimators/CVPR2020_hpm3d/models/
(hpm2d_model.py, hpm3d_model.py, hpm_model.py) with Adam at `--lr 2e-4 --beta1 0.5` (options/train_options.py:31-37,
models/networks/__init__.py:72).  The parse-time defaults `--lr 1e-4 --beta1 0.9` are this port's, for either net: pass the
reference's values to train as it does.

`--net hpm2d` (the default).  Images are read as `evaluate --pck_images` reads them (data._read_bgr, here on loader threads), go
to the device as bytes and through mmh_hpe_normalize (mmh_hpe_augment_normalize under the augmentation flags, below).  The loss is the sum over the six stage outputs of --stage_weights[s] times
the MSE against the sigma-5 Gaussian target; the reference's own (hpm2d_model.py:143-151) is that sum times 1000 =
`--stage_weights 1000 1000 1000 1000 1000 1000`; the default weights of 1 are this port's.  `--val_dataroot` scores the current
weights after every epoch with hpe.HPEstimator (the 2D PCK figures of `evaluate --pck_images`).  Writes
<checkpoints_dir>/<name>/latest_net_Hpm2d.pth after every epoch and <epoch>_net_Hpm2d.pth every --save_epoch_freq epochs, in
the reference's keys: what `evaluate --pck --hpm2d` loads.

`--net hpm3d`.  The reference's recipe (hpm3d_model.py:73,91-113): the input is the 21 ground-truth Gaussian maps, the target the
labels' depth, the loss nn.SmoothL1Loss() (--smooth_l1_beta) times --loss_scale; train as the reference does with
`--lr 2e-4 --beta1 0.5`.  `--heat_source target` (the default, the reference's) renders the maps from the labels on the device
(mmh_gauss_heatmaps) and reads no image file; `--heat_source predicted --hpm2d PTH` reads the images and feeds
ops.heatmap_upsample_argmax(Hpm2d(normalised image)), the distribution `evaluate --pck` hands the network.  The target is the
label's depth times hpe.Z_SCALE[dataset] / 256 - the depth itself for rhd, depth / 700 for stb - so that the evaluator's
output * H against depth * z_scale (hpe.py: HPEstimator.distances) compares like with like.  [The reference's STB loader hands
the raw depth over as the training target while its evaluator compares output * 256 with depth / 700 * 256: the two disagree
by the factor 700; this port trains what its evaluator scores.]  `--val_dataroot` logs the validation loss `val_L_z` and, with
--hpm2d, `pck3d_auc` / `epe3d_mean` of hpe.HPEstimator(hpm2d, the current weights).  --init_seed sizes depth_fc_1 for the first
training image (height / 8; square, a multiple of 8).  --batchSize is at most 64 (the Linear kernels' rows); --stage_weights
does not apply.  Writes latest_net_Hpm3d.pth / <epoch>_net_Hpm3d.pth, the names the reference's evaluator loads and what
`evaluate --pck --hpm3d` takes.

`--augment_geom` / `--augment_color` (additions; off: every epoch shows the network the files' pixels, as the reference does):
conventional augmentation of the TRAINING images, the row a "real + generated" table is compared with.  Per epoch and item - an
item's number is its position in the training list before the epoch's shuffle - the host draws a rotation, scale, shift (and
flip) from (aug_seed, epoch) (data.augment_draws, side 0; the names, defaults and checks of `train`) and a saturation, hue,
three channel gains and a gamma from a stream of their own (data.color_draws), so either switch leaves the other's draws as
they are.  The images go through ops.hpe_augment_normalize instead of ops.hpe_normalize - one fused pass that warps, applies
the colour matrix and the gamma curve and takes the min-max normalisation after them (it would cancel a plain brightness or
contrast change) - and the joints through data.affine_joints, so the targets the device builds from them follow the warp.
`--net hpm3d --heat_source target` has no image: --augment_geom moves the joints its maps are rendered from and
--augment_color is refused; with `--heat_source predicted` the augmented images feed --hpm2d and the depth labels stay (a 2D
warp).  Validation is never augmented."""
import argparse
import json
import os
import random
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import hpe_train

# the widths --init_seed builds (the reference's: networks/net_hpm2d.py:40-67, net_hpm3d.py:29-64); tests narrow them
INIT_WIDTHS = hpe_train.FULL_WIDTHS


# (flag, default, help) of the ranges behind each switch; the geometric ones are `train`'s (options.py)
GEOM_FLAGS = [("aug_rotate", 15.0, "with --augment_geom: degrees, theta ~ U(-r, r)"),
              ("aug_scale", 0.1, "with --augment_geom: s ~ U(1 - a, 1 + a), 0 <= a < 1"),
              ("aug_shift", 0.05, "with --augment_geom: shift ~ U(-f, f) of the image size, per axis"),
              ("aug_flip", 0.0, "with --augment_geom: probability of a horizontal flip (a mirrored hand is the other hand)")]
COLOR_FLAGS = [("aug_saturation", 0.3, "with --augment_color: s ~ U(1 - a, 1 + a), clipped at 0"),
               ("aug_hue", 10.0, "with --augment_color: degrees about the grey axis, h ~ U(-d, d)"),
               ("aug_gain", 0.1, "with --augment_color: per channel, gain ~ U(1 - g, 1 + g)"),
               ("aug_gamma", 0.2, "with --augment_color: gamma = exp(U(-q, q))")]


def build_parser():
    p = argparse.ArgumentParser(prog="python -m mmhand_amd.train_hpe", description=__doc__.split("\n\n")[0])
    p.add_argument("--dataroot", required=True, help="prepared RHD / STB directory (annotation.pickle + PNGs)")
    p.add_argument("--dataset", required=True, choices=["rhd", "stb"])
    p.add_argument("--extra_dataroot", action="append", default=[], metavar="DIR",
                   help="a further prepared directory of the same --dataset kind (repeatable), e.g. aug --novel output")
    p.add_argument("--name", required=True, help="experiment name: checkpoints go to <checkpoints_dir>/<name>")
    p.add_argument("--net", default="hpm2d", choices=["hpm2d", "hpm3d"], help="which estimator to train")
    p.add_argument("--checkpoints_dir", default="./checkpoints")
    p.add_argument("--batchSize", type=int, default=32)
    p.add_argument("--niter", type=int, default=100, help="epochs at the initial learning rate")
    p.add_argument("--niter_decay", type=int, default=100, help="epochs over which the rate falls linearly to zero")
    p.add_argument("--lr", type=float, default=1e-4, help="the reference trains both nets at 2e-4")
    p.add_argument("--beta1", type=float, default=0.9, help="the reference trains both nets at 0.5")
    p.add_argument("--sigma", type=float, default=5.0, help="the target Gaussian's sigma in pixels (RHD_dataset.py:143)")
    p.add_argument("--stage_weights", type=float, nargs=hpe_train.N_OUT, default=[1.0] * hpe_train.N_OUT,
                   help="hpm2d: the weight of each of the six stage outputs' loss (the reference: 1000 each)")
    p.add_argument("--smooth_l1_beta", type=float, default=1.0, help="hpm3d: nn.SmoothL1Loss's beta")
    p.add_argument("--loss_scale", type=float, default=10.0, help="hpm3d: the factor on the loss (hpm3d_model.py:105)")
    p.add_argument("--heat_source", default="target", choices=["target", "predicted"],
                   help="hpm3d: the input maps - rendered from the labels (the reference's recipe; no image is read) or predicted "
                        "by --hpm2d from the images")
    p.add_argument("--hpm2d", default=None, help="hpm3d: an Hpm2d checkpoint, for --heat_source predicted and the validation's PCK")
    p.add_argument("--init_from", default=None, help="start from this checkpoint of the --net kind")
    p.add_argument("--init_seed", type=int, default=None, help="start from torch's default nn.Conv2d / nn.Linear initialisation "
                                                               "under this seed (default 0 when --init_from is not given)")
    p.add_argument("--val_dataroot", default=None, help="prepared directory scored with the current weights after every epoch")
    p.add_argument("--save_epoch_freq", type=int, default=5)
    p.add_argument("--augment_geom", action="store_true",
                   help="a random rotation, scale, shift (and flip) per training image and epoch, inside the normalisation pass "
                        "(mmh_hpe_augment_normalize; bilinear, edge replicate); the joints follow")
    for flag, default, text in GEOM_FLAGS + COLOR_FLAGS:
        p.add_argument("--" + flag, type=float, default=None, help=f"{text} (default {default})")
    p.add_argument("--augment_color", action="store_true",
                   help="a random saturation, hue, gain per channel and gamma per training image and epoch, in the same pass; the "
                        "min-max normalisation is taken after them")
    p.add_argument("--aug_seed", type=int, default=None, help="with --augment_geom / --augment_color: seed of the draws (with "
                                                              "the epoch number; default 0)")
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
    if a.net == "hpm3d":
        if a.batchSize > 64:
            parser.error("--net hpm3d: --batchSize is at most 64 (the rows of the Linear kernels)")
        if a.stage_weights != [1.0] * hpe_train.N_OUT:
            parser.error("--net hpm3d: --stage_weights does not apply (one output is supervised)")
        if not (a.smooth_l1_beta > 0 and np.isfinite(a.smooth_l1_beta) and a.loss_scale > 0 and np.isfinite(a.loss_scale)):
            parser.error("--smooth_l1_beta and --loss_scale must be positive and finite")
        if a.heat_source == "predicted" and not a.hpm2d:
            parser.error("--heat_source predicted needs --hpm2d <checkpoint of the 2D hand-pose machine>")
    elif a.hpm2d or a.heat_source != "target" or a.smooth_l1_beta != 1.0 or a.loss_scale != 10.0:
        parser.error("--hpm2d, --heat_source, --smooth_l1_beta and --loss_scale belong to --net hpm3d")
    check_augment_args(parser, a)


def check_augment_args(parser, a):
    """the augmentation flags: a range without its switch is an error; the defaults are filled in (they land in the log)"""
    from .options import check_augment, check_augment_color
    for switch, flags in (("augment_geom", GEOM_FLAGS), ("augment_color", COLOR_FLAGS)):
        for flag, default, _ in flags:
            if getattr(a, flag) is None:
                setattr(a, flag, default)
            elif not getattr(a, switch):
                parser.error(f"--{flag} does nothing without --{switch}")
    if a.aug_seed is None:
        a.aug_seed = 0
    elif not (a.augment_geom or a.augment_color):
        parser.error("--aug_seed does nothing without --augment_geom or --augment_color")
    if a.augment_color and a.net == "hpm3d" and a.heat_source == "target":
        parser.error("--augment_color: --net hpm3d --heat_source target reads no image (its maps are rendered from the joints)")
    try:
        check_augment(a)
        check_augment_color(a)
    except ValueError as e:
        parser.error(str(e))


def _loader(root, a, dev):
    from .data import HandFolderLoader
    from .evaluate import _opt
    ns = types.SimpleNamespace(batchSize=a.batchSize, gpu=a.gpu, dataroot=root, dataset=a.dataset, augmentation_ratio=0.0)
    return HandFolderLoader(_opt(ns), device=dev)


def labelled_images(roots, a, dev, with_depth=False):
    """[(path, uv float64 [21,2])] of every colour image the prepared directories list, in the loaders' order; with_depth:
    [(path, uv, depth float64 [21])]"""
    out = []
    for root in roots:
        loader = _loader(root, a, dev)
        for p in loader._all_images:
            lab = loader.get_labels(p)
            item = (p, np.asarray(lab["uv_coord"], dtype=np.float64).reshape(21, 2))
            out.append(item + (np.asarray(lab["depth"], dtype=np.float64).reshape(21),) if with_depth else item)
    return out


class Augment:
    """--augment_geom / --augment_color for the training list of `n_items`: one epoch's draws for every item (set_epoch), applied
    to a batch by the items' numbers - what an image gets depends on (aug_seed, epoch, item) and on nothing else"""

    def __init__(self, a, n_items):
        self.a, self.n = a, int(n_items)
        self.geom = self.color = None

    @classmethod
    def of(cls, a, n_items):
        return cls(a, n_items) if a.augment_geom or a.augment_color else None

    def set_epoch(self, epoch):
        from .data import augment_draws, color_draws
        self.geom = augment_draws(self.n, epoch, self.a)[:, 0] if self.a.augment_geom else None      # side 0
        self.color = color_draws(self.n, epoch, self.a) if self.a.augment_color else None

    def forward_maps(self, ids, src):
        """-> the forward matrices float64 [B,2,3] of these items on the src = (H, W) grid, or None without --augment_geom"""
        from .data import affine_forward
        if self.geom is None:
            return None
        d = self.geom[np.asarray(ids, dtype=np.int64)]
        return affine_forward(d[:, 0], d[:, 1], d[:, 2], d[:, 3], d[:, 4], src)

    def joints(self, uv, ids, src):
        """uv [B,21,2] of the files -> on the warped images"""
        from .data import affine_joints
        fwd = self.forward_maps(ids, src)
        return uv if fwd is None else affine_joints(uv, fwd, src)

    def normalize(self, images, ids):
        """images uint8 [B,H,W,3] BGR on the device -> the estimators' input fp32 [B,H,W,4] (ops.hpe_augment_normalize)"""
        from . import ops
        from .data import affine_inverse, color_matrix
        src, dev = tuple(images.shape[1:3]), images.device
        fwd = self.forward_maps(ids, src)
        xf = cm = gamma = None
        if fwd is not None:
            xf = torch.from_numpy(affine_inverse(fwd, src).reshape(-1, 6)).to(dev)
        if self.color is not None:
            c = self.color[np.asarray(ids, dtype=np.int64)]
            cm = torch.from_numpy(color_matrix(c[:, 0], c[:, 1], c[:, 2:5]).reshape(-1, 9)).to(dev)
            gamma = torch.from_numpy(np.ascontiguousarray(c[:, 5])).to(dev)
        return ops.hpe_augment_normalize(images, xf, cm, gamma)


def batches(items, batch, pool, dev, ids=None):
    """-> (images uint8 [B,H,W,3] BGR on the device, uv [B,21,2]) per batch, the next batch's files being read meanwhile; with
    `ids` (one number per item, for Augment) -> (images, uv, the batch's numbers)"""
    from .data import _read_bgr
    chunks = [items[i:i + batch] for i in range(0, len(items), batch)]
    pending = [pool.submit(_read_bgr, it[0]) for it in chunks[0]] if chunks else []
    for i, chunk in enumerate(chunks):
        imgs = [f.result() for f in pending]
        pending = [pool.submit(_read_bgr, it[0]) for it in chunks[i + 1]] if i + 1 < len(chunks) else []
        if any(im.shape != imgs[0].shape for im in imgs):
            raise SystemExit(f"train_hpe: images of different sizes in one batch ({chunk[0][0]} ...)")
        out = torch.from_numpy(np.stack(imgs)).to(dev), np.stack([it[1] for it in chunk])
        yield out if ids is None else out + (list(ids[i * batch:(i + 1) * batch]),)


def validate(trainer, items, a, pool, dev):
    from .hpe import HPEstimator
    est = HPEstimator(trainer.inference_net(), None, device=dev)
    for images, uv in batches(items, a.batchSize, pool, dev):
        est.feed(images, uv, layout="bgr_hwc")
    m = est.results()["pck2d"]
    return {"pck2d_auc": m["auc"], "epe2d_mean": m["epe_mean"], "epe2d_median": m["epe_median"]}


# ------------------------------------------------------------------------------------------------- --net hpm3d
def batches_3d(items, a, pool, dev, hpm2d, aug=None, ids=None, size=None):
    """-> (the network's input: uv [B,21,2] under --heat_source target - no file is opened - or the 2D machine's upsampled maps
    fp32 [B,H,W,24]; the target depths [B,21]; the images or None) per batch.  aug (an Augment, with the items' numbers `ids`):
    the training epoch's augmentation - the joints moved on the size x size grid, or the images in front of the 2D machine"""
    from . import hpe, ops
    zs = hpe.Z_SCALE[a.dataset] / 256.0
    if a.heat_source == "target":
        for i in range(0, len(items), a.batchSize):
            chunk = items[i:i + a.batchSize]
            uv = np.stack([it[1] for it in chunk])
            if aug is not None:
                uv = aug.joints(uv, ids[i:i + a.batchSize], (size, size))
            yield uv, np.stack([it[2] for it in chunk]) * zs, None
        return
    at = 0
    for images, _ in batches(items, a.batchSize, pool, dev):
        chunk = items[at:at + images.shape[0]]
        with torch.no_grad():
            x = ops.hpe_normalize(images, "bgr_hwc") if aug is None else aug.normalize(images, ids[at:at + images.shape[0]])
            up = ops.heatmap_upsample_argmax(hpm2d(x))[0]
        at += images.shape[0]
        yield up, np.stack([it[2] for it in chunk]) * zs, images


def validate_3d(trainer, items, a, pool, dev, hpm2d):
    from . import hpe
    total, n = torch.zeros(1, dtype=torch.float64, device=dev), 0
    for x, z, _ in batches_3d(items, a, pool, dev, hpm2d):
        trainer.forward(trainer.heatmaps(x) if a.heat_source == "target" else x)
        total += trainer.loss(z, with_grad=False)[0] * len(z)
        n += len(z)
    row = {"val_L_z": float(total / n)}
    if hpm2d is not None:
        est = hpe.HPEstimator(hpm2d, trainer.inference_net(), device=dev, z_scale=hpe.Z_SCALE[a.dataset])
        at = 0
        for images, uv in batches(items, a.batchSize, pool, dev):
            est.feed(images, uv, np.stack([it[2] for it in items[at:at + len(uv)]]), layout="bgr_hwc")
            at += len(uv)
        res = est.results()
        row.update(pck2d_auc=res["pck2d"]["auc"], pck3d_auc=res["pck3d"]["auc"], epe3d_mean=res["pck3d"]["epe_mean"],
                   epe3d_median=res["pck3d"]["epe_median"])
    return row


def _head_hw(path):
    from .data import png_size
    size = png_size(path)
    if size is None or size[0] != size[1] or size[0] % 8 or size[0] < 8:
        raise SystemExit(f"train_hpe --net hpm3d: {path} is {size}: depth_fc_1 needs square images whose side is a multiple of 8")
    return size[0] // 8


def main_3d(a):
    from . import hpe
    torch.cuda.set_device(a.gpu)
    dev = torch.device("cuda", a.gpu)
    train = labelled_images([a.dataroot] + a.extra_dataroot, a, dev, with_depth=True)
    if not train:
        raise SystemExit("train_hpe: no images")
    val = labelled_images([a.val_dataroot], a, dev, with_depth=True) if a.val_dataroot else None
    hpm2d = hpe.Hpm2d(dev).load_state_dict(torch.load(a.hpm2d, map_location="cpu")) if a.hpm2d else None
    trainer = hpe_train.Hpm3dTrainer(dev, lr=a.lr, beta1=a.beta1, sigma=a.sigma, beta=a.smooth_l1_beta, scale=a.loss_scale)
    head_hw = _head_hw(train[0][0])
    if a.init_from is not None:
        trainer.load_state_dict(torch.load(a.init_from, map_location="cpu"))
        if trainer.head_hw != head_hw:
            raise SystemExit(f"train_hpe: {a.init_from} is sized for {trainer.head_hw * 8}^2 images, {train[0][0]} is "
                             f"{head_hw * 8}^2")
    else:
        trainer.load_state_dict(hpe_train.init_state_dict_3d(a.init_seed or 0, INIT_WIDTHS, head_hw))
    out_dir = os.path.join(a.checkpoints_dir, a.name)
    os.makedirs(out_dir, exist_ok=True)
    rng, log, aug = random.Random(a.seed), [], Augment.of(a, len(train))
    with ThreadPoolExecutor(a.threads) as pool:
        for epoch in range(1, a.niter + a.niter_decay + 1):
            lr = hpe_train.linear_lr(a.lr, epoch - 1, a.niter, a.niter_decay)
            ids = list(range(len(train)))
            rng.shuffle(ids)                                        # the permutation list(train) would get
            order = [train[i] for i in ids]
            if aug is not None:
                aug.set_epoch(epoch)
            total, n = torch.zeros(1, dtype=torch.float64, device=dev), 0
            for x, z, _ in batches_3d(order, a, pool, dev, hpm2d, aug, ids, head_hw * 8):
                total += trainer.step(x, z, lr=lr) * len(z)
                n += len(z)
            row = {"epoch": epoch, "lr": lr, "images": n, "loss": float(total / n)}
            if val is not None:
                row.update(validate_3d(trainer, val, a, pool, dev, hpm2d))
            print(json.dumps(row), flush=True)
            log.append(row)
            sd = trainer.state_dict()
            torch.save(sd, os.path.join(out_dir, "latest_net_Hpm3d.pth"))
            if epoch % a.save_epoch_freq == 0:
                torch.save(sd, os.path.join(out_dir, f"{epoch}_net_Hpm3d.pth"))
    with open(os.path.join(out_dir, "train_hpe_log.json"), "w") as fh:
        json.dump({"options": vars(a), "epochs": log}, fh, indent=1)
    return log


def main(argv=None):
    parser = build_parser()
    a = parser.parse_args(argv)
    check_args(parser, a)
    if a.net == "hpm3d":
        return main_3d(a)
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
    rng, log, aug = random.Random(a.seed), [], Augment.of(a, len(train))
    with ThreadPoolExecutor(a.threads) as pool:
        for epoch in range(1, a.niter + a.niter_decay + 1):
            lr = hpe_train.linear_lr(a.lr, epoch - 1, a.niter, a.niter_decay)
            ids = list(range(len(train)))
            rng.shuffle(ids)                                        # the permutation list(train) would get
            order = [train[i] for i in ids]
            sums, n = torch.zeros(hpe_train.N_OUT, dtype=torch.float64, device=dev), 0
            if aug is None:
                for images, uv in batches(order, a.batchSize, pool, dev):
                    sums += trainer.step(images, uv, layout="bgr_hwc", lr=lr) * images.shape[0]
                    n += images.shape[0]
            else:
                aug.set_epoch(epoch)
                for images, uv, which in batches(order, a.batchSize, pool, dev, ids):
                    x = aug.normalize(images, which)
                    sums += trainer.step_normalized(x, aug.joints(uv, which, tuple(images.shape[1:3])), lr=lr) * images.shape[0]
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
