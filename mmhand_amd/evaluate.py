"""Scores generated hand images on a held-out split: per-image SSIM (the reference Evaluator's metric, utils.py:100-111),
L1 and PSNR, all on images mapped to [0, 1] (generator output (x + 1) / 2, PNG pixels u8 / 255; see mmhand_amd/metrics.py).

Generator mode - runs a checkpoint over the generation split of a prepared directory (the pairs aug.py generates) and
scores each output against its target image H2:

    python -m mmhand_amd.evaluate --name CKP [--checkpoints_dir checkpoints] [--which_epoch latest] --dataroot DIR
        --dataset rhd|stb [--augmentation_ratio R] [--batchSize 16] [--bf16] [--gpu 0] [--window 11]
        [--resize_inputs N] [--pairing P [--match_pool M]] [--depth_source files|joints [--render_radius R] [--render_bg Z]]
        [--ms_ssim] [--hand_region [--hand_radius R]] [--results_json PATH] [--per_image_csv PATH]

Directory mode - scores the PNGs aug.py wrote (<DIR>/<folder of the target>/<name>) against the target colour PNGs:

    python -m mmhand_amd.evaluate --generated DIR --dataroot DIR --dataset rhd|stb [--augmentation_ratio R] ...

`--resize_inputs N`: the pairs are decoded to N x N inside the device's decode pass (ops.decode_inputs; what `train` and `aug`
do under the same flag); directory mode then expects N x N PNGs and scores them against the targets decoded at that size.

`--pairing random|curriculum|nearest [--match_pool self|train]`: the loader's pairing (data.HandFolderLoader; what `aug` does
under the same flags).  SSIM, L1 and PSNR of a generated image depend strongly on how far the source pose is from the target
pose; with the flag given the results JSON also carries `pairing` and `pose_distance_avg` (the reference's pose distance,
nearest_neighbor_search.py:68-83, mean over the scored pairs) and the per-image CSV a `pose_distance` column.  Without the
flag both files are what they were.

Both print one summary line (SSIM_avg, SSIM_std, L1_avg, PSNR_avg, n) and write it with the options used as JSON.

`--pck --hpm2d <pth> [--hpm3d <pth>] [--pck_max 30] [--pck_steps 20]`: also the reference Evaluator's pose metric (utils.py:71-78,
hpe_estimator.py:97-143; mmhand_amd/hpe.py): every scored image goes to the 2D hand-pose machine on the device and its joints
are compared with the TARGET pose's labels - `pck2d_auc`, `epe2d_mean`, `epe2d_median`, `pck2d_curve` and, with `--hpm3d`, the
same for 3D - in the summary, `epe2d` [, `epe3d`] columns in the per-image CSV.  Without `--pck` nothing of it is launched and
both files are what they were.

PCK-only mode - the colour images of a prepared directory against that directory's own labels; no generator, no pairs, no
SSIM.  This scores `aug --novel` output (a prepared directory with annotation.pickle) and gives the estimator's own PCK on
real images, the ceiling of the generated ones:

    python -m mmhand_amd.evaluate --pck_images DIR --dataset rhd|stb --hpm2d <pth> [--hpm3d <pth>] [--batchSize 16] ...

The reference ships no estimator weights: a PCK figure means what its --hpm2d / --hpm3d checkpoints mean.

`--inception <pth> [--is_group 64]`: also the reference Evaluator's Inception score (utils.py:81-98,196-232; mmhand_amd/
inception.py): every scored image becomes the bytes `aug` writes for it, is resized to 299 as PIL resizes and goes through
Inception-v3 on the device; the logits are scored in consecutive groups of --is_group images (a tail group on its own) -
`IS_avg`, `IS_std` (the reference's keys: mean and standard deviation over the groups), `IS_all` (one group over every image)
and `is_groups` in the summary, an `is_kl` column in the per-image CSV.  <pth> is torchvision's inception_v3_google state dict.
Without `--inception` nothing of it is launched and both files are what they were.

IS-only mode - every PNG below a directory, no labels, no pairs; on real images this is the ceiling row of the paper's table:

    python -m mmhand_amd.evaluate --is_images DIR --inception <pth> [--is_group 64] [--batchSize 16] ...

No Inception weights ship with this repository or the reference: a score means what its --inception file means.

`--fid <pth> [--fid_variant torchvision|fid] [--fid_real DIR|stats.npz] [--fid_stats_out PATH] [--kid_subsets 100]
[--kid_subset_size 1000] [--kid_seed 0]`: also the Frechet Inception Distance (pytorch-fid's definition) and the Kernel Inception
Distance (torch-fidelity's) of the scored images against real ones (mmhand_amd/fid.py): the pooled 2048 features of both sets
stay on the device, their means and covariances and the polynomial-kernel sums are taken there, the matrix square root's
trace on the host - `FID`, `KID_mean`, `KID_std` (over --kid_subsets random subsets of --kid_subset_size images, clamped to the
smaller set), `KID_full` (one estimate over all images), `n_real`, `n_generated`, `fid_variant` in the summary; no per-image
column.  The real set is the split's own target images unless --fid_real names a directory of PNGs or a statistics file (an
.npz with pytorch-fid's mu / sigma; KID is null when it holds no features); --fid_stats_out writes the real set's statistics.
--fid_variant fid: pytorch-fid's graph for its pt_inception-2015-12-05 weights (the resize stays PIL's).  With
--inception on the same file and graph one forward serves both.  With fewer images than features FID is biased and a warning
says so: KID is the figure to read.  Without `--fid` nothing of it is imported or launched and the files are what they were.

Two-directory mode - any two sets of PNGs, no labels; this scores `aug --novel` output against real images:

    python -m mmhand_amd.evaluate --fid_images DIR --fid_real DIR|stats.npz --fid <pth> [--fid_variant V] [--batchSize 16] ...

`--lpips <pth> --lpips_lin <pth>|uniform`: also LPIPS, the learned perceptual distance (the `lpips` package's LPIPS(net="vgg");
mmhand_amd/lpips.py) of every scored image against its target: both go through a VGG-16 trunk on the device and the five
taps' normalised, weighted squared differences are averaged there - `LPIPS_avg`, `LPIPS_layers` (the five taps' means) and
`lpips_lin` in the summary, a `lpips` column in the per-image CSV.  <pth> is torchvision's VGG-16 state dict; --lpips_lin names
the package's linear heads (weights/v0.1/vgg.pth) or `uniform` for the unweighted form (the package's lpips=False).  The image
size must be a multiple of 16.  Under --resize_inputs N the target is the decode pass's N x N image, as for SSIM.  AlexNet-LPIPS
is not offered (its stride-4 convolution has no kernel here).  Without `--lpips` nothing of it is imported or launched and the
files are what they were.

Two-directory mode - two directories of PNGs paired by relative file name, no labels; an unpaired file is an error:

    python -m mmhand_amd.evaluate --lpips_images DIR --lpips_ref DIR --lpips <pth> --lpips_lin <pth>|uniform [--batchSize 16] ...

No VGG-16 or LPIPS weights ship with this repository or the reference: a distance means what its files mean.

`--ms_ssim`: also multi-scale SSIM (Wang, Simoncelli, Bovik 2003; mmhand_amd/metrics.py ms_ssim, mmh_ms_ssim) of the pair SSIM
scores, with --window: five scales with the paper's weights, the contrast-structure term of the first four and the SSIM of the
last, each over the pixels whose window lies inside the image, 2 x 2 average pooling in between - `MS_SSIM_avg`, `MS_SSIM_std`
and `ms_weights` in the summary, an `ms_ssim` column in the per-image CSV.  The image's smaller side must exceed
(window - 1) * 16 (160 at the default window); a smaller image ends the run before anything is scored (see --resize_inputs).

`--hand_region [--hand_radius R]`: also SSIM, L1 and PSNR over the hand alone.  About a quarter of a frame lies under a bone;
the rest is background the generator mostly carries over, and it dominates the whole-image figures.  The region is the coverage
of the TARGET pose's 20 bones drawn as capsules of R pixels of the scored grid (ops.render_pose_depth on the labels' joints, at
the files' size or on the --resize_inputs grid); R defaults to 10 * H / 256, a definition and not a tuned value - capsules of
that radius leave gaps in the palm between the metacarpals, a larger R closes them.  The same SSIM map, |a-b| and (a-b)^2 as the
whole-image figures, averaged over the region, from the same pass (mmh_image_metrics_masked) - `SSIM_hand_avg`, `SSIM_hand_std`,
`L1_hand_avg`, `PSNR_hand_avg`, `hand_fraction_avg` (region pixels / (H W)), all over the `n_hand` images whose region is not
empty, and `hand_radius` in the summary; `ssim_hand`, `l1_hand`, `psnr_hand`, `hand_fraction` columns in the per-image CSV.  The
name is "hand", not "mask-SSIM", on purpose: PATN's mask-SSIM multiplies both images by the mask before scoring the whole
frame, which this does not.

Both flags apply to generator and directory mode alike.  Without them nothing of this is launched and both files are what they
were."""
import argparse
import csv
import json
import os
import re
import sys

import numpy as np
import torch

from .metrics import QualityMeter

DOMAIN = ("Both images are mapped to [0, 1] before scoring: generator output (x + 1) / 2, PNG pixels u8 / 255 - the range "
          "a written PNG represents, so scoring the generator's tensors and scoring aug.py's PNGs agree up to quantisation.")


def build_parser():
    p = argparse.ArgumentParser(prog="python -m mmhand_amd.evaluate", description=__doc__.split("\n\n")[0] + "  " + DOMAIN,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--name", help="checkpoint name: <checkpoints_dir>/<name>/<which_epoch>_net_netG.pth")
    src.add_argument("--generated", help="directory of aug.py's output PNGs, scored instead of running a generator")
    src.add_argument("--pck_images", help="prepared directory whose colour images are scored against its own labels: PCK only")
    src.add_argument("--is_images", help="directory whose PNGs (at any depth) get an Inception score: no labels, IS only")
    src.add_argument("--fid_images", help="directory whose PNGs (at any depth) are scored against --fid_real: FID / KID only")
    src.add_argument("--lpips_images", help="directory whose PNGs are scored against the same names below --lpips_ref: LPIPS only")
    p.add_argument("--checkpoints_dir", default="checkpoints")
    p.add_argument("--which_epoch", default="latest")
    p.add_argument("--dataroot", default=None, help="prepared RHD / STB directory (annotation.pickle + PNGs); required except "
                                                    "with --pck_images")
    p.add_argument("--dataset", default=None, choices=("rhd", "stb"), help="required except with --is_images")
    p.add_argument("--augmentation_ratio", type=float, default=None,
                   help="the generation split is the first (1 - ratio) share; a root with 'test' in its path serves all")
    p.add_argument("--batchSize", type=int, default=16)
    p.add_argument("--bf16", action="store_true", help="the generator's 16-bit (bf16 MFMA) inference mode")
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--device_png", action="store_true", help="decode the dataset's PNGs on the device (= MMH_DEVICE_PNG=1)")
    p.add_argument("--resize_inputs", type=int, default=0,
                   help="score at N x N: the dataset's images resized inside the device's decode pass (0 = the files' size)")
    p.add_argument("--pairing", default=None, choices=("random", "curriculum", "nearest"),
                   help="how a target gets its source (as aug's flag); given, the outputs also report the pairs' pose distance")
    p.add_argument("--match_pool", default=None, choices=("self", "train"), help="with --pairing nearest: the sources' pool")
    p.add_argument("--depth_source", default="files", choices=("files", "joints"),
                   help="joints: the depth conditions are rendered from the 3D joints on the device (as train's and aug's flag); "
                        "no depth PNG is opened")
    p.add_argument("--render_radius", type=float, default=5.0, help="with --depth_source joints: half-width of a bone, pixels")
    p.add_argument("--render_bg", type=float, default=255.0, help="with --depth_source joints: depth where no bone covers")
    p.add_argument("--window", type=int, default=11, help="SSIM window, odd, 3 .. 15 (the reference's default 11)")
    p.add_argument("--results_json", default=None,
                   help="default: <checkpoints_dir>/<name>/eval_<which_epoch>_<dataset>.json, or <generated>/eval_<dataset>.json")
    p.add_argument("--per_image_csv", default=None, help="one row per target: target, source, ssim, l1, psnr")
    p.add_argument("--pck", action="store_true", help="also score the pose of every image with the hand-pose estimators")
    p.add_argument("--hpm2d", default=None, help="with --pck: the 2D hand-pose machine's checkpoint (the reference's Hpm2d)")
    p.add_argument("--hpm3d", default=None, help="with --pck: the 3D lift's checkpoint (Hpm3d); without it only 2D figures")
    p.add_argument("--pck_max", type=float, default=30, help="largest PCK threshold in pixels (the reference's 30)")
    p.add_argument("--pck_steps", type=int, default=20, help="number of PCK thresholds from 0 to --pck_max (the reference's 20)")
    p.add_argument("--inception", default=None, help="also the Inception score: torchvision's inception_v3_google state dict")
    p.add_argument("--is_group", type=int, default=64, help="with --inception: images per scored group (the reference's 64)")
    p.add_argument("--fid", default=None, help="also FID and KID against real images: an Inception-v3 state dict")
    p.add_argument("--fid_variant", default="torchvision", choices=("torchvision", "fid"),
                   help="with --fid: torchvision's graph, or pytorch-fid's (for its pt_inception-2015-12-05 weights)")
    p.add_argument("--fid_real", default=None, help="with --fid: the real set - a directory of PNGs or a statistics .npz "
                                                    "(default: the split's target images; required with --fid_images)")
    p.add_argument("--fid_stats_out", default=None, help="with --fid: write the real set's mu, sigma, n, variant and features here")
    p.add_argument("--kid_subsets", type=int, default=100, help="with --fid: number of random subsets of KID (torch-fidelity's 100)")
    p.add_argument("--kid_subset_size", type=int, default=1000, help="with --fid: images per subset, clamped to the smaller set")
    p.add_argument("--kid_seed", type=int, default=0, help="with --fid: seed of the subsets' np.random.RandomState")
    p.add_argument("--lpips", default=None, help="also LPIPS (VGG-16) against the target: torchvision's vgg16 state dict")
    p.add_argument("--lpips_lin", default=None, help="with --lpips: the lpips package's linear heads (lin{0..4}.model.1.weight), "
                                                     "or 'uniform' for the unweighted form; required with --lpips")
    p.add_argument("--lpips_ref", default=None, help="with --lpips_images: the directory of the reference PNGs, same relative names")
    p.add_argument("--ms_ssim", action="store_true",
                   help="also multi-scale SSIM (5 scales, the weights of Wang, Simoncelli, Bovik 2003) of the pair SSIM scores, with "
                        "--window; the image's smaller side must exceed (window - 1) * 16 (160 at the default window)")
    p.add_argument("--hand_region", action="store_true",
                   help="also SSIM, L1 and PSNR over the hand alone: the pixels under one of the target pose's 20 bones, drawn as "
                        "capsules of --hand_radius pixels from the target's labels")
    p.add_argument("--hand_radius", type=float, default=None,
                   help="with --hand_region: half-width of a bone in pixels of the scored grid; default 10 * H / 256.  Capsules of "
                        "the default radius leave gaps in the palm between the metacarpals; a larger radius closes them")
    return p


def strip_module(sd):
    """Evaluator._get_weights (utils.py:126-136): DataParallel / DDP checkpoints carry a leading 'module.'"""
    return type(sd)((k[len("module."):] if k.startswith("module.") else k, v) for k, v in sd.items())


def infer_generator_config(sd):
    """(ngf, n_blocks, norm, use_dropout) of a Generator state_dict (values may be tensors or shapes): ngf from the first
    stem conv, n_blocks from the model.att.<i> indices, batch norm iff running statistics are stored, dropout iff the
    second conv of conv_block_stream1 sits at index 6 (5 without the Dropout layer; InferenceGenerator's fold reads it)."""
    sd = strip_module(sd)
    w = sd.get("model.stream1_down.1.weight")
    if w is None:
        raise ValueError("not a Generator state_dict: no model.stream1_down.1.weight")
    ngf = int((w.shape if hasattr(w, "shape") else w)[0])
    blocks = {int(m.group(1)) for k in sd for m in [re.match(r"model\.att\.(\d+)\.", k)] if m}
    n_blocks = max(blocks) + 1 if blocks else 0
    norm = "batch" if any(k.endswith("running_mean") for k in sd) else "instance"

    def conv_at(i):         # a 4-D weight (conv) at index i; under batch norm the norm after the conv at 5 sits at 6
        v = sd.get(f"model.att.0.conv_block_stream1.{i}.weight")
        return v is not None and len(v.shape if hasattr(v, "shape") else v) == 4

    use_dropout = conv_at(6)
    if n_blocks and not use_dropout and not conv_at(5):
        raise ValueError("not a Generator state_dict: no second conv in model.att.0.conv_block_stream1")
    return ngf, n_blocks, norm, use_dropout


def _opt(args):
    from .options import default_train_opt
    opt = default_train_opt(batchSize=args.batchSize, local_rank=args.gpu, isTrain=False)
    opt.dataroot, opt.dataset, opt.augmentation_ratio, opt.distributed = (args.dataroot, args.dataset,
                                                                          args.augmentation_ratio, False)
    opt.device_png = bool(getattr(args, "device_png", False))
    opt.resize_inputs = int(getattr(args, "resize_inputs", 0) or 0)
    opt.pairing, opt.match_pool = getattr(args, "pairing", None) or "random", getattr(args, "match_pool", None) or "self"
    opt.depth_source = getattr(args, "depth_source", None) or "files"
    opt.render_radius, opt.render_bg = float(getattr(args, "render_radius", 5.0)), float(getattr(args, "render_bg", 255.0))
    return opt


def _pose_distances(args, loader):
    """{(target, source): pose distance} of the loader's pairs when --pairing is given, else None (nothing is launched)"""
    if not getattr(args, "pairing", None):
        return None
    d = loader.pair_distance
    return {(t, s): float(d[i]) for i, (s, t) in enumerate(zip(loader.image_source, loader.image_target))}


PCK_FLAGS = ("pck", "pck_images", "hpm2d", "hpm3d", "pck_max", "pck_steps")


def _estimator(args, dev):
    """the hand-pose estimators of --pck, or None (then nothing of them is loaded or launched)"""
    if not args.pck:
        return None
    from .hpe import HPEstimator, Z_SCALE
    return HPEstimator(args.hpm2d, args.hpm3d, device=dev, z_scale=Z_SCALE[args.dataset])


IS_FLAGS = ("inception", "is_group", "is_images")


def _scorer(args, dev):
    """the Inception scorer of --inception, or None (then nothing of it is loaded or launched)"""
    if not args.inception:
        return None
    from .inception import InceptionScorer
    return InceptionScorer(args.inception, group=args.is_group, device=dev)


FID_FLAGS = ("fid", "fid_variant", "fid_real", "fid_stats_out", "kid_subsets", "kid_subset_size", "kid_seed", "fid_images")
FID_KEYS = ("FID", "KID_mean", "KID_std", "KID_full", "n_real", "n_generated", "fid_variant")


def _png_batches(root, batch_size, flag):
    """every PNG below `root` in sorted order as (paths, uint8 [B,H,W,3] B,G,R) batches, cut where the size changes"""
    from .data import _read_bgr
    if not os.path.isdir(root):
        raise SystemExit(f"evaluate: {flag} {root} is not a directory")
    paths = sorted(os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs if f.lower().endswith(".png"))
    if not paths:
        raise SystemExit(f"evaluate: {flag} {root} holds no PNG")
    batch = []
    for p in paths:
        im = _read_bgr(p)
        if batch and (len(batch) == batch_size or batch[0][1].shape != im.shape):
            yield [q for q, _ in batch], np.stack([i for _, i in batch])
            batch = []
        batch.append((p, im))
    yield [q for q, _ in batch], np.stack([i for _, i in batch])


def _fid_scorer(args, dev, isc=None):
    """the FID / KID scorer of --fid, or None (then nothing of it is imported, loaded or launched).  It shares the network of
    --inception when both name the same file and graph.  With --fid_real the real side is complete on return (fsc.own_real is
    False) and the caller feeds generated images only."""
    if not args.fid:
        return None
    from .fid import FidScorer, load_stats
    shared = (isc is not None and args.fid_variant == "torchvision" and
              os.path.abspath(args.fid) == os.path.abspath(args.inception))
    fsc = FidScorer(isc.net if shared else args.fid, variant=args.fid_variant, device=dev, kid_subsets=args.kid_subsets,
                    kid_subset_size=args.kid_subset_size, kid_seed=args.kid_seed)
    fsc.shared, fsc.own_real = shared, not args.fid_real
    if args.fid_real and os.path.isfile(args.fid_real):
        fsc.set_real_stats(load_stats(args.fid_real))
    elif args.fid_real:
        for _, u8 in _png_batches(args.fid_real, args.batchSize, "--fid_real"):
            fsc.feed_real(torch.from_numpy(u8).to(dev), "bgr_hwc")
    return fsc


def _feed_scorers(isc, fsc, images, layout, paths, real=None, real_layout=None):
    """one batch of scored images to the Inception score and / or FID; `real`: its targets, fed unless --fid_real was given"""
    if fsc is not None:
        feats = fsc.features(images, layout)
        fsc.feed_generated(images, layout, features=feats)
        if real is not None and fsc.own_real:
            fsc.feed_real(real, real_layout)
        if isc is not None and fsc.shared:      # one forward serves both: features first, then fc
            isc.feed_features(feats, paths)
            return
    if isc is not None:
        isc.feed(images, layout, paths)


def _fid_summary(args, fsc, summary):
    res = fsc.results(args.fid_stats_out)
    for k in FID_KEYS:
        summary[k] = res[k]


def _main_fid_images(args):
    """--fid_images DIR --fid_real DIR|NPZ: two sets of PNGs, no labels"""
    torch.cuda.set_device(args.gpu)
    dev = torch.device("cuda", args.gpu)
    fsc = _fid_scorer(args, dev)
    n = 0
    for paths, u8 in _png_batches(args.fid_images, args.batchSize, "--fid_images"):
        fsc.feed_generated(torch.from_numpy(u8).to(dev), "bgr_hwc")
        n += len(paths)
    summary = {"n": n}
    _fid_summary(args, fsc, summary)
    print(json.dumps(summary))
    out = args.results_json or os.path.join(args.fid_images, "eval_fid.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump({"summary": summary, "options": {k: v for k, v in vars(args).items() if k not in IS_FLAGS + PCK_FLAGS + LPIPS_FLAGS},
                   "generator": None,
                   "domain": "the PNGs' bytes, resized to 299 as PIL.Image.resize(BILINEAR), centre crop, the variant's normalisation"},
                  fh, indent=1)
    return {"summary": summary, "rows": []}


LPIPS_FLAGS = ("lpips", "lpips_lin", "lpips_images", "lpips_ref")
LPIPS_KEYS = ("LPIPS_avg", "LPIPS_layers", "lpips_lin")


def _lpips_scorer(args, dev):
    """the LPIPS scorer of --lpips, or None (then nothing of it is imported, loaded or launched)"""
    if not getattr(args, "lpips", None):
        return None
    from .lpips import LpipsScorer
    return LpipsScorer(args.lpips, args.lpips_lin, device=dev)


def _lpips_summary(lsc, summary, rows):
    """the scorer's figures into the summary, a lpips value into the rows"""
    res = lsc.results()
    for k in LPIPS_KEYS:
        summary[k] = res[k]
    own = lsc.rows()
    if rows is None:
        return own
    assert len(rows) == len(own)
    for r, e in zip(rows, own):
        assert r.get("target") == e.get("target"), (r, e)
        r["lpips"] = e["lpips"]
    return rows


def _main_lpips_images(args):
    """--lpips_images DIR --lpips_ref DIR: two directories of PNGs paired by relative file name, no labels"""
    from .data import _read_bgr

    def listing(root, flag):
        if not os.path.isdir(root):
            raise SystemExit(f"evaluate: {flag} {root} is not a directory")
        names = sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs
                       if f.lower().endswith(".png"))
        if not names:
            raise SystemExit(f"evaluate: {flag} {root} holds no PNG")
        return names

    names, ref = listing(args.lpips_images, "--lpips_images"), listing(args.lpips_ref, "--lpips_ref")
    if names != ref:
        odd = sorted(set(names) ^ set(ref))
        raise SystemExit(f"evaluate: --lpips_images / --lpips_ref: {len(odd)} file(s) without a partner of the same relative name, "
                         f"e.g. {odd[0]}")
    torch.cuda.set_device(args.gpu)
    dev = torch.device("cuda", args.gpu)
    lsc = _lpips_scorer(args, dev)
    batch = []

    def flush():
        if batch:
            lsc.feed(torch.from_numpy(np.stack([a for _, a, _ in batch])).to(dev), "bgr_hwc",
                     torch.from_numpy(np.stack([b for _, _, b in batch])).to(dev), "bgr_hwc", [{"target": n} for n, _, _ in batch])
            batch.clear()

    for n in names:
        a, b = _read_bgr(os.path.join(args.lpips_images, n)), _read_bgr(os.path.join(args.lpips_ref, n))
        if a.shape != b.shape:
            raise SystemExit(f"evaluate: {n}: {a.shape} below --lpips_images, {b.shape} below --lpips_ref")
        if batch and (len(batch) == args.batchSize or batch[0][1].shape != a.shape):
            flush()
        batch.append((n, a, b))
    flush()
    summary = {"n": len(names)}
    rows = _lpips_summary(lsc, summary, None)
    print(json.dumps(summary))
    out = args.results_json or os.path.join(args.lpips_images, "eval_lpips.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump({"summary": summary,
                   "options": {k: v for k, v in vars(args).items() if k not in IS_FLAGS + PCK_FLAGS + FID_FLAGS},
                   "generator": None, "domain": "the PNGs' bytes as RGB in [-1, 1]: u / 255 * 2 - 1, then the LPIPS scaling layer"},
                  fh, indent=1)
    if args.per_image_csv:
        with open(args.per_image_csv, "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(["target", "lpips"])
            for r in rows:
                w.writerow([r["target"], repr(r["lpips"])])
    return {"summary": summary, "rows": rows}


def _pose_labels(loader, paths, size=None):
    """(uv [B,21,2], depth [B,21]) of the images' labels, float64; under --resize_inputs N the joints on the N x N grid"""
    from . import ops
    from .data import png_size
    uv, depth = [], []
    for p in paths:
        a = loader.get_labels(p)
        j = torch.as_tensor(np.asarray(a["uv_coord"], dtype=np.float64).reshape(21, 2))
        if size:
            j = ops.resize_joints(j, png_size(p), (size, size))
        uv.append(j.numpy())
        depth.append(np.asarray(a["depth"], dtype=np.float64).reshape(21))
    return np.stack(uv), np.stack(depth)


REGION_FLAGS = ("ms_ssim", "hand_region", "hand_radius")
MS_LEVELS = 5


def _meter(args, rng):
    """the SSIM / L1 / PSNR meter; --ms_ssim and --hand_region add their columns to it, and without them it is the plain one"""
    return QualityMeter(rng, args.window, ms_ssim=args.ms_ssim, hand=args.hand_region)


def _scored_size(loader):
    """(H, W) of the scored grid: --resize_inputs N, or the first target file's size"""
    from .data import png_size
    if loader.out_size:
        return loader.out_size, loader.out_size
    return png_size(loader.image_target[0]) if len(loader.image_target) else None


def _check_ms_size(args, loader):
    """--ms_ssim: the min-side rule of mmh_ms_ssim, before anything is scored"""
    from .metrics import ms_ssim_min_side
    size = _scored_size(loader) if args.ms_ssim else None
    if size is not None and min(size) <= ms_ssim_min_side(args.window, MS_LEVELS):
        raise SystemExit(f"evaluate: --ms_ssim: images of {size[0]} x {size[1]}: the smaller side must exceed (window - 1) * "
                         f"2^(levels - 1) = {ms_ssim_min_side(args.window, MS_LEVELS)} for {MS_LEVELS} levels at --window "
                         f"{args.window} (see --resize_inputs)")


def hand_radius(args, H):
    """--hand_radius, or its default on an H-row grid: 10 pixels at 256 rows, in proportion"""
    return float(args.hand_radius) if args.hand_radius is not None else 10.0 * H / 256.0


def _hand_masks(args, loader, meter, targets, H, W, dev):
    """--hand_region: the targets' hand masks uint8 [B,H,W] on the scored grid, from their labels (the radius used is left on
    the meter for the summary); None without the flag"""
    if not args.hand_region:
        return None
    from .metrics import hand_mask
    uv, _ = _pose_labels(loader, targets, loader.out_size)
    meter.hand_radius = hand_radius(args, H)
    return hand_mask(torch.from_numpy(uv).to(dev), (H, W), meter.hand_radius)


def _score_generator(args, ckpt, dev):
    from .data import HandFolderLoader
    from .inference import InferenceGenerator
    from .networks import Generator
    est, isc = _estimator(args, dev), _scorer(args, dev)
    fsc, lsc = _fid_scorer(args, dev, isc), _lpips_scorer(args, dev)
    sd = strip_module(torch.load(ckpt, map_location="cpu"))
    ngf, n_blocks, norm, use_dropout = infer_generator_config(sd)
    net = Generator(input_nc=[3, 42, 6], output_nc=3, ngf=ngf, norm_layer=norm, use_dropout=use_dropout, n_blocks=n_blocks)
    net.load_state_dict(sd)
    gen = InferenceGenerator(net.to(dev).eval(), use_graph=True, bf16=args.bf16)
    loader = HandFolderLoader(_opt(args), device=dev, decoded=True)
    _check_ms_size(args, loader)
    meter = _meter(args, "pm1")
    for s in loader:
        fake = gen([s["H1"], torch.cat((s["P1"], s["P2"]), 1), torch.cat((s["D1"], s["D2"]), 1)])
        # gen returns its graph's static output buffer: the metric is enqueued here, before the next replay
        paths = [{"target": t, "source": h} for t, h in zip(s["H2_path"], s["H1_path"])]
        meter.feed(fake, s["H2"], paths, _hand_masks(args, loader, meter, s["H2_path"], fake.shape[2], fake.shape[3], dev))
        if est is not None:     # the fake batch as it lies on the device: min-max normalised by the estimator's first kernel
            est.feed(fake, *_pose_labels(loader, s["H2_path"], loader.out_size), paths=paths)
        if fsc is not None:     # FID / KID: the fake batch against its targets; --inception may ride on the same forward
            _feed_scorers(isc, fsc, fake, "nchw", paths, s["H2"], "nchw")
        elif isc is not None:   # likewise: the scorer's first kernel turns the tensor into the bytes aug would write
            isc.feed(fake, "nchw", paths)
        if lsc is not None:     # LPIPS: the fake batch against the target the SSIM meter scores it against
            lsc.feed(fake, "nchw", s["H2"], "nchw", paths)
    return (meter, {"ngf": ngf, "n_blocks": n_blocks, "norm": norm, "use_dropout": use_dropout}, _pose_distances(args, loader),
            est, isc, fsc, lsc)


def _read_generated(path):
    from .data import _read_bgr
    if os.path.isfile(path):
        return _read_bgr(path)
    npy = os.path.splitext(path)[0] + ".npy"            # aug.py's fallback without PIL: RGB uint8 arrays
    if os.path.isfile(npy):
        return np.ascontiguousarray(np.load(npy)[:, :, ::-1])
    raise SystemExit(f"--generated: {path} is missing (aug.py writes <DIR>/<folder of the target>/<name>)")


def _targets_at(ref, size):
    """uint8 [B,H,W,3] BGR target images -> fp32 [B,3,N,N] RGB in [-1, 1] as the device's decode pass delivers them at
    N x N (the colour lanes of ops.decode_inputs; its other inputs are not looked at)"""
    from . import ops
    uv = torch.zeros((ref.shape[0], 21, 2), dtype=torch.float64, device=ref.device)
    xh, _, _, _ = ops.decode_inputs(ref, ref, ref, ref, uv, uv, out_size=size)
    return ops.nhwc_to_nchw_view(xh, 3)


def _score_directory(args, dev):
    from .data import HandFolderLoader, _read_bgr
    loader = HandFolderLoader(_opt(args), device=dev)
    size = loader.out_size
    # at the files' size both sides are bytes; at --resize_inputs N the targets are the decode pass's fp32 images, and the
    # PNGs' bytes are mapped to the same [-1, 1] range
    _check_ms_size(args, loader)
    meter = _meter(args, "pm1" if size else "u8_bgr_hwc")
    est, isc = _estimator(args, dev), _scorer(args, dev)
    fsc, lsc = _fid_scorer(args, dev, isc), _lpips_scorer(args, dev)
    idx = loader.indices()
    for i in range(0, len(idx), args.batchSize):
        tgts = [loader.image_target[j] for j in idx[i:i + args.batchSize]]
        srcs = [loader.image_source[j] for j in idx[i:i + args.batchSize]]
        gen = [_read_generated(os.path.join(args.generated, *t.split("/")[-2:])) for t in tgts]
        ref = [_read_bgr(t) for t in tgts]
        for g, r, t in zip(gen, ref, tgts):
            want = (size, size, 3) if size else r.shape
            if g.shape != want:
                raise SystemExit(f"--generated: {t}: generated image {g.shape} vs target {want}")
        g8 = torch.from_numpy(np.stack(gen)).to(dev)
        mask = _hand_masks(args, loader, meter, tgts, g8.shape[1], g8.shape[2], dev)
        if est is not None:     # the PNGs' bytes, B,G,R as they were read
            est.feed(g8, *_pose_labels(loader, tgts, size), paths=[{"target": t, "source": s} for t, s in zip(tgts, srcs)],
                     layout="bgr_hwc")
        if fsc is not None:     # the real side: the targets' bytes, or at --resize_inputs N the decode pass's images
            real, real_layout = None, None
            if fsc.own_real:
                real, real_layout = torch.from_numpy(np.stack(ref)).to(dev).contiguous(), "bgr_hwc"
                if size:
                    real, real_layout = _targets_at(real, size), "nchw"
            _feed_scorers(isc, fsc, g8, "bgr_hwc", [{"target": t, "source": s} for t, s in zip(tgts, srcs)], real, real_layout)
        elif isc is not None:
            isc.feed(g8, "bgr_hwc", [{"target": t, "source": s} for t, s in zip(tgts, srcs)])
        if lsc is not None:     # LPIPS: the PNGs' bytes against what the SSIM meter below takes as the target
            r8 = torch.from_numpy(np.stack(ref)).to(dev).contiguous()
            tgt, tgt_layout = (_targets_at(r8, size), "nchw") if size else (r8, "bgr_hwc")
            lsc.feed(g8, "bgr_hwc", tgt, tgt_layout, [{"target": t, "source": s} for t, s in zip(tgts, srcs)])
        if size:
            pred = (g8.flip(-1).permute(0, 3, 1, 2).float() / 255.0 - 0.5) / 0.5
            meter.feed(pred, _targets_at(torch.from_numpy(np.stack(ref)).to(dev).contiguous(), size),
                       [{"target": t, "source": s} for t, s in zip(tgts, srcs)], mask)
            continue
        meter.feed(g8, torch.from_numpy(np.stack(ref)).to(dev),
                   [{"target": t, "source": s} for t, s in zip(tgts, srcs)], mask)
    return meter, {}, _pose_distances(args, loader), est, isc, fsc, lsc


def _is_summary(isc, summary, rows):
    """the scorer's figures into the summary (IS_avg / IS_std are the reference's keys, utils.py:67-68), is_kl into the rows"""
    res = isc.results()
    summary["IS_avg"], summary["IS_std"], summary["IS_all"] = res["IS_avg"], res["IS_std"], res["IS_all"]
    summary["is_groups"] = res["n_groups"]
    if rows is None:
        return res["rows"]
    assert len(rows) == len(res["rows"])
    for r, e in zip(rows, res["rows"]):
        assert r.get("target") == e.get("target"), (r, e)
        r["is_kl"] = e["is_kl"]
    return rows


def _main_is_images(args):
    """--is_images: every PNG below the directory in sorted order, batched while the size stays the same"""
    from .data import _read_bgr
    if not os.path.isdir(args.is_images):
        raise SystemExit(f"evaluate: --is_images {args.is_images} is not a directory")
    paths = sorted(os.path.join(d, f) for d, _, fs in os.walk(args.is_images) for f in fs if f.lower().endswith(".png"))
    if not paths:
        raise SystemExit(f"evaluate: --is_images {args.is_images} holds no PNG")
    torch.cuda.set_device(args.gpu)
    dev = torch.device("cuda", args.gpu)
    isc = _scorer(args, dev)
    batch = []

    def flush():
        if batch:
            isc.feed(torch.from_numpy(np.stack([im for _, im in batch])).to(dev), "bgr_hwc", [{"target": p} for p, _ in batch])
            batch.clear()

    for p in paths:
        im = _read_bgr(p)
        if batch and (len(batch) == args.batchSize or batch[0][1].shape != im.shape):
            flush()
        batch.append((p, im))
    flush()
    summary = {"n": len(paths)}
    rows = _is_summary(isc, summary, None)
    print(json.dumps(summary))
    out = args.results_json or os.path.join(args.is_images, "eval_is.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump({"summary": summary, "options": {k: v for k, v in vars(args).items() if k not in FID_FLAGS + LPIPS_FLAGS}, "generator": None,
                   "domain": "the PNGs' bytes, resized to 299 as PIL.Image.resize(BILINEAR), centre crop, ImageNet normalisation"},
                  fh, indent=1)
    if args.per_image_csv:
        with open(args.per_image_csv, "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(["target", "is_kl"])
            for r in rows:
                w.writerow([r["target"], repr(r["is_kl"])])
    return {"summary": summary, "rows": rows}


def _score_pck_images(args, dev):
    """--pck_images: every colour image the prepared directory lists (the loader's own list and order), against its labels"""
    from .data import HandFolderLoader, _read_bgr
    args.dataroot = args.pck_images
    loader = HandFolderLoader(_opt(args), device=dev)
    est = _estimator(args, dev)
    paths = list(loader._all_images)
    for i in range(0, len(paths), args.batchSize):
        chunk = paths[i:i + args.batchSize]
        imgs = [_read_bgr(p) for p in chunk]
        if any(im.shape != imgs[0].shape for im in imgs):
            raise SystemExit(f"--pck_images: images of different sizes in one batch ({chunk[0]} ...)")
        est.feed(torch.from_numpy(np.stack(imgs)).to(dev), *_pose_labels(loader, chunk), paths=[{"target": p} for p in chunk],
                 layout="bgr_hwc")
    return est


def _pck_summary(args, est, summary, rows):
    """the estimator's figures under the reference's keys (utils.py:71-73) into the summary, epe columns into the rows"""
    res = est.results(args.pck_max, args.pck_steps)
    for tag in ("2d", "3d"):
        m = res["pck" + tag]
        if m is None:
            continue
        summary[f"pck{tag}_auc"] = m["auc"]
        summary[f"epe{tag}_mean"], summary[f"epe{tag}_median"] = m["epe_mean"], m["epe_median"]
        summary[f"pck{tag}_curve"] = m["curve"]
    summary["pck_thresholds"] = res["pck2d"]["thresholds"]
    cols = ["epe2d"] + (["epe3d"] if res["pck3d"] is not None else [])
    if rows is None:
        return res["rows"], cols
    assert len(rows) == len(res["rows"])
    for r, e in zip(rows, res["rows"]):
        assert r.get("target") == e.get("target"), (r, e)
        r.update({k: e[k] for k in cols})
    return rows, cols


def _main_pck_images(args):
    if not os.path.isdir(args.pck_images):
        raise SystemExit(f"evaluate: --pck_images {args.pck_images} is not a directory")
    torch.cuda.set_device(args.gpu)
    dev = torch.device("cuda", args.gpu)
    est = _score_pck_images(args, dev)
    summary = {"n": 0}
    rows, cols = _pck_summary(args, est, summary, None)
    summary["n"] = len(rows)
    print(json.dumps(summary))
    out = args.results_json or os.path.join(args.pck_images, f"eval_pck_{args.dataset}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump({"summary": summary, "options": {k: v for k, v in vars(args).items() if k not in IS_FLAGS + FID_FLAGS + LPIPS_FLAGS}, "generator": None,
                   "domain": "min-max normalised per image, as the reference's datasets hand real images to the estimators"},
                  fh, indent=1)
    if args.per_image_csv:
        with open(args.per_image_csv, "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(["target"] + cols)
            for r in rows:
                w.writerow([r["target"]] + [repr(r[k]) for k in cols])
    return {"summary": summary, "rows": rows}


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if not (3 <= args.window <= 15 and args.window % 2 == 1):
        parser.error(f"--window {args.window}: the SSIM window is odd, from 3 to 15")
    if args.batchSize < 1:
        parser.error("--batchSize must be >= 1")
    from .options import check_depth_source, check_resize_inputs
    check_resize_inputs(args)
    check_depth_source(args)
    if args.pck_images:
        args.pck = True
    if args.pck and not args.hpm2d:
        parser.error("--pck / --pck_images need --hpm2d <checkpoint of the 2D hand-pose machine>")
    if args.pck and not (args.pck_max > 0 and args.pck_steps >= 2):
        parser.error("--pck_max must be > 0 and --pck_steps >= 2")
    if args.is_images and not args.inception:
        parser.error("--is_images needs --inception <torchvision's inception_v3_google state dict>")
    if args.inception and args.is_group < 1:
        parser.error("--is_group must be >= 1")
    if args.fid_images and not (args.fid and args.fid_real):
        parser.error("--fid_images needs --fid <Inception-v3 state dict> and --fid_real <directory of PNGs | stats.npz>")
    if not args.fid and (args.fid_real or args.fid_stats_out):
        parser.error("--fid_real / --fid_stats_out need --fid <Inception-v3 state dict>")
    if args.fid and (args.is_images or args.pck_images):
        parser.error("--fid scores generated images against real ones: not with --is_images / --pck_images (see --fid_images)")
    if args.fid and (args.kid_subsets < 1 or args.kid_subset_size < 2):
        parser.error("--kid_subsets must be >= 1 and --kid_subset_size >= 2")
    if args.lpips and not args.lpips_lin:
        parser.error("--lpips needs --lpips_lin <the lpips package's linear heads | uniform>")
    if args.lpips_images and not (args.lpips and args.lpips_ref):
        parser.error("--lpips_images needs --lpips <VGG-16 state dict>, --lpips_lin <file | uniform> and --lpips_ref <directory>")
    if not args.lpips and args.lpips_lin:
        parser.error("--lpips_lin needs --lpips <VGG-16 state dict>")
    if args.lpips_ref and not args.lpips_images:
        parser.error("--lpips_ref belongs to --lpips_images")
    if args.lpips and (args.is_images or args.pck_images or args.fid_images):
        parser.error("--lpips scores image pairs: not with --is_images / --pck_images / --fid_images (see --lpips_images)")
    if args.hand_radius is not None and not args.hand_region:
        parser.error("--hand_radius belongs to --hand_region")
    if args.hand_radius is not None and not (args.hand_radius >= 0 and np.isfinite(args.hand_radius)):
        parser.error("--hand_radius must be finite and >= 0")
    if (args.ms_ssim or args.hand_region) and not (args.name or args.generated):
        parser.error("--ms_ssim / --hand_region score image pairs against their targets: with --name or --generated only")
    if not (args.name or args.generated):       # the other modes' option dumps never knew these flags
        for k in REGION_FLAGS:
            delattr(args, k)
    if args.is_images:
        return _main_is_images(args)
    if args.fid_images:
        return _main_fid_images(args)
    if args.lpips_images:
        return _main_lpips_images(args)
    if not args.dataset:
        parser.error("the following arguments are required: --dataset")
    if args.pck_images:
        return _main_pck_images(args)
    if not args.dataroot:
        parser.error("the following arguments are required: --dataroot")
    ckpt = None
    if args.name:
        ckpt = os.path.join(args.checkpoints_dir, args.name, f"{args.which_epoch}_net_netG.pth")
        if not os.path.isfile(ckpt):
            raise SystemExit(f"evaluate: no checkpoint {ckpt} (--name / --checkpoints_dir / --which_epoch)")
    elif not os.path.isdir(args.generated):
        raise SystemExit(f"evaluate: --generated {args.generated} is not a directory")
    torch.cuda.set_device(args.gpu)
    dev = torch.device("cuda", args.gpu)
    meter, config, pose_d, est, isc, fsc, lsc = _score_generator(args, ckpt, dev) if ckpt else _score_directory(args, dev)
    res = meter.result()
    summary = res["summary"]
    if args.hand_region:
        summary["hand_radius"] = getattr(meter, "hand_radius", None)
    meter_cols = ((["ms_ssim"] if args.ms_ssim else []) +
                  (["ssim_hand", "l1_hand", "psnr_hand", "hand_fraction"] if args.hand_region else []))
    pck_cols = _pck_summary(args, est, summary, res["rows"])[1] if est is not None else []
    if isc is not None:
        _is_summary(isc, summary, res["rows"])
        pck_cols = pck_cols + ["is_kl"]
    if fsc is not None:
        _fid_summary(args, fsc, summary)
    if lsc is not None:
        _lpips_summary(lsc, summary, res["rows"])
        pck_cols = pck_cols + ["lpips"]
    if pose_d is not None:
        for r in res["rows"]:
            r["pose_distance"] = pose_d[(r["target"], r["source"])]
        known = [r["pose_distance"] for r in res["rows"] if r["pose_distance"] == r["pose_distance"]]
        summary["pairing"] = args.pairing
        summary["pose_distance_avg"] = float(np.mean(known)) if known else float("nan")
    print(json.dumps(summary))
    out = args.results_json or (os.path.join(args.checkpoints_dir, args.name, f"eval_{args.which_epoch}_{args.dataset}.json")
                                if ckpt else os.path.join(args.generated, f"eval_{args.dataset}.json"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        # the pairing flags appear among the options only when --pairing was given: without it the file is what it always was
        options = {k: v for k, v in vars(args).items() if pose_d is not None or k not in ("pairing", "match_pool")}
        if args.depth_source == "files":       # likewise the render's flags: only under --depth_source joints
            options = {k: v for k, v in options.items() if k not in ("depth_source", "render_radius", "render_bg")}
        if est is None:                         # and the estimators' flags: only under --pck
            options = {k: v for k, v in options.items() if k not in PCK_FLAGS}
        if isc is None:                         # and the Inception score's: only under --inception
            options = {k: v for k, v in options.items() if k not in IS_FLAGS}
        if fsc is None:                         # and FID / KID's: only under --fid
            options = {k: v for k, v in options.items() if k not in FID_FLAGS}
        if lsc is None:                         # and LPIPS's: only under --lpips
            options = {k: v for k, v in options.items() if k not in LPIPS_FLAGS}
        if not args.ms_ssim:                    # and the multi-scale and hand-region flags, each only when given
            options = {k: v for k, v in options.items() if k != "ms_ssim"}
        if not args.hand_region:
            options = {k: v for k, v in options.items() if k not in ("hand_region", "hand_radius")}
        json.dump({"summary": summary, "options": options, "generator": config or None,
                   "domain": "[0, 1]: generator output (x + 1) / 2, PNG pixels u8 / 255"}, fh, indent=1)
    if args.per_image_csv:
        with open(args.per_image_csv, "w", newline="") as fh:
            w = csv.writer(fh)
            extra = meter_cols + (["pose_distance"] if pose_d is not None else []) + pck_cols
            w.writerow(["target", "source", "ssim", "l1", "psnr"] + extra)
            for r in res["rows"]:
                w.writerow([r["target"], r["source"], repr(r["ssim"]), repr(r["l1"]), repr(r["psnr"])] + [repr(r[k]) for k in extra])
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
