"""Batches for the step, with the reference loader's batch-dict contract (data/generic_dataset.py:169-180: keys
H1,H2,P1,P2,D1,D2,C1,C2,H1_path,H2_path).

`SyntheticHandLoader`: RHD/STB-shaped synthetic batches: H ~ U(-1,1) [B,3,H,W]; P = 21 Gaussian pose
maps (sigma 6, threshold 0.0099, clamp 1) at joints uv ~ U(20,H-20); D = one U(-1,1) plane replicated to 3 channels (RHD
and STB share this live code path, generic_dataset.py:151-159).  Pose maps are synthesised on the device by
mmh_pose_heatmaps.

`HandFolderLoader`: the reference's PREPARED dataset directory -
`annotation.pickle` + `<folder>/<name>.png` colour images + the depth PNG at the same path with "color" replaced by
"depth" (data/generic_dataset.py:86-180, data/rhd_dataset.py:16-45, data/stb_dataset.py:16-45) - read with PIL (cv2 is
absent from this image) into pinned uint8 batches that travel to the device as they are; everything arithmetic the
reference's loader workers do per sample on the CPU (normalise, depth = 256 G + R, / 700, 21 full-image Gaussians x 2)
happens in ONE device kernel behind `MMHandModel.set_input` (mmh_decode_inputs).  The legacy pair-list format of
data/mmhand_dataset.py (CSV pairs + .npy pose arrays) is not read.

`HandFolderLoader(device_png=True)` (--device_png, MMH_DEVICE_PNG=1; off by default) moves the boundary from decoded pixels
to the files' bytes: the threads only read the files, the batch's zlib streams go up as one pinned buffer and
mmh_png_decode_batch (png.py) writes the same uint8 [B,H,W,3] BGR tensors.

`HandFolderLoader(resident=True)` (--resident_dataset, MMH_RESIDENT_DATASET=1; off by default): the loader's order never
changes between epochs, so the decoded images of this rank's batches are kept in device memory (uint8 [S,Hs,Ws,3], one slot
per file).  The first epoch reads the files as above and copies each batch into the store (mmh_store_images); from then on a
batch is a row of slots and ONE kernel (mmh_decode_inputs_indexed) - no file read, no PNG decode, no upload.

`HandFolderLoader` with `opt.pairing` = curriculum | nearest (--pairing; the default `random` is the reference's live loader):
the paper's two pairing strategies on the reference's pose distance (nearest_neighbor_search.py:68-83, on the device:
ops.pose_features / pose_knn / pose_pair_distance).  Both are decided once, in the constructor, so the order stays static.

`HandFolderLoader` with `opt.augment_geom` (--augment_geom; off by default): every image gets a random rotation, scale, shift
(and flip) per epoch.  The host draws the parameters for the whole dataset from (aug_seed, epoch) (`augment_draws`), builds
the 2x3 sampling matrices and transforms the joints in float64 (`affine_forward`, `affine_inverse`, `affine_joints`); the
device samples through the matrix inside its decode pass (mmh_decode_inputs_affine / mmh_decode_inputs_indexed_affine).  The
order of the batches, and with it the resident store, stays what it is: only `set_epoch`'s number reaches the draws.

`HandFolderLoader` with `opt.depth_source` = joints (--depth_source joints; the default `files` is the reference's loader): D1 /
D2 are rendered from C1 / C2 - the joints as each path has them on the device, on the output grid - by
ops.render_pose_depth, launched right behind the decode pass (here for the decoded form, in MMHandModel.set_input for the raw
and resident forms).  No depth file is opened or sized: a raw batch carries img1 / img2 only, the decode pass is fed the
colour images in the depth arguments and the render overwrites all of x_d; the resident store holds one slot per colour file."""
import math
import os
import pickle
import random

import numpy as np
import torch

from . import ops
from .options import check_augment, check_augment_color, check_depth_source, check_resize_inputs


class SyntheticHandLoader:
    """Iterable of device-resident batches; per-rank shard like DistributedSampler
    (data/mmhand_dataset_data_loader.py:22-24): rank r sees samples r, r+world, ..."""

    def __init__(self, opt, n_samples=256, size=None, device=None):
        self.opt = opt
        self.n = int(n_samples)
        self.size = size or opt.fineSize
        self.device = device or torch.device("cuda", opt.local_rank)
        self.world = getattr(opt, "world_size", 1) or 1
        self.rank = torch.distributed.get_rank() if (self.world > 1 and torch.distributed.is_initialized()) else 0
        self.epoch = 0
        self.name = "synthetic-" + str(getattr(opt, "dataset", None) or "rhd")

    def __len__(self):
        return self.n // self.world

    def set_epoch(self, epoch):
        self.epoch = epoch

    def make_batch(self, B, seed):
        H = W = self.size
        dev = self.device
        g = torch.Generator(device=dev).manual_seed(int(seed))
        out = {}
        for s in ("1", "2"):
            out["H" + s] = torch.rand((B, 3, H, W), generator=g, device=dev) * 2 - 1
            uv = torch.rand((B * 21, 2), generator=g, device=dev, dtype=torch.float64) * (H - 40) + 20
            out["C" + s] = uv.view(B, 21, 2)
            out["P" + s] = ops.pose_heatmaps(uv.contiguous(), H, W).view(B, 21, H, W)
            d = torch.rand((B, 1, H, W), generator=g, device=dev) * 2 - 1
            out["D" + s] = d.expand(B, 3, H, W).contiguous()
        out["H1_path"] = [f"{self.name}/{seed:08d}_{i}_a.png" for i in range(B)]
        out["H2_path"] = [f"{self.name}/{seed:08d}_{i}_b.png" for i in range(B)]
        return out

    def __iter__(self):
        B = self.opt.batchSize
        per_rank = len(self)
        for it in range(per_rank // B):
            seed = (getattr(self.opt, "seed", 49) * 1000003 + self.epoch * 7919 + it) * self.world + self.rank
            yield self.make_batch(B, seed)


# ----------------------------------------------------------------------------- the reference's prepared directories
def _read_bgr(path):
    """what cv2.imread(path) returns for the 8-bit PNGs of the prepared datasets: uint8 [H,W,3] in B,G,R order"""
    from PIL import Image
    with Image.open(path) as im:
        rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return np.ascontiguousarray(rgb[:, :, ::-1])


def _read_bytes(path):
    with open(path, "rb") as fh:
        return fh.read()


_IMAGE_KEYS = ("img1", "img2", "dep1", "dep2")


# ----------------------------------------------------------------------------- resident dataset: host-side planning
def _batch_groups(indices, batch_size, max_batches):
    """the loader's batches as lists of pair indices: in order, the last one may be short, at most `max_batches` of them (the
    reference compares the BATCH index with max_dataset_size)"""
    groups = [list(indices[i:i + batch_size]) for i in range(0, len(indices), batch_size)]
    return groups[: int(min(len(groups), max_batches))]


def resident_plan(image_source, image_target, indices, batch_size, max_batches=float("inf"), depth_source="files"):
    """Which files one rank's batches touch, and where each batch finds them: pure host code, no torch.

    -> (paths, table).  paths: the unique files in order of first use - every colour file and its "color" -> "depth" twin;
    a file that is source in one pair and target in another has ONE slot.  table: int32 [n_batches, batch_size, 4] = the
    slots of (img1, img2, dep1, dep2) of every sample.  A short last batch keeps its own length: its unused rows are -1 and
    are never handed to the device (`table_lengths`), they are not padding a kernel reads.
    depth_source "joints" (--depth_source joints): no depth path is named - `paths` holds the colour files alone and the two
    depth columns repeat the colour slots (the decode pass reads SOMETHING there; the render overwrites what it makes of it)."""
    if depth_source not in ("files", "joints"):
        raise ValueError(f"resident_plan: depth_source {depth_source!r}")
    groups = _batch_groups(indices, batch_size, max_batches)
    slot, paths = {}, []

    def slot_of(path):
        if path not in slot:
            slot[path] = len(paths)
            paths.append(path)
        return slot[path]

    table = np.full((len(groups), int(batch_size), 4), -1, dtype=np.int32)
    for g, items in enumerate(groups):
        for r, item in enumerate(items):
            h1, h2 = image_source[item], image_target[item]
            if depth_source == "joints":
                table[g, r] = [slot_of(h1), slot_of(h2), slot_of(h1), slot_of(h2)]
            else:
                table[g, r] = [slot_of(h1), slot_of(h2), slot_of(h1.replace("color", "depth")), slot_of(h2.replace("color", "depth"))]
    return paths, table


def table_lengths(table):
    """samples per batch of a resident_plan table (the rows in front of the first unused one)"""
    return [int((t[:, 0] >= 0).sum()) for t in table]


def check_table(table, n_slots):
    """The host's range check of a batch table, before it is uploaded: every used row names four slots in [0, n_slots), the
    unused rows (all -1) come last in their batch.  The kernels guard their slots too, but a table that fails here is a bug
    of the plan, and says so."""
    table = np.asarray(table)
    if table.dtype != np.int32 or table.ndim != 3 or table.shape[2] != 4:
        raise ValueError(f"batch table: expected int32 [n_batches, B, 4], got {table.dtype} {table.shape}")
    for g, t in enumerate(table):
        n = int((t[:, 0] >= 0).sum())
        if n == 0 or (t[n:] != -1).any():
            raise ValueError(f"batch table: batch {g} is empty or has rows after its unused ones")
        if (t[:n] < 0).any() or (t[:n] >= n_slots).any():
            raise ValueError(f"batch table: batch {g} names a slot outside [0, {n_slots})")
    return table


def resident_decision(n_paths, Hs, Ws, budget_bytes, free_bytes=None):
    """-> (bytes of the store, "on" | "off: <reason>").  All or nothing: a store that does not fit the budget (--resident_gb)
    or the device's free memory is not built at all."""
    need = int(n_paths) * int(Hs) * int(Ws) * 3
    if n_paths < 1:
        return need, "off: no files to hold"
    if need > budget_bytes:
        return need, f"off: {n_paths} images of {Hs} x {Ws} need {need} bytes, over the budget of {int(budget_bytes)} (--resident_gb)"
    if free_bytes is not None and need > free_bytes:
        return need, f"off: {n_paths} images of {Hs} x {Ws} need {need} bytes, the device has {int(free_bytes)} free"
    return need, "on"


def png_size(path):
    """(height, width) out of a PNG file's IHDR, None for anything else"""
    with open(path, "rb") as fh:
        head = fh.read(24)
    if len(head) < 24 or head[:8] != b"\x89PNG\r\n\x1a\n" or head[12:16] != b"IHDR":
        return None
    return int.from_bytes(head[20:24], "big"), int.from_bytes(head[16:20], "big")


# ----------------------------------------------------------------------------- pose-distance pairing: host-side helpers
PAIRINGS = ("random", "curriculum", "nearest")
MATCH_POOLS = ("self", "train")


def curriculum_order(dist):
    """The curriculum's order of pairs: positions sorted by (pose distance, original position) - a stable ascending argsort,
    pairs without a distance (NaN) last, among themselves in their original order.  Pure host code, no torch."""
    d = np.asarray(dist, dtype=np.float64).reshape(-1)
    nan = np.isnan(d)
    return np.lexsort((np.arange(d.size), np.where(nan, 0.0, d), nan)).astype(np.int64)


def apply_nearest(sources, pool, idx):
    """-> (sources', fallbacks): the source of target i becomes pool[idx[i]] (idx: the nearest candidate of every target, [n]
    or the [n, k] of ops.pose_knn, whose first column counts); where idx is -1 - no valid neighbour - the given source stays
    and i is reported in `fallbacks`.  Pure host code, no torch."""
    idx = np.asarray(idx)
    if idx.ndim == 2:
        idx = idx[:, 0]
    if idx.shape != (len(sources),):
        raise ValueError(f"apply_nearest: {len(sources)} sources, idx of shape {idx.shape}")
    if ((idx < -1) | (idx >= len(pool))).any():
        raise ValueError(f"apply_nearest: an index outside [-1, {len(pool)})")
    out, fallbacks = list(sources), []
    for i, j in enumerate(idx.tolist()):
        if j < 0:
            fallbacks.append(i)
        else:
            out[i] = pool[j]
    return out, fallbacks


def check_pairing(opt):
    """(pairing, match_pool) of an options namespace, validated; absent attributes are the defaults (random, self)"""
    pairing = getattr(opt, "pairing", None) or "random"
    pool = getattr(opt, "match_pool", None) or "self"
    if pairing not in PAIRINGS:
        raise ValueError(f"--pairing {pairing!r}: expected one of {' | '.join(PAIRINGS)}")
    if pool not in MATCH_POOLS:
        raise ValueError(f"--match_pool {pool!r}: expected one of {' | '.join(MATCH_POOLS)}")
    return pairing, pool


# ----------------------------------------------------------------------------- geometric augmentation: host-side maths
# THE place the matrices of --augment_geom are built (as ops.resize_joints is for the resize): float64 numpy, every
# function broadcasting over leading dimensions.  Conventions: a point is (u, v) = (x, y) in pixels; a 2x3 matrix
# [m00 m01 m02; m10 m11 m12] acts as u' = m00 u + m01 v + m02, v' = m10 u + m11 v + m12.
def _cos_sin_deg(theta_deg):
    """cos and sin of degrees, one libm call per element (an array routine may round differently from a scalar one, and a
    batch must get the matrix a whole epoch's table gets); multiples of 90 degrees are exact"""
    t = np.asarray(theta_deg, dtype=np.float64)
    c, s = np.empty(t.shape, np.float64), np.empty(t.shape, np.float64)
    exact = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0)}
    for i, d in np.ndenumerate(t):
        d = float(d)
        c[i], s[i] = exact.get(math.fmod(d, 360.0) % 360.0) or (math.cos(math.radians(d)), math.sin(math.radians(d)))
    return c, s


def affine_forward(theta_deg, scale, tx, ty, flip, src):
    """Forward map of one draw on the Hs x Ws source grid, float64 [..., 2, 3]: p' = c + t + s R(theta) F (p - c) with the
    centre c = ((Ws - 1) / 2, (Hs - 1) / 2), the shift t = (tx Ws, ty Hs) and F = diag(-1, 1) where `flip` is set."""
    Hs, Ws = int(src[0]), int(src[1])
    theta_deg, scale, tx, ty, flip = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (theta_deg, scale, tx, ty, flip)))
    cos, sin = _cos_sin_deg(theta_deg)
    f = np.where(flip != 0, -1.0, 1.0)
    m = np.empty(theta_deg.shape + (2, 3), np.float64)
    m[..., 0, 0], m[..., 0, 1] = scale * cos * f, -(scale * sin)
    m[..., 1, 0], m[..., 1, 1] = scale * sin * f, scale * cos
    cx, cy = (Ws - 1) / 2.0, (Hs - 1) / 2.0
    m[..., 0, 2] = cx + tx * Ws - (m[..., 0, 0] * cx + m[..., 0, 1] * cy)
    m[..., 1, 2] = cy + ty * Hs - (m[..., 1, 0] * cx + m[..., 1, 1] * cy)
    return m


def affine_inverse(fwd, src, dst=None):
    """The sampling matrix the kernels take, float64 [..., 2, 3]: output pixel (x, y) of the Ho x Wo grid -> source coordinate
    on the Hs x Ws grid = the inverse of (`fwd`, then the resize map u' = (u + 0.5) Wo / Ws - 0.5 of ops.resize_joints).
    Closed form on the 2x2 part; non-finite entries and a zero determinant are refused."""
    (Hs, Ws), (Ho, Wo) = (int(src[0]), int(src[1])), ((int(dst[0]), int(dst[1])) if dst is not None else (int(src[0]), int(src[1])))
    fwd = np.asarray(fwd, dtype=np.float64)
    if fwd.shape[-2:] != (2, 3):
        raise ValueError(f"affine_inverse: [..., 2, 3] expected, got {fwd.shape}")
    if not np.isfinite(fwd).all():
        raise ValueError("affine_inverse: a matrix with a non-finite entry")
    det = fwd[..., 0, 0] * fwd[..., 1, 1] - fwd[..., 0, 1] * fwd[..., 1, 0]
    if (det == 0.0).any() or not np.isfinite(1.0 / det).all():
        raise ValueError("affine_inverse: a singular matrix (determinant 0)")
    i00, i01, i10, i11 = fwd[..., 1, 1] / det, -fwd[..., 0, 1] / det, -fwd[..., 1, 0] / det, fwd[..., 0, 0] / det
    kx, ky = float(Ws) / float(Wo), float(Hs) / float(Ho)
    dx, dy = (0.5 * kx - 0.5) - fwd[..., 0, 2], (0.5 * ky - 0.5) - fwd[..., 1, 2]
    a = np.empty(fwd.shape, np.float64)
    a[..., 0, 0], a[..., 0, 1], a[..., 0, 2] = i00 * kx, i01 * ky, i00 * dx + i01 * dy
    a[..., 1, 0], a[..., 1, 1], a[..., 1, 2] = i10 * kx, i11 * ky, i10 * dx + i11 * dy
    if not np.isfinite(a).all():
        raise ValueError("affine_inverse: the inverse has a non-finite entry")
    return a


def affine_joints(uv, fwd, src, dst=None):
    """Joints [..., 21, 2 or 3] = (u, v[, depth]) of the source image on the output grid: through `fwd` ([2,3], or
    [..., 2, 3] with the joints' leading dimensions), then the resize map of ops.resize_joints; depth unchanged.  numpy in,
    numpy out, float64."""
    (Hs, Ws), (Ho, Wo) = (int(src[0]), int(src[1])), ((int(dst[0]), int(dst[1])) if dst is not None else (int(src[0]), int(src[1])))
    out = np.array(uv, dtype=np.float64, copy=True)
    m = np.asarray(fwd, dtype=np.float64)[..., None, :, :]          # one matrix for the 21 joints of an image
    u, v = out[..., 0].copy(), out[..., 1].copy()
    pu = (m[..., 0, 0] * u + m[..., 0, 1] * v) + m[..., 0, 2]
    pv = (m[..., 1, 0] * u + m[..., 1, 1] * v) + m[..., 1, 2]
    out[..., 0] = (pu + 0.5) * float(Wo) / float(Ws) - 0.5
    out[..., 1] = (pv + 0.5) * float(Ho) / float(Hs) - 0.5
    return out


def augment_draws(n_items, epoch, opt):
    """The draws of one epoch for the WHOLE dataset, float64 [n_items, 2, 5] = (theta in degrees, scale, tx, ty, flip) per item
    and side (0 = source, 1 = target), from one np.random.default_rng([aug_seed, epoch]).  Indexed by dataset item, so what an
    item gets in an epoch depends on nothing else - batch size, rank, world size, file or store.  --aug_pair shared: side 1
    is side 0."""
    rotate, scale, shift, flip, pair, seed = check_augment(opt)
    u = np.random.default_rng([int(seed), int(epoch)]).random((int(n_items), 2, 5))
    d = np.empty_like(u)
    d[..., 0] = (2.0 * u[..., 0] - 1.0) * rotate
    d[..., 1] = 1.0 + (2.0 * u[..., 1] - 1.0) * scale
    d[..., 2] = (2.0 * u[..., 2] - 1.0) * shift
    d[..., 3] = (2.0 * u[..., 3] - 1.0) * shift
    d[..., 4] = u[..., 4] < flip
    if pair == "shared":
        d[:, 1] = d[:, 0]
    return d


# ----------------------------------------------------------------------------- colour jitter: host-side maths
# train_hpe --augment_color.  The estimators' input is min-max normalised per image, which cancels any change of brightness or
# contrast that is one affine map of the three channels together; what is left to vary is what mixes channels (saturation,
# hue, per-channel gains) or is non-linear (gamma).  Matrices act on column vectors (R, G, B).
_LUMA = (0.299, 0.587, 0.114)
_HUE_K = ((0.0, -1.0, 1.0), (1.0, 0.0, -1.0), (-1.0, 1.0, 0.0))


def color_matrix(saturation, hue_deg, gains):
    """float64 [..., 3, 3] = diag(gains) @ Hue(hue_deg) @ Sat(saturation), broadcasting saturation [...], hue_deg [...] and
    gains [..., 3].  Sat(s) = s I + (1 - s) 1 [0.299 0.587 0.114] (towards the luma grey), Hue(h) = cos h I + (1 - cos h) / 3 11^T
    + sin h / sqrt(3) K with K = [[0,-1,1],[1,0,-1],[-1,1,0]] (a rotation about the grey axis).  Both are closed forms that are
    the exact identity at the neutral value (s = 1; h a multiple of 360), so (1, 0, (1,1,1)) gives the identity bit for bit."""
    gains = np.asarray(gains, dtype=np.float64)
    if gains.shape[-1:] != (3,):
        raise ValueError(f"color_matrix: gains [..., 3] expected, got {gains.shape}")
    s, h, g0 = np.broadcast_arrays(np.asarray(saturation, dtype=np.float64), np.asarray(hue_deg, dtype=np.float64), gains[..., 0])
    gains = np.broadcast_to(gains, s.shape + (3,))
    eye, ones, K = np.eye(3), np.ones((3, 3)), np.array(_HUE_K)
    cos, sin = _cos_sin_deg(h)
    s, cos, sin = s[..., None, None], cos[..., None, None], sin[..., None, None]
    sat = s * eye + (1.0 - s) * (np.ones((3, 1)) @ np.array([_LUMA]))
    hue = cos * eye + (1.0 - cos) / 3.0 * ones + sin / math.sqrt(3.0) * K
    return gains[..., :, None] * (hue @ sat)


def color_draws(n_items, epoch, opt):
    """The colour draws of one epoch for the WHOLE dataset, float64 [n_items, 6] = (saturation, hue in degrees, gain_R, gain_G,
    gain_B, gamma) per item, from np.random.default_rng([aug_seed, epoch, 1]): a stream of its own, so switching colour on does
    not change augment_draws' geometry and vice versa.  Indexed by dataset item, as augment_draws is.  s ~ U(1 - a, 1 + a)
    clipped at 0, h ~ U(-d, d), gain ~ U(1 - g, 1 + g), gamma = exp(U(-q, q))."""
    sat, hue, gain, gamma, seed = check_augment_color(opt)
    u = 2.0 * np.random.default_rng([int(seed), int(epoch), 1]).random((int(n_items), 6)) - 1.0
    d = np.empty_like(u)
    d[:, 0] = np.maximum(1.0 + u[:, 0] * sat, 0.0)
    d[:, 1] = u[:, 1] * hue
    d[:, 2:5] = 1.0 + u[:, 2:5] * gain
    d[:, 5] = np.exp(u[:, 5] * gamma)
    return d


class ResidentBatch:
    """One batch of a resident store: `idx` int32 [B,4] (a row block of the loader's device table) names the slots of
    (img1, img2, dep1, dep2) in `store` uint8 [S,Hs,Ws,3]; `uv_table` float64 [S,21,2] holds every slot's joints on the grid
    of `out_size` (the loader's --resize_inputs; None = the store's size).  ops.decode_inputs_indexed consumes it as it is.
    --augment_geom: `xf` float64 [B,2,6] and `uv` float64 [B,2,21,2] - row blocks of the epoch's tables - replace `uv_table`
    (ops.decode_inputs_indexed_affine)."""

    def __init__(self, store, idx, uv_table, out_size=None, xf=None, uv=None):
        self.store, self.idx, self.uv_table, self.out_size = store, idx, uv_table, out_size
        self.xf, self.uv = xf, uv
        self.B = int(idx.shape[0])

    def gather(self):
        """the four uint8 [B,Hs,Ws,3] tensors a raw batch carries (img1, img2, dep1, dep2), copied out of the store"""
        return tuple(self.store[self.idx[:, j].long()] for j in range(4))


class HandFolderLoader:
    """Iterable of RAW device batches over a prepared RHD / STB directory; `MMHandModel.set_input` decodes them on the
    device (keys img1, img2, dep1, dep2: uint8 [B,H,W,3] BGR as cv2.imread delivers them; uv1, uv2: float64 [B,21,2];
    C1, C2: float64 [B,21,3] = (u, v, depth / 700 * 255); H1_path, H2_path).  `decoded=True` yields the reference's own
    keys instead (H1, P1, D1, ... as NCHW fp32 views of the decoded buffers) for callers that want tensors; with
    --resize_inputs N those come out at N x N (the resize is part of the decode kernel's pass, ops.decode_inputs).

    Mirrors, by file:line of the reference:
      * image lists: RHD - every image of annotation folder "color", sorted by the integer file stem
        (rhd_dataset.py:25-37); STB - the "*_color_*" images of the non-"BB" cameras, sorted by (folder digit, folder
        letter, frame number) (stb_dataset.py:24-41);
      * the split (generic_dataset.py:100-131): sep = int((1 - ratio) * n); a root with "test" in its path serves all of
        it (and refuses training); training takes [sep:], generation [:sep]; targets in sorted order, sources = the
        same list shuffled with Python's `random` (the generator one image is drawn FROM, the other TO);
      * labels (generic_dataset.py:204-210), the depth file = the colour path with "color" -> "depth" (:147-148);
      * batching (mmhand_dataset_data_loader.py:22-48): in order, no shuffle; under --distributed a
        DistributedSampler with its defaults (shuffle with seed 0, the epoch never advanced, padded to a multiple of the
        world size, rank r takes r, r + world, ...); the last batch may be short; iteration stops after
        `max_dataset_size` BATCHES (the reference compares the batch index with it)."""

    def __init__(self, opt, device=None, decoded=False, threads=None, device_png=None, resident=None):
        self.opt = opt
        # --resize_inputs N: the decoded form (decoded=True) comes out at N x N (joints in C1 / C2 scaled with it); the raw
        # form always travels at the files' size - MMHandModel.set_input resizes inside its decode pass
        self.out_size = check_resize_inputs(opt) or None
        self.root_dir = opt.dataroot
        if not self.root_dir or not os.path.isfile(os.path.join(self.root_dir, "annotation.pickle")):
            raise FileNotFoundError(f"--dataroot {self.root_dir!r}: no annotation.pickle (the directory create_RHD_DB.py / "
                                    "create_STB_DB.py of the reference prepare)")
        with open(os.path.join(self.root_dir, "annotation.pickle"), "rb") as fh:
            self.annotations = pickle.load(fh)
        kind = (getattr(opt, "dataset", None) or "rhd").lower()
        if kind == "rhd":
            data = [os.path.join(self.root_dir, folder, image) for folder in self.annotations
                    for image in self.annotations[folder] if folder == "color"]
            key = lambda x: int(x.split("/")[-1][0:-4])                                        # noqa: E731
        elif kind == "stb":
            data = []
            for folder in self.annotations:
                for image in self.annotations[folder]:
                    camera, spec, _ = image.split("_")
                    if camera != "BB" and spec == "color":
                        data.append(os.path.join(self.root_dir, folder, image))

            def key(x):
                *_, folder, name = x.split("/")
                return int(folder[1]), folder[2], int(name[0:-4].split("_")[-1])
        else:
            raise NotImplementedError(f"--dataset {kind}: HandFolderLoader reads the prepared 'rhd' and 'stb' directories "
                                      "(the pair-list format of data/mmhand_dataset.py is not supported)")
        ratio = getattr(opt, "augmentation_ratio", None)
        self.pairing, self.match_pool = check_pairing(opt)
        self.image_source, self.image_target = self._get_src_tgt(0.0 if ratio is None else float(ratio), data, key)
        self._all_images, self._ratio = data, 0.0 if ratio is None else float(ratio)       # `data` is sorted by now
        self.device = device or torch.device("cuda", getattr(opt, "local_rank", 0) or 0)
        # --pairing curriculum | nearest: decided here, once (see _pair); `pair_distance` = float64 [n] in loader order, in
        # random mode computed on first access only; `pairing_fallbacks` = the targets `nearest` found no neighbour for
        self.pairing_fallbacks = []
        self._pair_distance = None
        # --augment_geom: the validated ranges (None = off), the epoch number of the draws (set_epoch; nothing else reads it)
        # and the dataset item of every loader position - the target's place in the split's sorted list, which the curriculum's
        # reordering carries along, so an item's transform does not depend on the pairing order
        self.augment = check_augment(opt)
        # --depth_source joints: (radius, bg) of the render that replaces the depth files, None = files
        self.render = check_depth_source(opt)
        self.image_keys = _IMAGE_KEYS if self.render is None else _IMAGE_KEYS[:2]
        self.aug_epoch = 0
        self.aug_item = np.arange(len(self.image_target), dtype=np.int64)
        self._aug_draws = None
        if self.pairing != "random":
            self._pair(data, 0.0 if ratio is None else float(ratio))
        self.decoded = decoded
        self.world = (getattr(opt, "world_size", 1) or 1) if getattr(opt, "distributed", False) else 1
        self.rank = torch.distributed.get_rank() if (self.world > 1 and torch.distributed.is_initialized()) else 0
        self.threads = int(threads if threads is not None else (getattr(opt, "nThreads", 4) or 1))
        self.epoch = 0          # the reference never calls sampler.set_epoch: the permutation is the same every epoch
        self.name = type(self).__name__
        # opt-in: PNG bytes to the device (png.py).  Two buffer sets take turns, so a batch's raw tensors stay valid until the
        # loader has yielded two more; `png_fallbacks` lists (path, reason) of every file PIL decoded instead
        if device_png is None:
            device_png = bool(getattr(opt, "device_png", False)) or os.environ.get("MMH_DEVICE_PNG", "0") == "1"
        self.device_png = bool(device_png)
        self.png_fallbacks = []
        self._png_sets = self._png_stream = self._png_prev = None
        self._png_turn = 0
        # opt-in: the decoded dataset stays on the device (see the module docstring); "off: <reason>" = asked for and refused
        if resident is None:
            resident = bool(getattr(opt, "resident_dataset", False)) or os.environ.get("MMH_RESIDENT_DATASET", "0") == "1"
        self.resident_state = "off"
        self._res = None
        if resident:
            self._resident_setup()

    def _get_src_tgt(self, ratio, data, sort_fn):
        assert len(data) > 0, "no images listed in annotation.pickle for this --dataset"
        data.sort(key=sort_fn)
        sep_pnt = int((1 - ratio) * len(data))
        if "test" in self.root_dir:
            assert not self.opt.isTrain, "a 'test' directory serves generation only (generic_dataset.py:116-118)"
            tgt = data
        else:
            tgt = data[sep_pnt:] if self.opt.isTrain else data[:sep_pnt]
        src = tgt.copy()
        random.shuffle(src)
        return src, tgt

    # ------------------------------------------------------------------ pose-distance pairing
    def pose_of(self, image_path):
        """float64 [21,3] = (u, v, depth / 700 * 255) of an image, at the files' own size: what load_sample hands out as C1 / C2
        (--resize_inputs does not touch it, so the pairing does not depend on that flag)"""
        a = self.get_labels(image_path)
        uv = np.asarray(a["uv_coord"], dtype=np.float64).reshape(21, 2)
        z = np.expand_dims(np.asarray(a["depth"], dtype=np.float64), -1) / 700.0 * 255
        return np.concatenate([uv, z], axis=-1)

    def _features(self, paths):
        poses = np.stack([self.pose_of(p) for p in paths])
        return ops.pose_features(torch.from_numpy(poses).to(self.device).contiguous())

    def _distances(self):
        """pose distance of every (source, target) pair in the lists' present order, float64 [n] on the host"""
        with torch.cuda.device(self.device):
            d = ops.pose_pair_distance(self._features(self.image_source), self._features(self.image_target))
            return d.cpu().numpy()

    @property
    def pair_distance(self):
        if self._pair_distance is None:
            self._pair_distance = self._distances()
        return self._pair_distance

    def _pair(self, data, ratio):
        """curriculum: the random pairs as they are, fed from the smallest pose distance to the largest.  nearest: the source
        of every target is its nearest pose in the pool - the targets themselves without the target (self), or the training
        share data[sep:] of the same root (train; `data` is the sorted list _get_src_tgt cut)."""
        if self.pairing == "curriculum":
            d = self._distances()
            order = curriculum_order(d)
            self.image_source = [self.image_source[i] for i in order]
            self.image_target = [self.image_target[i] for i in order]
            self.aug_item = self.aug_item[order]
            self._pair_distance = d[order]
            return
        pool = self.match_pool_paths(self.match_pool)
        with torch.cuda.device(self.device):
            q = self._features(self.image_target)
            c = q if pool is self.image_target else self._features(pool)
            exclude = torch.arange(len(pool), dtype=torch.int32, device=self.device) if pool is self.image_target else None
            idx, _ = ops.pose_knn(q, c, 1, exclude=exclude)
            idx = idx.cpu().numpy()
        self.image_source, self.pairing_fallbacks = apply_nearest(self.image_source, pool, idx)
        self._pair_distance = self._distances()

    def match_pool_paths(self, match_pool):
        """the candidates of a nearest-pose search: the loader's own targets (self; the list object itself, so callers can
        tell) or the training share of the same root (train; the sorted list _get_src_tgt cut)"""
        if match_pool != "train":
            return self.image_target
        data, ratio = self._all_images, self._ratio
        if "test" in self.root_dir:
            raise ValueError(f"--match_pool train: {self.root_dir!r} is a 'test' directory, it has no training share")
        if self.opt.isTrain:
            raise ValueError("--match_pool train serves a generation split (isTrain False): a training loader's targets "
                             "ARE the training share (--match_pool self)")
        pool = data[int((1 - ratio) * len(data)):]
        if not pool:
            raise ValueError(f"--match_pool train: --augmentation_ratio {ratio} leaves no training share in {self.root_dir!r}")
        return pool

    def get_labels(self, image_path):
        *_, folder, name = image_path.split("/")
        if "joints" in name:
            parts = name.split("_")
            name = parts[0] + "_" + parts[1] + "_" + parts[-1]
        return self.annotations[folder][name]

    def set_epoch(self, epoch):
        """the epoch number of --augment_geom's draws, and nothing else: the reference's sampler stays at epoch 0 (see the
        class docstring), so indices() - and with it the order, the pairs and the resident store - does not see it"""
        self.aug_epoch = int(epoch)

    # ------------------------------------------------------------------ geometric augmentation
    def _draws(self):
        """this epoch's draws for the whole dataset, computed once per epoch number"""
        if self._aug_draws is None or self._aug_draws[0] != self.aug_epoch:
            self._aug_draws = (self.aug_epoch, augment_draws(len(self.image_target), self.aug_epoch, self.opt))
        return self._aug_draws[1]

    def _augment_rows(self, items, uv, c, src):
        """items: loader positions [n]; uv float64 [n,2,21,2] and c [n,2,21,3]: the joints of each position's (source, target)
        at the files' size src = (Hs, Ws) -> (xf [n,2,6] for the kernels, uv and c on the output grid).  One batch or a whole
        epoch's table: the same arithmetic per element, so the two agree bit for bit."""
        d = self._draws()[self.aug_item[np.asarray(items, dtype=np.int64)]]
        fwd = affine_forward(d[..., 0], d[..., 1], d[..., 2], d[..., 3], d[..., 4], src)
        dst = ops.resize_size(self.out_size, src) or src
        xf = affine_inverse(fwd, src, dst).reshape(len(d), 2, 6)
        return np.ascontiguousarray(xf), affine_joints(uv, fwd, src, dst), affine_joints(c, fwd, src, dst)

    def indices(self):
        n = len(self.image_source)
        if self.world <= 1:
            return list(range(n))
        if self.pairing == "curriculum":
            # no permutation: the padded range, rank-strided, so that all ranks step through the same difficulty together
            total = -(-n // self.world) * self.world
            idx = list(range(n))
            idx += (idx * -(-(total - n) // n))[:total - n]
            return idx[self.rank:total:self.world]
        g = torch.Generator().manual_seed(0 + self.epoch)
        idx = torch.randperm(n, generator=g).tolist()
        total = -(-n // self.world) * self.world
        pad = total - n
        idx += idx[:pad] if pad <= len(idx) else (idx * -(-pad // len(idx)))[:pad]      # DistributedSampler's wrap-around padding
        return idx[self.rank:total:self.world]

    def n_batches(self):
        B = self.opt.batchSize
        return -(-len(self.indices()) // B)

    def __len__(self):
        return min(len(self.image_source), self.opt.max_dataset_size)

    def load_sample(self, item):
        """host side of generic_dataset.py:133-180 for ONE pair: file reads only - the arithmetic is the device's"""
        h_1, h_2 = self.image_source[item], self.image_target[item]
        a1, a2 = self.get_labels(h_1), self.get_labels(h_2)
        uv1 = np.asarray(a1["uv_coord"], dtype=np.float64).reshape(21, 2)
        uv2 = np.asarray(a2["uv_coord"], dtype=np.float64).reshape(21, 2)
        z1 = np.expand_dims(np.asarray(a1["depth"], dtype=np.float64), -1) / 700.0 * 255
        z2 = np.expand_dims(np.asarray(a2["depth"], dtype=np.float64), -1) / 700.0 * 255
        if self.augment is not None:
            return self._load_augmented(item, h_1, h_2, uv1, uv2, np.concatenate([uv1, z1], axis=-1), np.concatenate([uv2, z2], axis=-1))
        if self.render is not None:         # --depth_source joints: two files per pair, no depth path is touched
            read = _read_bytes if self.device_png else _read_bgr
            return dict(img1=read(h_1), img2=read(h_2), uv1=uv1, uv2=uv2, C1=np.concatenate([uv1, z1], axis=-1),
                        C2=np.concatenate([uv2, z2], axis=-1), H1_path=h_1, H2_path=h_2)
        if self.device_png:
            return dict(img1=_read_bytes(h_1), img2=_read_bytes(h_2), dep1=_read_bytes(h_1.replace("color", "depth")),
                        dep2=_read_bytes(h_2.replace("color", "depth")), uv1=uv1, uv2=uv2,
                        C1=np.concatenate([uv1, z1], axis=-1), C2=np.concatenate([uv2, z2], axis=-1), H1_path=h_1, H2_path=h_2)
        return dict(img1=_read_bgr(h_1), img2=_read_bgr(h_2), dep1=_read_bgr(h_1.replace("color", "depth")),
                    dep2=_read_bgr(h_2.replace("color", "depth")), uv1=uv1, uv2=uv2,
                    C1=np.concatenate([uv1, z1], axis=-1), C2=np.concatenate([uv2, z2], axis=-1), H1_path=h_1, H2_path=h_2)

    def _load_augmented(self, item, h_1, h_2, uv1, uv2, c1, c2):
        """load_sample under --augment_geom: the same files, untouched; the sample's two sampling matrices ride along as `xf`
        [2,6] and uv1 / uv2 / C1 / C2 leave already transformed, on the output grid"""
        read = _read_bytes if self.device_png else _read_bgr
        s = dict(img1=read(h_1), img2=read(h_2), H1_path=h_1, H2_path=h_2)
        if self.render is None:
            s.update(dep1=read(h_1.replace("color", "depth")), dep2=read(h_2.replace("color", "depth")))
        src = png_size(h_1) if self.device_png else s["img1"].shape[:2]
        if src is None:
            raise ValueError(f"--augment_geom --device_png: {h_1} is not a PNG file, its size is unknown before the decode")
        xf, uv, c = self._augment_rows([item], np.stack([uv1, uv2])[None], np.stack([c1, c2])[None], src)
        s.update(xf=xf[0], uv1=uv[0, 0], uv2=uv[0, 1], C1=c[0, 0], C2=c[0, 1])
        return s

    def _collate(self, samples):
        out = {}
        if self.device_png:
            from .png import PngBatchDecoder
            if self._png_sets is None:
                self._png_sets = [PngBatchDecoder(self.device), PngBatchDecoder(self.device)]
            dec = self._png_sets[self._png_turn % 2]
            self._png_turn += 1
            out["_png"] = (dec, dec.pack([s[k] for k in self.image_keys for s in samples]))
        keys = ("uv1", "uv2", "C1", "C2") if self.device_png else self.image_keys + ("uv1", "uv2", "C1", "C2")
        for k in keys + (("xf",) if self.augment is not None else ()):
            t = torch.from_numpy(np.stack([s[k] for s in samples]))
            out[k] = t.pin_memory() if torch.cuda.is_available() else t
        out["H1_path"] = [s["H1_path"] for s in samples]
        out["H2_path"] = [s["H2_path"] for s in samples]
        return out

    def host_batches(self, only=None):
        """pinned host batches in loader order, file reads on a thread pool, one batch prepared ahead; `only`: the numbers of
        the batches to prepare (the resident loader's batches that still need their files), all of them when None"""
        from concurrent.futures import ThreadPoolExecutor
        groups = _batch_groups(self.indices(), self.opt.batchSize, self.opt.max_dataset_size)
        if only is not None:
            groups = [groups[g] for g in only]
        if not groups:
            return
        if self.augment is not None:
            self._draws()                   # once, here: not by whichever worker thread asks first
        with ThreadPoolExecutor(max_workers=max(1, self.threads)) as pool:
            nxt = [pool.submit(self.load_sample, i) for i in groups[0]]
            for gi in range(len(groups)):
                cur = nxt
                nxt = [pool.submit(self.load_sample, i) for i in groups[gi + 1]] if gi + 1 < len(groups) else []
                yield self._collate([f.result() for f in cur])

    def _png_to_device(self, hb):
        """upload + mmh_png_decode_batch on the loader's own stream (beside whatever the consumer still has queued), the
        four image tensors as views of the set's output buffer"""
        dec, plan = hb["_png"]
        cur = torch.cuda.current_stream(self.device)
        if self._png_stream is None:
            self._png_stream = torch.cuda.Stream(self.device)
        if self._png_prev is not None:
            # everything queued before the previous batch was handed out - the consumers of the batch this set held - is done
            self._png_stream.wait_event(self._png_prev)
        self._png_prev = torch.cuda.Event()
        self._png_prev.record(cur)
        pix, report = dec.launch(plan, bgr=True, stream=self._png_stream)
        cur.wait_stream(self._png_stream)
        B = len(hb["H1_path"])
        for i, reason in report:
            path = (hb["H1_path"] if i // B in (0, 2) else hb["H2_path"])[i % B]
            self.png_fallbacks.append((path.replace("color", "depth") if i // B >= 2 else path, reason))
        return {k: pix[j * B:(j + 1) * B] for j, k in enumerate(self.image_keys)}

    def to_device(self, hb, fill=None):
        out = {k: (v.to(self.device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in hb.items() if k != "_png"}
        if "_png" in hb:
            out = {**self._png_to_device(hb), **out}
        if fill is not None:
            self._fill(fill, out)
        if not self.decoded:
            return out
        src = tuple(out["img1"].shape[1:3])
        dst = ops.resize_size(self.out_size, src)
        # --depth_source joints: the colour images stand in the depth arguments, the render below overwrites what comes of it
        dep1, dep2 = (out[k] for k in (("dep1", "dep2") if self.render is None else ("img1", "img2")))
        if "xf" in out:                     # --augment_geom: joints and C arrive transformed, on the output grid
            xh1, xh2, xp, xd = ops.decode_inputs_affine(out["img1"], out["img2"], dep1, dep2, out["uv1"],
                                                        out["uv2"], out["xf"], out_size=dst)
            c1, c2 = out["C1"], out["C2"]
        else:
            xh1, xh2, xp, xd = ops.decode_inputs(out["img1"], out["img2"], dep1, dep2, out["uv1"], out["uv2"],
                                                 out_size=dst)
            c1, c2 = (out[k] if dst is None else ops.resize_joints(out[k], src, dst) for k in ("C1", "C2"))
        self._render(c1, c2, xd)
        v = ops.nhwc_to_nchw_view
        return {"H1": v(xh1, 3), "H2": v(xh2, 3), "P1": v(xp)[:, :21], "P2": v(xp)[:, 21:42], "D1": v(xd)[:, :3],
                "D2": v(xd)[:, 3:6], "C1": c1, "C2": c2, "H1_path": out["H1_path"], "H2_path": out["H2_path"]}

    def _render(self, c1, c2, xd):
        """--depth_source joints: D1 / D2 of the decoded form, rendered into x_d from the batch's own C1 / C2 (one launch)"""
        if self.render is not None:
            ops.render_pose_depth(c1.contiguous(), c2.contiguous(), radius=self.render[0], bg=self.render[1], out=xd)

    # ------------------------------------------------------------------ resident dataset
    def _resident_setup(self):
        """plan, budget decision, store and tables; leaves `resident_state` "on" or "off: <reason>" (then nothing else differs
        from a loader without the flag)"""
        paths, table = resident_plan(self.image_source, self.image_target, self.indices(), self.opt.batchSize,
                                     self.opt.max_dataset_size, depth_source="files" if self.render is None else "joints")
        size = png_size(paths[0]) if paths else None
        if size is None:
            state = "off: no batches" if not paths else f"off: {paths[0]} is not a PNG file"
        else:
            free = torch.cuda.mem_get_info(self.device)[0]
            budget = int(float(getattr(self.opt, "resident_gb", 64.0)) * 1e9)
            need, state = resident_decision(len(paths), size[0], size[1], budget, free)
        self.resident_state = state
        if state != "on":
            print(f"{self.name}: --resident_dataset {state}; batches keep coming from the files")
            return
        check_table(table, len(paths))
        Hs, Ws = size
        S, dev = len(paths), self.device
        uv, c = np.zeros((S, 21, 2), np.float64), np.zeros((S, 21, 3), np.float64)
        colour = set(self.image_source) | set(self.image_target)
        for slot, path in enumerate(paths):
            if path in colour:                          # the depth twins' rows are never read
                a = self.get_labels(path)
                uv[slot] = np.asarray(a["uv_coord"], dtype=np.float64).reshape(21, 2)
                c[slot] = np.concatenate([uv[slot], np.expand_dims(np.asarray(a["depth"], dtype=np.float64), -1) / 700.0 * 255], -1)
        uv0, c0 = uv, c                                 # at the files' size, on the host: what --augment_geom transforms per epoch
        uv, c = torch.from_numpy(uv).to(dev), torch.from_numpy(c).to(dev)
        dst = ops.resize_size(self.out_size, size)
        if dst is not None:                             # joints are scaled in ONE place, once
            uv, c = ops.resize_joints(uv, size, dst), ops.resize_joints(c, size, dst)
        self._res = dict(paths=paths, table=table, lengths=table_lengths(table), filled=np.zeros(S, dtype=bool), size=size,
                         store=torch.empty((S, Hs, Ws, 3), dtype=torch.uint8, device=dev), uv=uv.contiguous(),
                         c=c.contiguous(), table_dev=torch.from_numpy(table).to(dev), uv0=uv0, c0=c0, aug=None)
        self.resident_state = f"on: {S} images of {Hs} x {Ws}, {need} bytes"

    def _resident_epoch_tables(self):
        """--augment_geom on the resident path, at the top of an epoch: the epoch's xf [N,2,6], uv [N,2,21,2] and c [N,2,21,3]
        for this rank's N samples in loader order, built on the host and uploaded once; batch g is rows first[g] .. + its
        length, so serving it stays one kernel and no upload"""
        r = self._res
        if r["aug"] is not None and r["aug"]["epoch"] == self.aug_epoch:
            return
        groups = _batch_groups(self.indices(), self.opt.batchSize, self.opt.max_dataset_size)
        items = np.array([i for g in groups for i in g], dtype=np.int64)
        rows = np.concatenate([r["table"][g, :n] for g, n in enumerate(r["lengths"])])          # [N,4] slots
        xf, uv, c = self._augment_rows(items, r["uv0"][rows[:, :2]], r["c0"][rows[:, :2]], r["size"])
        first = np.concatenate([[0], np.cumsum(r["lengths"])]).astype(np.int64)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)                  # noqa: E731
        r["aug"] = dict(epoch=self.aug_epoch, xf=t(xf), uv=t(uv), c=t(c), first=first)

    def _batch_is_resident(self, g):
        r = self._res
        return bool(r["filled"][r["table"][g, : r["lengths"][g]]].all())

    def _fill(self, g, out):
        """copy a batch that came from the files into the store, on the current stream - behind the batch's upload (or the
        wait for the PNG stream) and in front of whatever reads the store later on this stream.  Images already resident, and
        a file's second appearance in the batch, get slot -1; images of another size than the store's never enter it."""
        r = self._res
        n = r["lengths"][g]
        if tuple(out["img1"].shape) != (n,) + r["size"] + (3,):
            return
        slots = r["table"][g, :n].T.copy()              # [4, n]: one row per image key
        fresh = ~r["filled"][slots]
        _, first = np.unique(slots.ravel(), return_index=True)
        once = np.zeros(slots.size, dtype=bool)
        once[first] = True
        fresh &= once.reshape(slots.shape)
        if not fresh.any():
            return
        dev_slots = torch.from_numpy(np.where(fresh, slots, -1).astype(np.int32)).to(self.device)
        for j, k in enumerate(_IMAGE_KEYS):
            if fresh[j].any():              # (--depth_source joints: the depth columns repeat the colour slots, never fresh)
                ops.store_images(out[k].contiguous(), dev_slots[j], r["store"])
        r["filled"][slots[fresh]] = True

    def _serve(self, g):
        """batch g out of the store: no host work beyond this dictionary"""
        r = self._res
        n = r["lengths"][g]
        idx = r["table_dev"][g, :n]
        p1, p2 = ([r["paths"][s] for s in r["table"][g, :n, j]] for j in (0, 1))
        if self.augment is not None:
            a = r["aug"]
            o = int(a["first"][g])
            c1, c2 = a["c"][o:o + n, 0], a["c"][o:o + n, 1]
            rb = ResidentBatch(r["store"], idx, r["uv"], self.out_size, xf=a["xf"][o:o + n], uv=a["uv"][o:o + n])
        else:
            c1, c2 = r["c"][idx[:, 0].long()], r["c"][idx[:, 1].long()]
            rb = ResidentBatch(r["store"], idx, r["uv"], self.out_size)
        if not self.decoded:
            return {"resident": rb, "C1": c1, "C2": c2, "H1_path": p1, "H2_path": p2}
        if rb.xf is not None:
            xh1, xh2, xp, xd = ops.decode_inputs_indexed_affine(rb.store, rb.idx, rb.uv, rb.xf, out_size=rb.out_size)
        else:
            xh1, xh2, xp, xd = ops.decode_inputs_indexed(rb.store, rb.idx, rb.uv_table, out_size=rb.out_size)
        self._render(c1, c2, xd)
        v = ops.nhwc_to_nchw_view
        return {"H1": v(xh1, 3), "H2": v(xh2, 3), "P1": v(xp)[:, :21], "P2": v(xp)[:, 21:42], "D1": v(xd)[:, :3],
                "D2": v(xd)[:, 3:6], "C1": c1, "C2": c2, "H1_path": p1, "H2_path": p2}

    def __iter__(self):
        if self._res is None:
            for hb in self.host_batches():
                yield self.to_device(hb)
            return
        # decided once per epoch: the batches whose slots are all filled come out of the store, the others take the file
        # path unchanged and fill it on their way
        n_batches = len(self._res["lengths"])
        todo = [g for g in range(n_batches) if not self._batch_is_resident(g)]
        if self.augment is not None and len(todo) < n_batches:
            self._resident_epoch_tables()
        from_files = self.host_batches(only=todo)
        todo = set(todo)
        try:
            for g in range(n_batches):
                yield self.to_device(next(from_files), fill=g) if g in todo else self._serve(g)
        finally:
            from_files.close()              # the thread pool goes with its last batch, not with the garbage collector


def make_loader(opt, synthetic_samples=256, device=None):
    """--dataroot given: the prepared directory; else synthetic batches (train.py:15-17's CreateDataLoader)"""
    if getattr(opt, "dataroot", None):
        return HandFolderLoader(opt, device=device)
    return SyntheticHandLoader(opt, synthetic_samples, device=device)
