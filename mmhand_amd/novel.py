"""Host side of `aug --novel K`: poses that are not in the dataset, and the prepared directory the generated images go to.

Every target t of the generation split is blended with each of its K nearest poses nb_1 .. nb_K of the pool (the reference's
pose distance; ops.pose_features / ops.pose_knn, t itself excluded):

    uv = (1 - A) * uv_t + A * uv_nb          depth = (1 - A) * depth_t + A * depth_nb

in float64 numpy on the raw annotation values.  The images go to <dst>/color/<number>.png, numbered consecutively in (target,
rank) order, with <dst>/annotation.pickle = {"color": {name: {"uv_coord": [21][2], "depth": [21]}}} (uv_coord on the written
image's grid, depth raw) - the prepared RHD layout, so `train --dataroot <dst> --dataset rhd --depth_source joints` reads it -
and <dst>/novel_index.json, one record per file.  Everything here is pure host code; nothing draws a random number, so two
runs write the same bytes."""
import json
import os
import pickle

import numpy as np

NOVEL_K_MAX = 15


def check_novel(k, alpha):
    """(K, A) validated: K an integer in 1 .. 15 (ops.pose_knn serves 16, one of them may be the excluded target), A a
    finite number in (0, 1]"""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= NOVEL_K_MAX:
        raise ValueError(f"--novel {k!r}: expected an integer in 1 .. {NOVEL_K_MAX}")
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not (0.0 < float(alpha) <= 1.0):
        raise ValueError(f"--novel_alpha {alpha!r}: expected a number in (0, 1]")
    return int(k), float(alpha)


def blend(uv_t, depth_t, uv_nb, depth_nb, alpha):
    """the new pose: float64 ([21,2], [21]) = (1 - A) * target + A * neighbour, on the raw annotation values"""
    a = np.float64(alpha)
    uv_t, uv_nb = (np.asarray(x, dtype=np.float64).reshape(21, 2) for x in (uv_t, uv_nb))
    d_t, d_nb = (np.asarray(x, dtype=np.float64).reshape(21) for x in (depth_t, depth_nb))
    return (1.0 - a) * uv_t + a * uv_nb, (1.0 - a) * d_t + a * d_nb


def file_name(number):
    """consecutive integers, zero-padded to at least five digits"""
    return f"{int(number):05d}.png"


def plan(targets, pool, labels_of, idx, dist, k, alpha):
    """targets, pool: lists of image paths; labels_of(path) -> {"uv_coord", "depth"}; idx int [n, >= k], dist float64 [n, >= k]
    = ops.pose_knn's result for the targets against the pool (-1 / NaN = no such neighbour) -> (records, fallbacks).
    A record = dict(file, target, neighbour, rank, alpha, pose_distance, uv [21,2], depth [21]) with uv and depth at the
    files' size; `fallbacks` lists the positions of the targets that got fewer than k neighbours (as
    HandFolderLoader.pairing_fallbacks lists those `nearest` found none for)."""
    k, alpha = check_novel(k, alpha)
    idx, dist = np.asarray(idx), np.asarray(dist, dtype=np.float64)
    if idx.ndim != 2 or idx.shape[0] != len(targets) or idx.shape[1] < k or dist.shape != idx.shape:
        raise ValueError(f"novel.plan: {len(targets)} targets, k = {k}, idx {idx.shape}, dist {dist.shape}")
    if ((idx < -1) | (idx >= len(pool))).any():
        raise ValueError(f"novel.plan: an index outside [-1, {len(pool)})")
    records, fallbacks = [], []
    for i, t in enumerate(targets):
        lt = labels_of(t)
        got = 0
        for r in range(k):
            j = int(idx[i, r])
            if j < 0:
                continue
            ln = labels_of(pool[j])
            uv, depth = blend(lt["uv_coord"], lt["depth"], ln["uv_coord"], ln["depth"], alpha)
            records.append(dict(file=file_name(len(records)), target=t, neighbour=pool[j], rank=r + 1, alpha=alpha,
                                pose_distance=float(dist[i, r]), uv=uv, depth=depth))
            got += 1
        if got < k:
            fallbacks.append(i)
    return records, fallbacks


def resize_uv(uv, src, dst):
    """joints of an Hs x Ws image on the grid of its Ho x Wo resize - ops.resize_joints' map, in float64 numpy"""
    if src is None or dst is None or tuple(dst) == tuple(src):
        return np.array(uv, dtype=np.float64, copy=True)
    (Hs, Ws), (Ho, Wo) = src, dst
    out = np.array(uv, dtype=np.float64, copy=True)
    out[..., 0] = (out[..., 0] + 0.5) * float(Wo) / float(Ws) - 0.5
    out[..., 1] = (out[..., 1] + 0.5) * float(Ho) / float(Hs) - 0.5
    return out


def write_annotation(dst, records, src=None, out=None):
    """<dst>/annotation.pickle in the prepared RHD layout; uv_coord on the written image's grid (src = the files' size, out =
    the size the PNGs are written at; both None = no resize), depth raw.  Plain lists of Python floats, a fixed protocol."""
    ann = {"color": {r["file"]: {"uv_coord": resize_uv(r["uv"], src, out).tolist(),
                                 "depth": np.asarray(r["depth"], dtype=np.float64).tolist()} for r in records}}
    os.makedirs(dst, exist_ok=True)
    with open(os.path.join(dst, "annotation.pickle"), "wb") as fh:
        pickle.dump(ann, fh, protocol=4)
    return ann


def write_index(dst, records, root=None):
    """<dst>/novel_index.json: one record per file, {file, target, neighbour, rank, alpha, pose_distance}; target and
    neighbour relative to `root` (the dataset's directory) when one is given"""
    rows = [{k: r[k] for k in ("file", "target", "neighbour", "rank", "alpha", "pose_distance")} for r in records]
    if root is not None:
        for row in rows:
            row["target"], row["neighbour"] = (os.path.relpath(row[k], root) for k in ("target", "neighbour"))
    os.makedirs(dst, exist_ok=True)
    with open(os.path.join(dst, "novel_index.json"), "w") as fh:
        json.dump(rows, fh, indent=1)
        fh.write("\n")
    return rows
