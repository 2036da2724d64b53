"""The float64 numpy oracle of the pose distance (nearest_neighbor_search.py:68-83 with the clamp), shared by
tests/test_pose_pairing_cpu.py - which checks it against the reference's recorded distances - and tests/test_pose_pairing_gpu.py."""
import numpy as np


def oracle_features(poses):
    """the 20 consecutive joint differences of [N,21,3] poses, flattened and divided by their 2-norm -> [N,60]"""
    d = (poses[:, 1:] - poses[:, :-1]).reshape(len(poses), 60)
    with np.errstate(invalid="ignore", divide="ignore"):
        return d / np.linalg.norm(d, axis=1, keepdims=True)


def oracle_valid(poses):
    finite = np.isfinite(poses.reshape(len(poses), -1)).all(1)
    p = np.where(finite[:, None, None], poses, 0.0)
    return finite & (np.linalg.norm((p[:, 1:] - p[:, :-1]).reshape(len(p), 60), axis=1) > 0)


def oracle_distance(cos):
    return np.arccos(np.clip(cos, -1.0, 1.0)) / np.pi


def draw_poses(n, seed, size=32):
    """poses as tests/_dataset_fixture.write_rhd draws its labels and the loader forms C1 / C2: (u, v, depth / 700 * 255)"""
    rs = np.random.RandomState(seed)
    uv = rs.uniform(-4, size + 4, size=(n, 21, 2))
    z = rs.uniform(100, 690, size=(n, 21, 1)) / 700.0 * 255
    return np.concatenate([uv, z], axis=-1)


def oracle_knn(q_poses, c_poses, k, exclude=None):
    """-> (idx [Nq,k] int64, cos [Nq,k], sorted cosines of the valid candidates per query): ranked by (-cos, index); invalid
    candidates and exclude[q] never appear; an invalid query and the slots past the valid candidates are -1 / NaN"""
    fq, fc = np.nan_to_num(oracle_features(q_poses)), np.nan_to_num(oracle_features(c_poses))
    vq, vc = oracle_valid(q_poses), oracle_valid(c_poses)
    # identical candidates get identical cosines, whatever the matrix product does at its block edges
    uniq, inv = np.unique(fc, axis=0, return_inverse=True)
    cos = (fq @ uniq.T)[:, inv.reshape(-1)]
    idx = np.full((len(fq), k), -1, dtype=np.int64)
    out = np.full((len(fq), k), np.nan)
    ranked = []
    for q in range(len(fq)):
        ok = vc.copy()
        if exclude is not None and exclude[q] >= 0:
            ok[exclude[q]] = False
        cand = np.nonzero(ok)[0] if vq[q] else np.zeros(0, dtype=np.int64)
        order = cand[np.lexsort((cand, -cos[q, cand]))]
        ranked.append(cos[q, order])
        n = min(k, len(order))
        idx[q, :n] = order[:n]
        out[q, :n] = cos[q, order[:n]]
    return idx, out, ranked
