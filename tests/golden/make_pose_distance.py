"""Writes tests/golden/pose_distance.npz: 24 poses and their 24 x 24 matrix of the REFERENCE's pose distance.

    python tests/golden/make_pose_distance.py <reference checkout>

`poseDistance` (nearest_neighbor_search/nearest_neighbor_search.py:68-83) is pulled out of the reference's file with `ast`
and only that function is executed: the module itself loads a dataset when it is imported, so it is never imported.  Only
the poses and the matrix are stored, none of the reference's text.  The poses are drawn as tests/_dataset_fixture.write_rhd
draws its labels (uv ~ U(-4, size + 4), depth ~ U(100, 690), size 32) and formed as the loader forms C1 / C2:
(u, v, depth / 700 * 255).  The diagonal is stored as the reference returns it - NaN where rounding puts the cosine of a
pose with itself above 1, which is why the tests compare off the diagonal."""
import ast
import os
import sys

import numpy as np

N, SIZE, SEED = 24, 32, 11


def reference_pose_distance(reference_root):
    path = os.path.join(reference_root, "nearest_neighbor_search", "nearest_neighbor_search.py")
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "poseDistance"]
    assert len(fn) == 1, "poseDistance not found in " + path
    scope = {"np": np}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), scope)
    return scope["poseDistance"]


def draw_poses():
    rs = np.random.RandomState(SEED)
    poses = np.empty((N, 21, 3), dtype=np.float64)
    for i in range(N):
        uv = np.asarray(rs.uniform(-4, SIZE + 4, size=(21, 2)).tolist(), dtype=np.float64)
        depth = np.asarray(rs.uniform(100, 690, size=21).tolist(), dtype=np.float64)
        poses[i] = np.concatenate([uv, np.expand_dims(depth, -1) / 700.0 * 255], axis=-1)
    return poses


def main(argv):
    if len(argv) != 1:
        raise SystemExit(__doc__)
    pose_distance = reference_pose_distance(argv[0])
    poses = draw_poses()
    with np.errstate(invalid="ignore"):
        d = np.array([[pose_distance(poses[i].copy(), poses[j].copy()) for j in range(N)] for i in range(N)], dtype=np.float64)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pose_distance.npz")
    np.savez(out, poses=poses, distance=d)
    off = d[~np.eye(N, dtype=bool)]
    print(out, d.shape, "off-diagonal range", off.min(), off.max())


if __name__ == "__main__":
    main(sys.argv[1:])
