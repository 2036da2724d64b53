"""The depth render of mmh_render_pose_depth (include/mmhand_hip.h) stated in numpy float64, operation for operation, and the
cases the CPU and GPU tests share.

Per sample and integer pixel (x, y), the 20 bones in BONES' order; bone a -> b:
    skipped if any of its six coordinates is not finite
    dx = bu-au; dy = bv-av; L2 = dx*dx + dy*dy;  px = x-au; py = y-av
    t = L2 > 0 ? (px*dx + py*dy) / L2 : 0;  t = t < 0 ? 0 : t;  t = t > 1 ? 1 : t
    cx = px - t*dx; cy = py - t*dy;  covered iff cx*cx + cy*cy <= radius*radius;  z = az + t*(bz-az)
D = the z of the first covering bone, replaced by every later covering bone with z < D; bg without one.
Stored: float32(((D / 255.0) - 0.5) / 0.5).  numpy rounds every array operation on its own, which is the kernel's contract.

Covered shares of the random cases (this file's seeds; the premises tests/test_render_depth_cpu.py asserts, 5 % .. 95 % covered
and at least 1 % under two or more bones; radius 300 and 1 x 1 exempt) are listed by `python -m tests._render_oracle`."""
import numpy as np

BONES = ((0, 1), (1, 2), (2, 3), (3, 4), (0, 5), (5, 6), (6, 7), (7, 8), (0, 9), (9, 10), (10, 11), (11, 12),
         (0, 13), (13, 14), (14, 15), (15, 16), (0, 17), (17, 18), (18, 19), (19, 20))
BG = 255.0


def render(xyz, H, W, radius, bg=BG, counts=False):
    """xyz float64 [N,21,3] -> float32 [N,H,W] (with counts=True also int32 [N,H,W]: the bones covering each pixel)"""
    xyz = np.asarray(xyz, dtype=np.float64)
    N = xyz.shape[0]
    assert xyz.shape == (N, 21, 3)
    radius, bg = np.float64(radius), np.float64(bg)
    r2 = radius * radius
    fy, fx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.empty((N, H, W), np.float32)
    cnt = np.zeros((N, H, W), np.int32)
    with np.errstate(all="ignore"):
        for n in range(N):
            D = np.full((H, W), bg, np.float64)
            found = np.zeros((H, W), bool)
            for a, b in BONES:
                (au, av, az), (bu, bv, bz) = xyz[n, a], xyz[n, b]
                if not np.isfinite([au, av, az, bu, bv, bz]).all():
                    continue
                dx, dy = bu - au, bv - av
                L2 = dx * dx + dy * dy
                px, py = fx - au, fy - av
                t = (px * dx + py * dy) / L2 if L2 > 0.0 else np.zeros((H, W), np.float64)
                t = np.where(t < 0.0, 0.0, t)
                t = np.where(t > 1.0, 1.0, t)
                cx, cy = px - t * dx, py - t * dy
                d2 = cx * cx + cy * cy
                z = az + t * (bz - az)
                cov = d2 <= r2
                take = cov & (~found | (z < D))
                D = np.where(take, z, D)
                found |= cov
                cnt[n] += cov
            out[n] = (((D / 255.0) - 0.5) / 0.5).astype(np.float32)
    return (out, cnt) if counts else out


def random_joints(N, H, W, seed):
    """uniform in [-4, W+4] x [-4, H+4], depth uniform in [100, 690] / 700 * 255"""
    g = np.random.default_rng(seed)
    xyz = np.empty((N, 21, 3), np.float64)
    xyz[..., 0] = g.uniform(-4.0, W + 4.0, (N, 21))
    xyz[..., 1] = g.uniform(-4.0, H + 4.0, (N, 21))
    xyz[..., 2] = g.uniform(100.0, 690.0, (N, 21)) / 700.0 * 255
    return xyz


def hand_placed():
    """One pose for grids of at least 29 x 37, [1,21,3]: bone (0,1) degenerate (a == b); bone (1,2) exactly on pixel row 3
    (with radius 0 it covers that row's pixels and nothing else); bones (2,3) and (5,6) cross at different z; bones (9,10)
    (10,11) (11,12) entirely outside the image; joint 14 has a NaN and joint 18 an infinite coordinate (bones (13,14) (14,15)
    (17,18) (18,19) are skipped); bone (0,17) ends behind bg = 255 and bone (19,20) lies entirely behind it."""
    nan, inf = float("nan"), float("inf")
    j = [(3, 3, 100),
         (3, 3, 100), (15, 3, 120), (15, 12, 130), (20, 12, 125),
         (5, 10, 90), (20, 5, 90), (22, 8, 95), (24, 10, 99),
         (-20, -20, 100), (-30, -25, 110), (-40, -10, 120), (-50, -5, 130),
         (8, 15, 110), (nan, 16, 110), (10, 18, 105), (12, 20, 100),
         (6, 20, 300), (inf, 5, 100), (25, 15, 400), (28, 25, 300)]
    return np.asarray(j, dtype=np.float64)[None]


# (id, H, W, N, radius, kind, seed)
CASES = (
    ("1x1-r0", 1, 1, 1, 0.0, "random", 1),
    ("1x1-r1.5", 1, 1, 3, 1.5, "random", 2),
    ("1x1-r300", 1, 1, 1, 300.0, "random", 3),
    ("29x37-r2.5", 29, 37, 3, 2.5, "random", 4),
    ("29x37-r1.5", 29, 37, 1, 1.5, "random", 5),
    ("16x48-r2.5", 16, 48, 3, 2.5, "random", 6),
    ("8x260-r1.5", 8, 260, 1, 1.5, "random", 7),
    ("8x260-r5", 8, 260, 3, 5.0, "random", 8),
    ("64x64-r5", 64, 64, 3, 5.0, "random", 9),
    ("64x64-r300", 64, 64, 1, 300.0, "random", 10),
    ("256x256-r5", 256, 256, 2, 5.0, "random", 11),
    ("29x37-hand-r0", 29, 37, 1, 0.0, "hand", 0),
    ("29x37-hand-r1.5", 29, 37, 1, 1.5, "hand", 0),
    ("64x64-hand-r2.5", 64, 64, 1, 2.5, "hand", 0),
    ("64x64-hand-r5", 64, 64, 1, 5.0, "hand", 0),
    ("64x64-hand-r0", 64, 64, 1, 0.0, "hand", 0),
)
CASE_IDS = [c[0] for c in CASES]


def case_joints(case):
    _, H, W, N, _, kind, seed = case
    return hand_placed() if kind == "hand" else random_joints(N, H, W, seed)


_CACHE = {}


def case_reference(case):
    """(xyz, out float32 [N,H,W], counts) of a case, computed once per process; callers must not write into them"""
    if case[0] not in _CACHE:
        xyz = case_joints(case)
        out, cnt = render(xyz, case[1], case[2], case[4], BG, counts=True)
        for a in (xyz, out, cnt):
            a.setflags(write=False)
        _CACHE[case[0]] = (xyz, out, cnt)
    return _CACHE[case[0]]


def premises_apply(case):
    """the coverage premises hold for the random cases; radius 300 and the 1 x 1 shape are exempt"""
    return case[5] == "random" and case[4] != 300.0 and (case[1], case[2]) != (1, 1)


if __name__ == "__main__":
    for c in CASES:
        _, _, cnt = case_reference(c)
        print(f"{c[0]:18s} covered {(cnt >= 1).mean():.2f}  two or more {(cnt >= 2).mean():.2f}")
