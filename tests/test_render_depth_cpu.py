"""Host side of the depth render (--depth_source joints, aug --novel): the oracle's premises, the C-ABI's declaration, option
validation, the --novel planner and writers, and the resident plan without depth files.  No GPU."""
import argparse
import ctypes
import fnmatch
import json
import os
import pickle
import re

import numpy as np
import pytest

from tests import _render_oracle as R
from tests._dataset_fixture import write_rhd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- premises of the oracle
def test_oracle_hand_computed_5x5():
    """One bone, (1,2), from (1, 2, z = 51) to (3, 2, z = 102), radius 1, bg 255; every other joint is NaN, which switches
    the other 19 bones off.  Row 2: x = 0 is at distance 1 from the end a (t = 0, z = 51),
    x = 1, 2, 3 lie on the bone (t = 0, 0.5, 1 -> z = 51, 76.5, 102), x = 4 is at distance 1 from b (z = 102).  Rows 1 and 3
    are covered for x = 1, 2, 3 (distance exactly 1) and not for x = 0 and 4 (distance sqrt 2).  Rows 0 and 4 are background."""
    xyz = np.full((1, 21, 3), np.nan)
    xyz[0, 1], xyz[0, 2] = (1.0, 2.0, 51.0), (3.0, 2.0, 102.0)
    out, cnt = R.render(xyz, 5, 5, 1.0, 255.0, counts=True)
    f = lambda z: np.float32(((np.float64(z) / 255.0) - 0.5) / 0.5)                     # noqa: E731
    bg = f(255.0)
    assert bg == np.float32(1.0)
    want = np.full((5, 5), bg, np.float32)
    want[2] = [f(51.0), f(51.0), f(76.5), f(102.0), f(102.0)]
    want[1, 1:4] = want[3, 1:4] = [f(51.0), f(76.5), f(102.0)]
    assert np.array_equal(out[0], want)
    assert cnt.sum() == 11 and cnt.max() == 1
    assert f(51.0) == np.float32(-0.6) and f(76.5) == np.float32(-0.4)


def test_oracle_depth_test_and_background_rules():
    """two bones over one pixel: the smaller z wins whatever the order; a bone behind bg still wins over the background"""
    xyz = np.full((1, 21, 3), np.nan)
    xyz[0, 1], xyz[0, 2], xyz[0, 3] = (0.0, 0.0, 200.0), (4.0, 0.0, 200.0), (0.0, 0.0, 100.0)     # bones (1,2) z 200, (2,3) 200 -> 100
    out = R.render(xyz, 1, 5, 0.0, 255.0)
    z = [100.0, 125.0, 150.0, 175.0, 200.0]
    assert np.array_equal(out[0, 0], np.float32([((v / 255.0) - 0.5) / 0.5 for v in z]))
    xyz[0, :, 2] += 300.0                                                                       # everything behind bg
    out = R.render(xyz, 1, 5, 0.0, 255.0)
    assert np.array_equal(out[0, 0], np.float32([(((v + 300.0) / 255.0) - 0.5) / 0.5 for v in z])) and (out > 1).all()


@pytest.mark.parametrize("case", [c for c in R.CASES if R.premises_apply(c)], ids=lambda c: c[0])
def test_oracle_random_cases_cover_enough(case):
    """every random case has between 5 % and 95 % of its pixels covered and at least 1 % under two or more bones (radius 300
    and 1 x 1 exempt).  Measured with this file's seeds: 29x37 r2.5 0.74 / 0.56, 29x37 r1.5 0.60 / 0.28, 16x48 r2.5 0.81 / 0.69,
    8x260 r1.5 0.56 / 0.37, 8x260 r5 0.93 / 0.90, 64x64 r5 0.68 / 0.51, 256x256 r5 0.36 / 0.10."""
    _, _, cnt = R.case_reference(case)
    covered, twice = (cnt >= 1).mean(), (cnt >= 2).mean()
    assert 0.05 <= covered <= 0.95, covered
    assert twice >= 0.01, twice


def test_case_list_holds_what_it_must():
    shapes = {(c[1], c[2]) for c in R.CASES}
    assert shapes == {(1, 1), (29, 37), (16, 48), (8, 260), (64, 64), (256, 256)}
    assert [c for c in R.CASES if (c[1], c[2]) == (256, 256)] == [("256x256-r5", 256, 256, 2, 5.0, "random", 11)]
    assert {c[4] for c in R.CASES} == {0.0, 1.5, 2.5, 5.0, 300.0} and {c[3] for c in R.CASES} == {1, 2, 3}
    h = R.hand_placed()[0]
    assert (h[0] == h[1]).all()                                             # degenerate bone (0,1)
    assert h[1][1] == h[2][1] == 3.0                                         # bone (1,2) on pixel row 3
    assert np.isnan(h[14]).any() and np.isinf(h[18]).any()
    assert (h[9:13, :2] < 0).all()                                          # bones (9,10) (10,11) (11,12) outside
    assert h[19][2] > R.BG and h[20][2] > R.BG
    out, cnt = R.render(R.hand_placed(), 29, 37, 0.0, counts=True)
    assert (cnt[0, 3, 3:16] >= 1).all() and cnt[0, 2, 5:16].sum() == 0 and cnt[0, 4, 5:14].sum() == 0   # radius 0: the row itself
    assert R.render(R.hand_placed(), 29, 37, 1.5, counts=True)[1][0, 5:9, 13:18].max() >= 2      # where (2,3) and (5,6) cross


# ----------------------------------------------------------------------------- the C-ABI
def test_entry_point_is_declared_and_exported():
    from mmhand_amd import lib
    name, n_args = "mmh_render_pose_depth", 10
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmhand_hip.h")).read(), flags=re.S)
    vs = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "mmhand_amd", "csrc", "exports.map")).read(), flags=re.S)
    pats = [p.strip() for p in re.search(r"global\s*:(.*?)local\s*:", vs, flags=re.S).group(1).split(";") if p.strip()]
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, f"include/mmhand_hip.h does not declare {name}"
    assert len(m.group(1).split(",")) == n_args
    assert any(fnmatch.fnmatchcase(name, p) for p in pats), pats
    assert len(lib.SIGNATURES[name][1]) == n_args
    full = open(os.path.join(ROOT, "include", "mmhand_hip.h")).read()
    assert "utils.py:113-124,142-194" in full[full.index("depth condition rendered"):full.index("int mmh_render_pose_depth")]


@pytest.fixture(scope="module")
def built():
    from mmhand_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mmhand_amd", "csrc")])
    return lib.load()


def test_entry_point_refuses_bad_arguments_without_gpu(built):
    buf = (ctypes.c_char * 64)()
    p = ctypes.c_void_p((ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 4)

    def call(xyz0=p, xyz1=p, N=1, H=4, W=4, radius=5.0, bg=255.0, out=p, lanes=8):
        return built.mmh_render_pose_depth(xyz0, xyz1, N, H, W, radius, bg, out, lanes, None)

    for kw in (dict(out=None), dict(xyz0=None, xyz1=None), dict(lanes=3), dict(lanes=4), dict(lanes=4, xyz0=None),
               dict(N=0), dict(H=0), dict(W=-1), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")),
               dict(bg=float("nan")), dict(out=odd), dict(xyz0=odd), dict(N=70000)):
        assert call(**kw) != 0, kw
        assert b"mmh_render_pose_depth" in built.mmh_last_error()


# ----------------------------------------------------------------------------- options
def test_option_validation():
    from mmhand_amd.options import TestOptions, TrainOptions, check_depth_source, default_train_opt
    ns = argparse.Namespace
    assert check_depth_source(ns()) is None
    assert check_depth_source(ns(depth_source="files", render_radius=3.0)) is None
    assert check_depth_source(ns(depth_source="joints", dataroot="/d")) == (5.0, 255.0)
    assert check_depth_source(ns(depth_source="joints", dataroot="/d", render_radius=0, render_bg=100)) == (0.0, 100.0)
    assert check_depth_source(ns(depth_source="joints"), need_dataroot=False) == (5.0, 255.0)
    for bad, match in ((ns(depth_source="render"), "depth_source"), (ns(depth_source="joints"), "dataroot"),
                       (ns(render_radius=-1.0), "render_radius"), (ns(render_radius=float("nan")), "render_radius"),
                       (ns(render_radius="5"), "render_radius"), (ns(render_radius=True), "render_radius"),
                       (ns(render_bg=float("inf")), "render_bg"), (ns(depth_source="joints", dataroot="/d", render_bg=None,
                                                                      render_radius=float("-inf")), "render_radius")):
        with pytest.raises(ValueError, match=match):
            check_depth_source(bad)
    opt = TrainOptions().parse(["--depth_source", "joints", "--dataroot", "/d", "--render_radius", "2.5"], init_dist=False, save=False)
    assert (opt.depth_source, opt.render_radius, opt.render_bg) == ("joints", 2.5, 255.0)
    assert TestOptions().parse(["--depth_source", "joints", "--dataroot", "/d"], init_dist=False, save=False).depth_source == "joints"
    with pytest.raises(ValueError, match="dataroot"):
        TrainOptions().parse(["--depth_source", "joints"], init_dist=False, save=False)
    with pytest.raises(ValueError, match="render_radius"):
        TrainOptions().parse(["--render_radius", "-2"], init_dist=False, save=False)
    with pytest.raises(SystemExit):
        TrainOptions().parse(["--depth_source", "png"], init_dist=False, save=False)
    d = default_train_opt()
    assert (d.depth_source, d.render_radius, d.render_bg) == ("files", 5.0, 255.0)


def test_novel_flag_validation():
    from mmhand_amd import aug, novel
    assert novel.check_novel(1, 1) == (1, 1.0) and novel.check_novel(15, 0.5) == (15, 0.5)
    for k, a in ((0, 0.5), (16, 0.5), (2.0, 0.5), (True, 0.5), (2, 0.0), (2, 1.5), (2, float("nan")), (2, "x")):
        with pytest.raises(ValueError):
            novel.check_novel(k, a)
    # refused before anything touches a device or a checkpoint
    for argv, match in ((["c", "/d", "out", "rhd", "0.5", "0", "--novel", "0"], "novel"),
                        (["c", "/d", "out", "rhd", "0.5", "0", "--novel", "x"], "novel"),
                        (["c", "/d", "out", "rhd", "0.5", "0", "--novel_alpha", "0.5"], "novel_alpha"),
                        (["c", "/d", "out", "rhd", "0.5", "0", "--novel", "2", "--novel_alpha", "0"], "novel_alpha"),
                        (["c", "/d", "out", "rhd", "0.5", "0", "--novel", "2", "--pairing", "nearest"], "pairing"),
                        (["c", "/d", "out", "rhd", "0.5", "0", "--depth_source", "png"], "depth_source"),
                        (["c", "out", "--novel", "2"], "prepared-directory"),
                        (["c", "out", "--depth_source", "joints"], "prepared-directory")):
        with pytest.raises(ValueError, match=match):
            aug.main(argv)
    assert "was not trained on" in aug.__doc__


# ----------------------------------------------------------------------------- --novel: planner and writers
def _brute_knn(poses_q, poses_c, k, exclude_self):
    """the reference's pose distance by brute force in numpy (tests/_pose_oracle states it in full; here it only has to
    produce SOME ranking for the host logic under test)"""
    def feat(p):
        d = (p[:, 1:] - p[:, :-1]).reshape(len(p), -1)
        return d / np.linalg.norm(d, axis=1, keepdims=True)
    cos = np.clip(feat(poses_q) @ feat(poses_c).T, -1, 1)
    dist = np.arccos(cos) / np.pi
    if exclude_self:
        np.fill_diagonal(dist, np.inf)
    idx = np.argsort(dist, axis=1, kind="stable")[:, :k]
    return idx.astype(np.int32), np.take_along_axis(dist, idx, axis=1)


def test_novel_plan_and_writers_round_trip(tmp_path):
    from mmhand_amd import novel
    root = str(tmp_path / "rhd")
    names = sorted(write_rhd(root, n=6, size=32))
    ann = pickle.load(open(os.path.join(root, "annotation.pickle"), "rb"))["color"]
    paths = [os.path.join(root, "color", n) for n in names]
    labels_of = lambda p: ann[os.path.basename(p)]                                      # noqa: E731
    poses = np.stack([np.concatenate([np.asarray(ann[n]["uv_coord"]), np.asarray(ann[n]["depth"])[:, None] / 700 * 255], 1)
                      for n in names])
    K, A = 3, 0.25
    idx, dist = _brute_knn(poses, poses, K, True)
    idx[4, 1:] = -1                                                                     # a target with one neighbour only
    dist[4, 1:] = np.nan
    records, fallbacks = novel.plan(paths, paths, labels_of, idx, dist, K, A)
    assert fallbacks == [4] and len(records) == 6 * K - 2
    assert [r["file"] for r in records] == [f"{i:05d}.png" for i in range(len(records))]
    assert novel.file_name(123456) == "123456.png"
    it = iter(records)
    for i in range(6):
        for r in range(K):
            if idx[i, r] < 0:
                continue
            rec = next(it)
            t, nb = ann[names[i]], ann[names[idx[i, r]]]
            assert (rec["target"], rec["neighbour"], rec["rank"], rec["alpha"]) == (paths[i], paths[idx[i, r]], r + 1, A)
            assert rec["pose_distance"] == dist[i, r]
            assert np.array_equal(rec["uv"], (1.0 - A) * np.float64(t["uv_coord"]) + A * np.float64(nb["uv_coord"]))
            assert np.array_equal(rec["depth"], (1.0 - A) * np.float64(t["depth"]) + A * np.float64(nb["depth"]))
    # alpha 1 is the neighbour's pose itself
    r1, _ = novel.plan(paths, paths, labels_of, idx, dist, 1, 1.0)
    assert np.array_equal(r1[0]["uv"], np.float64(ann[names[idx[0, 0]]]["uv_coord"]))
    with pytest.raises(ValueError):
        novel.plan(paths, paths, labels_of, idx[:, :2], dist[:, :2], 3, A)
    with pytest.raises(ValueError):
        novel.plan(paths, paths[:2], labels_of, idx, dist, K, A)

    dst = str(tmp_path / "out")
    novel.write_annotation(dst, records, (32, 32), (24, 24))
    novel.write_index(dst, records, root=root)
    back = pickle.load(open(os.path.join(dst, "annotation.pickle"), "rb"))
    assert list(back) == ["color"] and list(back["color"]) == [r["file"] for r in records]
    for r in records:
        lab = back["color"][r["file"]]
        assert isinstance(lab["uv_coord"], list) and isinstance(lab["uv_coord"][0][0], float) and len(lab["depth"]) == 21
        assert np.array_equal(np.float64(lab["uv_coord"]), (r["uv"] + 0.5) * 24.0 / 32.0 - 0.5)
        assert np.array_equal(np.float64(lab["depth"]), r["depth"])
    rows = json.load(open(os.path.join(dst, "novel_index.json")))
    assert [set(x) for x in rows] == [{"file", "target", "neighbour", "rank", "alpha", "pose_distance"}] * len(records)
    assert rows[0]["target"] == os.path.join("color", names[0]) and rows[0]["pose_distance"] == records[0]["pose_distance"]
    first = [open(os.path.join(dst, f), "rb").read() for f in ("annotation.pickle", "novel_index.json")]
    novel.write_annotation(dst, records, (32, 32), (24, 24))
    novel.write_index(dst, records, root=root)
    assert first == [open(os.path.join(dst, f), "rb").read() for f in ("annotation.pickle", "novel_index.json")]
    # no resize: the raw blend, and a loader's eye view of the directory: every name sorts by its integer stem
    same = novel.write_annotation(dst, records)
    assert np.array_equal(np.float64(same["color"]["00000.png"]["uv_coord"]), records[0]["uv"])
    assert sorted(same["color"], key=lambda x: int(x[:-4])) == list(same["color"])


# ----------------------------------------------------------------------------- the resident plan
def test_resident_plan_in_joints_mode_names_no_depth_path():
    from mmhand_amd.data import check_table, resident_plan, table_lengths
    src = [f"/r/color/{i}.png" for i in (3, 1, 2, 0, 1)]
    tgt = [f"/r/color/{i}.png" for i in (0, 1, 2, 3, 4)]
    paths, table = resident_plan(src, tgt, list(range(5)), 2, depth_source="joints")
    assert sorted(paths) == sorted(set(src) | set(tgt)) and not any("depth" in p for p in paths)
    assert (table[..., 2:][table[..., 0] >= 0] == table[..., :2][table[..., 0] >= 0]).all()
    assert table_lengths(table) == [2, 2, 1]
    check_table(table, len(paths))
    for g in range(3):
        for r in range(table_lengths(table)[g]):
            assert [paths[s] for s in table[g, r]] == [src[2 * g + r], tgt[2 * g + r]] * 2
    files_paths, files_table = resident_plan(src, tgt, list(range(5)), 2)
    assert len(files_paths) == 2 * len(paths) and sum("depth" in p for p in files_paths) == len(paths)
    assert (files_table == resident_plan(src, tgt, list(range(5)), 2, depth_source="files")[1]).all()
    with pytest.raises(ValueError):
        resident_plan(src, tgt, list(range(5)), 2, depth_source="render")
