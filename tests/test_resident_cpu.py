"""--resident_dataset without a GPU: the host-side plan (which files one rank's batches touch, and the slot table that
names them), its range check, the budget decision, the flags, and the two entry points' declarations and argument checks."""
import ctypes
import fnmatch
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mmh_store_images": 9, "mmh_decode_inputs_indexed": 16}


def _files(n):
    return [f"/d/color/{i:03d}.png" for i in range(n)]


def _pairs(table, lengths, paths):
    """the (img1, img2, dep1, dep2) file names the table's used rows name, batch by batch"""
    return [[tuple(paths[s] for s in row) for row in t[:n]] for t, n in zip(table, lengths)]


def test_plan_deduplicates_files_and_keeps_depth_twins():
    from mmhand_amd.data import check_table, resident_plan, table_lengths
    tgt = _files(5)
    src = [tgt[i] for i in (2, 0, 4, 1, 3)]                # every file is source in one pair and target in another
    paths, table = resident_plan(src, tgt, list(range(5)), 2, float("inf"))
    assert len(paths) == len(set(paths)) == 10              # 5 colour files + 5 depth twins, each once
    assert set(paths) == set(tgt) | {p.replace("color", "depth") for p in tgt}
    assert table.dtype == np.int32 and table.shape == (3, 2, 4)
    lengths = table_lengths(table)
    assert lengths == [2, 2, 1]                             # the short last batch keeps its own length ...
    assert (table[2, 1] == -1).all() and (table[:2] >= 0).all() and (table[2, 0] >= 0).all()      # ... its unused row is no slot
    want = [(src[i], tgt[i], src[i].replace("color", "depth"), tgt[i].replace("color", "depth")) for i in range(5)]
    got = _pairs(table, lengths, paths)
    assert [p for b in got for p in b] == want
    # one slot per file wherever it appears: file 2 is img1 of pair 0 and img2 of pair 2
    assert table[0, 0, 0] == table[1, 0, 1] and table[0, 0, 2] == table[1, 0, 3]
    assert check_table(table, len(paths)) is table


def test_plan_truncates_to_max_batches():
    from mmhand_amd.data import resident_plan, table_lengths
    tgt = _files(9)
    src = tgt[::-1]
    paths, table = resident_plan(src, tgt, list(range(9)), 2, 2)
    assert table.shape == (2, 2, 4) and table_lengths(table) == [2, 2]
    used = {f for i in range(4) for f in (src[i], tgt[i])}
    assert set(paths) == used | {p.replace("color", "depth") for p in used}        # nothing of the batches that are cut
    paths_all, table_all = resident_plan(src, tgt, list(range(9)), 2)
    assert table_all.shape == (5, 2, 4) and table_lengths(table_all)[-1] == 1 and len(paths_all) == 18
    assert resident_plan(src, tgt, [], 2, 5)[0] == [] and resident_plan(src, tgt, [], 2, 5)[1].shape == (0, 2, 4)


def test_plan_of_a_world_of_two_covers_each_ranks_own_pairs():
    """the two ranks' index lists as DistributedSampler deals them (padded to a multiple of the world: pair 0 twice): each
    rank's store holds exactly the files of its own pairs; the stores may overlap (a file that is source for one rank and
    target for the other), neither holds the whole dataset"""
    from mmhand_amd.data import check_table, resident_plan, table_lengths
    tgt = _files(7)
    src = [tgt[i] for i in (1, 2, 3, 4, 5, 6, 0)]
    order = [3, 0, 6, 2, 5, 1, 4, 3]
    ranks = [order[0::2], order[1::2]]
    stores = []
    for idx in ranks:
        paths, table = resident_plan(src, tgt, idx, 3, float("inf"))
        check_table(table, len(paths))
        lengths = table_lengths(table)
        assert lengths == [3, 1]
        own = {f for i in idx for f in (src[i], tgt[i])}
        assert set(paths) == own | {p.replace("color", "depth") for p in own}
        got = [p for b in _pairs(table, lengths, paths) for p in b]
        assert [(a, b) for a, b, _, _ in got] == [(src[i], tgt[i]) for i in idx]
        stores.append(set(paths))
    assert stores[0] & stores[1] and stores[0] != stores[1]
    assert all(len(s) < 14 for s in stores)


def test_table_range_check():
    from mmhand_amd.data import check_table, resident_plan
    tgt = _files(4)
    paths, table = resident_plan(tgt[::-1], tgt, list(range(4)), 3)
    check_table(table, len(paths))
    with pytest.raises(ValueError, match="outside"):
        check_table(table, len(paths) - 1)                  # a slot == S
    bad = table.copy()
    bad[0, 1, 2] = -3
    with pytest.raises(ValueError, match="outside"):
        check_table(bad, len(paths))
    bad = table.copy()
    bad[1, 2, 1] = 0                                         # a row after the unused ones
    with pytest.raises(ValueError, match="unused"):
        check_table(bad, len(paths))
    with pytest.raises(ValueError, match="int32"):
        check_table(table.astype(np.int64), len(paths))


def test_budget_decision():
    from mmhand_amd.data import resident_decision
    need, state = resident_decision(10, 32, 32, 1)
    assert need == 10 * 32 * 32 * 3 and state.startswith("off: ") and "budget" in state
    assert resident_decision(10, 32, 32, need) == (need, "on")
    assert resident_decision(10, 32, 32, need, free_bytes=need) == (need, "on")
    assert resident_decision(10, 32, 32, need, free_bytes=need - 1)[1].startswith("off: ")
    assert resident_decision(0, 32, 32, need)[1].startswith("off: ")
    # 40 k colour + depth images of 256 x 256: 15.7 GB, inside the default budget
    assert resident_decision(80000, 256, 256, int(64e9)) == (80000 * 196608, "on")


def test_png_size_reads_the_ihdr(tmp_path):
    from PIL import Image
    from mmhand_amd.data import png_size
    p = os.path.join(tmp_path, "a.png")
    Image.fromarray(np.zeros((12, 20, 3), np.uint8)).save(p)
    assert png_size(p) == (12, 20)
    with open(p, "wb") as fh:
        fh.write(b"not a png at all, but long enough")
    assert png_size(p) is None


def test_flags_parse():
    from mmhand_amd.options import TestOptions, TrainOptions, default_train_opt
    opt = TrainOptions().parse([], init_dist=False, save=False)
    assert opt.resident_dataset is False and opt.resident_gb == 64.0                          # off by default
    opt = TrainOptions().parse(["--resident_dataset", "--resident_gb", "1.5"], init_dist=False, save=False)
    assert opt.resident_dataset is True and opt.resident_gb == 1.5
    assert TestOptions().parse(["--resident_dataset"], init_dist=False, save=False).resident_dataset is True
    assert default_train_opt(resident_dataset=True).resident_dataset is True
    from mmhand_amd import options
    assert "policy" in dict(options._BASE)["--resident_gb"]["help"]        # the default is a choice, not a measurement


def test_entry_points_are_declared_and_exported():
    from mmhand_amd import lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmhand_hip.h")).read(), flags=re.S)
    vs = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "mmhand_amd", "csrc", "exports.map")).read(), flags=re.S)
    pats = [p.strip() for p in re.search(r"global\s*:(.*?)local\s*:", vs, flags=re.S).group(1).split(";") if p.strip()]
    for name, n_args in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"include/mmhand_hip.h does not declare {name}"
        assert len(m.group(1).split(",")) == n_args
        assert any(fnmatch.fnmatchcase(name, p) for p in pats), pats
        assert len(lib.SIGNATURES[name][1]) == n_args


@pytest.fixture(scope="module")
def built():
    from mmhand_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mmhand_amd", "csrc")])
    return lib.load()


def test_symbols_are_in_the_librarys_table(built):
    import subprocess
    from mmhand_amd import lib
    syms = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    table = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    for name in NAMES:
        assert name in table and getattr(built, name) is not None


def test_entry_points_refuse_bad_arguments_without_gpu(built):
    """MMH_REQUIRE runs before any launch: NULL buffers, non-positive shapes, S = 0 and misaligned outputs come back as
    errors, each with its own message, on a machine without a device"""
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    lb = built
    for args in ((None, p, 1, 2, 2, p, 1, None, None), (p, None, 1, 2, 2, p, 1, None, None), (p, p, 1, 2, 2, None, 1, None, None)):
        assert lb.mmh_store_images(*args) != 0
        assert b"mmh_store_images: NULL buffer" in lb.mmh_last_error()
    for shape in ((0, 2, 2), (1, 0, 2), (1, 2, -2)):
        assert lb.mmh_store_images(p, p, *shape, p, 1, None, None) != 0
        assert b"mmh_store_images: bad shape" in lb.mmh_last_error()
    for S in (0, -1):
        assert lb.mmh_store_images(p, p, 1, 2, 2, p, S, None, None) != 0
        assert b"mmh_store_images: S must be at least 1" in lb.mmh_last_error()

    def dec(store=p, S=1, Hs=2, Ws=2, idx=p, uv=p, B=1, Ho=4, Wo=4, sigma=6.0, outs=(p, p, p, p)):
        return lb.mmh_decode_inputs_indexed(store, S, Hs, Ws, idx, uv, B, Ho, Wo, sigma, *outs, None, None)

    for kw in (dict(store=None), dict(idx=None), dict(uv=None), dict(outs=(None, p, p, p)), dict(outs=(p, p, p, None))):
        assert dec(**kw) != 0
        assert b"mmh_decode_inputs_indexed: NULL buffer" in lb.mmh_last_error()
    for kw in (dict(B=0), dict(Hs=0), dict(Ws=-1), dict(Ho=0), dict(Wo=-4), dict(sigma=0.0)):
        assert dec(**kw) != 0
        assert b"mmh_decode_inputs_indexed: bad shape" in lb.mmh_last_error()
    assert dec(S=0) != 0
    assert b"mmh_decode_inputs_indexed: S must be at least 1" in lb.mmh_last_error()
    assert dec(outs=(p, p, odd, p)) != 0
    assert b"mmh_decode_inputs_indexed: outputs must be 16-byte aligned" in lb.mmh_last_error()
