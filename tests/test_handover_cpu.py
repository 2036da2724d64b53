"""The hand-over tables of mmhand_amd/ops.py (mmhand_amd/handover.py) on plain CPU tensors: one rule for every table - an entry
is returned only to a tensor with the shape, strides and version of the one it was left under, while its anchor lives - and
each table's bound, eviction and reset."""
import pytest
import torch

from mmhand_amd import ops
from mmhand_amd.handover import Handover

TABLES = ("_pending_stats", "_stem_masks", "_nbr_sites", "_pack_twins", "_lp_grads", "_nb_defer")
WEAK = ("_pending_stats", "_stem_masks", "_nbr_sites")
SHAPE = (2, 4, 4, 8)


@pytest.fixture(autouse=True)
def _empty_tables():
    for n in TABLES:
        getattr(ops, n).clear()
    yield
    for n in TABLES:
        getattr(ops, n).clear()


@pytest.fixture(params=TABLES)
def table(request):
    t = getattr(ops, request.param)
    assert isinstance(t, Handover) and t.held == (request.param not in WEAK)
    return t


def test_handed_over_once_kept_every_time_and_dropped(table):
    x, v = torch.zeros(SHAPE), object()
    assert table.get(x) is None and x.data_ptr() not in table
    table.put(x, v)
    assert x.data_ptr() in table and len(table) == 1 and table
    assert table.get(x, pop=False) is v and table.get(x) is v and table.get(x) is None and not table
    table.put(x, v, keep=True)
    assert table.get(x) is v and table.get(x) is v
    table.drop(x)
    assert table.get(x) is None and not table
    table.drop(x)                       # nothing there: no error


def test_in_place_write_invalidates(table):
    x = torch.zeros(SHAPE)
    table.put(x, 1, keep=True)
    x.add_(1)
    assert len(table) == 1 and table.get(x) is None and not table


def test_same_address_other_shape_or_strides_misses(table):
    x = torch.zeros(SHAPE)
    table.put(x, 1)
    assert table.get(x[:1]) is None and not table
    table.put(x, 1)
    assert table.get(x.as_strided(SHAPE, (128, 8, 32, 1))) is None and not table


def test_dead_anchor_at_the_same_address_shape_strides_and_version(table):
    """the allocator hands a dead tensor's address to a new one: only the anchor tells them apart.  A weak table misses; a
    table that holds an alias kept the storage, so the new tensor is over the very same, unchanged bytes"""
    y = torch.zeros(SHAPE)
    y.add_(0)
    st, ptr = y.untyped_storage(), y.data_ptr()
    table.put(y, 1)
    del y
    z = torch.empty(0).set_(st, 0, SHAPE)
    assert z.data_ptr() == ptr and z._version == 1 and ptr in table
    assert table.get(z) == (None if not table.held else 1) and not table


@pytest.mark.parametrize("name", ["_pending_stats", "_nbr_sites", "_pack_twins"])
def test_bound_drops_the_oldest(name):
    """40 live keys never leave more than the bound, and the newest `bound` entries are all still there"""
    table = getattr(ops, name)
    live = [torch.zeros(SHAPE) for _ in range(40)]
    for i, t in enumerate(live):
        table.put(t, i)
        assert len(table) <= table.bound
    assert [table.get(t) for t in live] == [None] * (40 - table.bound) + list(range(40 - table.bound, 40))


def test_ninth_statistics_entry_does_not_empty_the_table():
    """(it used to: the entries owed to the other generator streams' norms went with it, and those norms ran a full pass)"""
    live = [torch.zeros(SHAPE) for _ in range(9)]
    for i, y in enumerate(live):
        ops._park_stats(y, i)
    assert [ops._take_stats(y) for y in live] == [None] + [(i,) for i in range(1, 9)]


@pytest.mark.parametrize("name", WEAK)
def test_dead_entries_go_first_at_the_bound(name):
    table = getattr(ops, name)
    storages, live = [], [torch.zeros(SHAPE) for _ in range(4)]
    for i, t in enumerate(live):
        table.put(t, i)
    for _ in range(40):
        d = torch.zeros(SHAPE)
        storages.append(d.untyped_storage())            # the address is not handed out again
        table.put(d, -1)
        del d
        assert len(table) <= table.bound
    assert [table.get(t) for t in live] == [0, 1, 2, 3]


def test_bounds_are_8_8_8_16_and_masks_alone_keep_live_entries():
    assert [getattr(ops, n).bound for n in TABLES] == [8, 8, 8, 16, None, None]
    assert [getattr(ops, n).evict_live for n in TABLES] == [True, False, True, True, True, True]


def test_live_masks_survive_the_bound():
    """8 live and 4 dead anchors, then more requests: the dead go, every live mask stays (its stem's wgrad is still owed it)"""
    t = ops._stem_masks
    doomed = [torch.zeros(SHAPE) for _ in range(4)]
    live = [torch.zeros(SHAPE) for _ in range(11)]
    for i, x in enumerate(doomed + live[:8]):
        t.put(x, i - 4)
    assert len(t) == 12
    keep_storage = [d.untyped_storage() for d in doomed]       # their addresses are not handed out again
    del doomed, x
    for i, x in enumerate(live[8:], 8):
        t.put(x, i)
    assert len(t) == 11 and [t.get(x, pop=False) for x in live] == list(range(11))
    live[0].add_(1)                                     # a rewritten tensor's mask is as good as dead
    one_more = torch.zeros(SHAPE)
    t.put(one_more, 11)
    assert live[0].data_ptr() not in t and len(t) == 11 and t.get(live[1], pop=False) == 1


def test_mask_table_asks_for_the_capture_side_of_device_tensors_only(monkeypatch):
    def boom():
        raise RuntimeError("no device")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", boom)
    x = torch.zeros(SHAPE)
    ops._stem_masks.put(x, 1, keep=True)
    assert ops._stem_mask_for(x) == 1 and ops._stem_mask_for(x) == 1       # a mask is not consumed
    ops.stem_mask_forget(x[:1])                                              # a leading slice: the address decides
    assert ops._stem_mask_for(x) is None


def test_accessors_of_the_statistics_table():
    y, stats = torch.zeros(SHAPE), torch.ones(3)
    ops._park_stats(y, stats)
    assert ops._take_stats(y, peek=True)[0] is stats and ops._take_stats(y)[0] is stats and ops._take_stats(y) is None


def test_reset_empties_the_per_iteration_tables_and_keeps_kept_twins_and_masks():
    xs = [torch.zeros(SHAPE) for _ in range(7)]
    twin = torch.zeros(SHAPE, dtype=torch.bfloat16)
    ops._lp_grads.put(xs[0], 1)
    ops._nb_defer.put(xs[1], 1)
    ops.nbr_site_put(xs[2], 1)
    ops._park_stats(xs[3], 1)
    ops.pack_twin_put(xs[4], twin)
    ops.pack_twin_put(xs[5], twin, keep=True)
    ops._stem_masks.put(xs[6], 1, keep=True)
    ops.handover_reset()
    assert not ops._lp_grads and not ops._nb_defer and not ops._nbr_sites and not ops._pending_stats
    assert ops.pack_twin_get(xs[4], True) is None and ops.pack_twin_get(xs[5], True) is twin and len(ops._pack_twins) == 1
    assert ops._stem_mask_for(xs[6]) == 1
    ops._park_stats(xs[3], 1)
    ops.bump_weights_epoch()            # an optimizer step empties the pending statistics too, and nothing else here
    assert not ops._pending_stats and len(ops._pack_twins) == 1 and len(ops._stem_masks) == 1


def test_foreign_proxies_fail_loudly():
    g = ops.lp_proxy(SHAPE, "cpu")
    with pytest.raises(RuntimeError, match="did not arrive through the 16-bit channel"):
        ops.lp_grad_in(g, "test")
    with pytest.raises(RuntimeError, match="test: expected the deferred gradient of a fused norm \\(NormBwdDefer\\) on this edge"):
        ops.norm_bwd_defer_in(g, "test")
    for take in (ops.lp_grad_in, ops.norm_bwd_defer_in):
        with pytest.raises(RuntimeError):
            take(None, "test")
    t16 = torch.zeros(SHAPE, dtype=torch.bfloat16)
    p = ops.lp_grad_out(t16)
    assert p.shape == t16.shape and p.stride() == (0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="NormBwdDefer"):
        ops.norm_bwd_defer_in(p, "test")            # the other table's proxy
    assert ops.lp_grad_in(p, "test") is t16
    with pytest.raises(RuntimeError, match="16-bit channel"):
        ops.lp_grad_in(p, "test")                   # handed over once
