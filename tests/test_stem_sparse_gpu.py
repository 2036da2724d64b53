"""The compacted-channel fp32 7x7 stem kernels (stem_sparse.hip) against the dense kernels they stand in for: the activity
mask against a torch expression, the fprop bit for bit against mmh_conv2d_fprop_stats, the wgrad exactly on integer operands
and within 1.5x of the dense kernel's own error on floats, and the routing of a whole training step.

Shapes: B = 2, 64 x 64 (the smallest width the stem wgrad family accepts): a 4 x 8 grid of 8 x 16 blocks - interior, edge and
corner tiles - with 44 -> 64 (the Generator's pose stem) and 24 -> 64 (D_PB)."""
import ctypes
import random
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

from oracle import mmhand_ref as O
from oracle import ops_ref as R
from tests.golden import recipe as RC

pytestmark = pytest.mark.gpu
B, H, W = 2, 64, 64
CS = (44, 24)


def _pose_input(C, dev, seed):
    """pose lanes from ops.pose_heatmaps with hand-placed joints; C = 24: lanes 21-23 dense noise; C = 44: lanes 42, 43 zero"""
    from mmhand_amd import ops
    P = 42 if C == 44 else 21
    uv = torch.full((B, P, 2), -30.0, dtype=torch.float64)            # (-30, -30): an all-zero channel
    uv[0, 0] = torch.tensor([32.0, 32.0])                             # the centre
    uv[0, 1] = torch.tensor([1.5, 1.5])                               # crosses two borders, its mirror image enters the halo
    uv[0, 3] = torch.tensor([20.0, 40.0])                             # two joints 4 px apart: two active channels per tile
    uv[0, 4] = torch.tensor([24.0, 40.0])
    uv[0, P - 1] = torch.tensor([62.0, 5.0])                          # the last pose lane, at the right border
    for i in range(12):                                               # image 1: 12 joints inside one tile, a long list
        uv[1, 5 + i] = torch.tensor([33.0 + (i % 4) * 4, 17.0 + (i // 4) * 5])
    maps = ops.pose_heatmaps(uv.reshape(B * P, 2).contiguous().to(dev), H, W).reshape(B, P, H, W)
    x = torch.zeros((B, H, W, C), device=dev)
    x[..., :P] = maps.permute(0, 2, 3, 1)
    if C == 24:
        g = torch.Generator(device="cpu").manual_seed(seed)
        x[..., 21:24] = torch.randn((B, H, W, 3), generator=g).to(dev)
    return x.contiguous()


def _dense_input(C, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((B, H, W, C), generator=g).to(dev).contiguous()


def _inputs(C, dev):
    return {"pose": _pose_input(C, dev, 11), "dense": _dense_input(C, dev, 12)}


def _mask_ref(x):
    """reflect-pad by 3, != 0, max-pool over each block's 14 x 22 window -> int64 [B, H/8, W/16]"""
    nz = (F.pad(x.permute(0, 3, 1, 2), (3, 3, 3, 3), mode="reflect") != 0).float()
    on = F.max_pool2d(nz, kernel_size=(14, 22), stride=(8, 16)).to(torch.int64)        # [B, C, H/8, W/16]
    bits = torch.zeros(on[:, 0].shape, dtype=torch.int64, device=x.device)
    for c in range(x.shape[3]):
        bits |= on[:, c] << c
    return bits


def _mask(x):
    from mmhand_amd import lib as L, ops
    nb = L.load().mmh_stem_activity_bytes(*x.shape[:3])
    assert nb == x.shape[0] * (x.shape[1] // 8) * (x.shape[2] // 16) * 8
    m = torch.full((nb // 8,), -1, dtype=torch.int64, device=x.device)
    L.call("mmh_stem_activity", ops._ptr(x), *x.shape, ops._ptr(m), ops._stream())
    return m


@pytest.mark.parametrize("C", CS)
def test_activity_mask_is_exact(C, dev):
    for name, x in _inputs(C, dev).items():
        if name == "pose":
            x = x.clone()
            x[0, 40:48, 0:16, 2] = -0.0         # -0.0 counts as zero: lane 2 stays all-zero
            x[1, 8:10, 20:22, 0] = -0.0
            x[1, 63, 63, 20] = float("nan")     # NaN counts as non-zero; the corner pixel reaches no other block's halo
            x[1, 3, 3, 19] = 1e-30              # inside the reflected ring of the corner block
        m = _mask(x).view(B, H // 8, W // 16)
        assert torch.equal(m, _mask_ref(x)), name
        if name == "pose":
            assert not bool(((m >> 2) & 1).any()) and bool(((m >> 19) & 1).sum() == 1) and bool(((m[1] >> 20) & 1).sum() == 1)
            pop = sum(((m >> c) & 1) for c in range(C))
            assert int(pop.max()) >= 12 and int(pop.min()) <= 3       # the long list and nearly empty tiles are both there
        else:
            assert bool((m == (1 << C) - 1).all())


def _fprop(x, w, bias, mask):
    from mmhand_amd import lib as L, ops
    C = x.shape[3]
    d = ops.conv_desc(B, H, W, C, 64, 7, 1, 3, True)
    chunks = L.load().mmh_conv2d_fprop_stats_chunks(ctypes.byref(d))
    assert chunks > 0
    y = torch.full((B, H, W, 64), 7.0, device=x.device)
    st = torch.full((chunks, 3, 64), 7.0, device=x.device)
    if mask is None:
        L.call("mmh_conv2d_fprop_stats", ctypes.byref(d), ops._ptr(x), ops._ptr(w), ops._ptr(bias), ops._ptr(y), ops._ptr(st),
               ops._stream())
    else:
        assert L.load().mmh_conv7_stem_sparse_fprop_supported(ctypes.byref(d)) == 1
        L.call("mmh_conv7_stem_sparse_fprop", ctypes.byref(d), ops._ptr(x), ops._ptr(mask), ops._ptr(w), ops._ptr(bias),
               ops._ptr(y), ops._ptr(st), ops._stream())
    return y, st


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("C", CS)
def test_sparse_fprop_is_the_dense_fprop_bit_for_bit(C, with_bias, dev):
    g = torch.Generator(device="cpu").manual_seed(5 + C)
    w = (torch.randn((7, 7, C, 64), generator=g) * 0.05).to(dev)
    bias = (torch.randn((64,), generator=g) * 0.1).to(dev) if with_bias else None
    for name, x in _inputs(C, dev).items():
        y0, s0 = _fprop(x, w, bias, None)
        mask = _mask(x)
        y1, s1 = _fprop(x, w, bias, mask)
        assert torch.equal(y1, y0), (name, float((y1 - y0).abs().max()))
        assert torch.equal(s1, s0), name
        y2, s2 = _fprop(x, w, bias, mask)
        assert torch.equal(y2, y1) and torch.equal(s2, s1), name


def _wgrad(x, dy, sparse, out=None):
    """dense: ops.raw_conv_wgrad without a mask (mmh_conv7_stem_wgrad at 44 lanes, mmh_conv2d_wgrad at 24); sparse: the entry
    point itself (ops routes to it only where the dense route is mmh_conv7_stem_wgrad: the test below)"""
    from mmhand_amd import lib as L, ops
    ops._stem_masks.clear()
    if not sparse:
        return ops.raw_conv_wgrad(x, dy, 7, 1, 3, True, out=out)
    C = x.shape[3]
    d = ops.conv_desc(B, H, W, C, 64, 7, 1, 3, True)
    assert L.load().mmh_conv7_stem_sparse_wgrad_supported(ctypes.byref(d)) == 1
    mask = _mask(x)
    nb = L.load().mmh_conv7_stem_sparse_wgrad_ws_bytes(ctypes.byref(d))
    ws = torch.full((nb // 4,), float("nan"), device=x.device)
    dw = out if out is not None else torch.full((7, 7, C, 64), float("nan"), device=x.device)
    L.call("mmh_conv7_stem_sparse_wgrad", ctypes.byref(d), ops._ptr(x), ops._ptr(mask), ops._ptr(dy), ops._ptr(dw), ops._ptr(ws), nb,
           int(out is not None), ops._stream())
    return dw


def test_sparse_wgrad_is_the_dense_stem_wgrad_bit_for_bit(dev):
    """44 lanes, where the dense route is mmh_conv7_stem_wgrad: the sparse kernel keeps its tiles, splits, pixel order and slab
    sum and leaves out all-zero terms, so dw is equal on floats - with accumulate 0 and 1, on sparse and on dense inputs -
    and ops.raw_conv_wgrad takes it exactly when a mask was requested"""
    from mmhand_amd import lib as L, ops
    g = torch.Generator(device="cpu").manual_seed(77)
    dy = torch.randn((B, H, W, 64), generator=g).to(dev)
    base = torch.randn((7, 7, 44, 64), generator=g).to(dev)
    for name, x in _inputs(44, dev).items():
        assert torch.equal(_wgrad(x, dy, True), _wgrad(x, dy, False)), name
        assert torch.equal(_wgrad(x, dy, True, out=base.clone()), _wgrad(x, dy, False, out=base.clone())), name
    for C, want in ((44, True), (24, False)):
        x = _inputs(C, dev)["pose"]
        ops._stem_masks.clear()
        assert ops.stem_mask_request(x) is not None
        calls, orig = [], L.call

        def spy(name, *a):
            calls.append(name)
            return orig(name, *a)
        L.call = spy
        try:
            routed = ops.raw_conv_wgrad(x, dy, 7, 1, 3, True)
        finally:
            L.call = orig
            ops._stem_masks.clear()
        assert ("mmh_conv7_stem_sparse_wgrad" in calls) == want, (C, calls)
        assert torch.equal(routed, _wgrad(x, dy, False)), C


def test_cached_mask_serves_only_the_tensor_and_contents_it_was_made_from(dev, monkeypatch):
    """ops.stem_mask_request computes once per tensor; an in-place write, stem_mask_forget, a new tensor at a dead one's
    address (same shape, strides and version) and the other side of a graph capture each make a new mask pass"""
    from mmhand_amd import lib as L, ops
    calls, real = [], L.call
    monkeypatch.setattr(L, "call", lambda n, *a: (calls.append(n), real(n, *a))[1])
    ops._stem_masks.clear()
    x = _pose_input(24, dev, 11)
    masks = [ops.stem_mask_request(x)]

    def again(t, launches):
        masks.append(ops.stem_mask_request(t))
        assert calls.count("mmh_stem_activity") == launches
        assert masks[-1] is not None and torch.equal(masks[-1], masks[0])
        return masks[-1]
    assert masks[0] is not None and calls.count("mmh_stem_activity") == 1
    assert again(x, 1) is masks[0]
    x.mul_(1)
    assert again(x, 2) is not masks[0]
    ops.stem_mask_forget(x)
    assert again(x, 3) is not masks[-2]
    st, ptr, shape, stride, version = x.untyped_storage(), x.data_ptr(), x.shape, x.stride(), x._version
    del x
    z = torch.empty(0, device=dev).set_(st, 0, shape).data          # .data: a version counter of its own, at 0
    while z._version < version:
        z.mul_(1)
    assert (z.data_ptr(), z.shape, z.stride(), z._version) == (ptr, shape, stride, version) and ptr in ops._stem_masks
    assert again(z, 4) is not masks[-2]
    assert again(z, 4) is masks[-2]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert again(z, 5) is not masks[-2]         # made eagerly: not for a capture
    monkeypatch.undo()
    ops._stem_masks.clear()


def _dw_oracle(x, dy):
    C = x.shape[3]
    return R.conv2d_grads(x.cpu(), torch.zeros((7, 7, C, 64)), None, dy.cpu(), 1, 3, True)[2]


@pytest.mark.parametrize("C", CS)
def test_sparse_wgrad_is_exact_on_integer_operands(C, dev):
    """pose lanes in {0, 1, 2} on the heat maps' supports, dense lanes in {0, 1, 2}, dy in {-2 .. 2}: every partial sum is an
    integer below 2^24, so the fp64 oracle, the dense kernel and the sparse kernel agree exactly"""
    g = torch.Generator(device="cpu").manual_seed(21 + C)
    dy = torch.randint(-2, 3, (B, H, W, 64), generator=g).float().to(dev)
    for name, xf in _inputs(C, dev).items():
        x = torch.ceil(xf.clamp(0, 1) * 2).contiguous() if name == "pose" else torch.randint(0, 3, xf.shape, generator=g).float().to(dev)
        if name == "pose" and C == 24:
            x[..., 21:24] = torch.randint(0, 3, (B, H, W, 3), generator=g).float().to(dev)
        ref = _dw_oracle(x, dy).float()
        assert float(ref.abs().max()) < 2 ** 24
        dense, sparse = _wgrad(x, dy, False), _wgrad(x, dy, True)
        assert torch.equal(dense.cpu(), ref), name
        assert torch.equal(sparse.cpu(), ref), (name, float((sparse.cpu() - ref).abs().max()))
        base = torch.randint(-3, 4, ref.shape, generator=g).float()
        for fn in (False, True):
            acc = _wgrad(x, dy, fn, out=base.clone().to(dev))
            assert torch.equal(acc.cpu(), ref + base), (name, fn)


@pytest.mark.parametrize("C", CS)
def test_sparse_wgrad_error_on_floats_is_the_dense_kernels(C, dev):
    """relative L1 against the fp64 oracle: the sparse kernel sums the same products in another order, so at most 1.5x the
    dense kernel's figure (the margin the 16-bit bars use over their yardstick); run twice: reproducible"""
    g = torch.Generator(device="cpu").manual_seed(31 + C)
    dy = torch.randn((B, H, W, 64), generator=g).to(dev)
    for name, x in _inputs(C, dev).items():
        ref = _dw_oracle(x, dy)
        dense, sparse = _wgrad(x, dy, False), _wgrad(x, dy, True)
        e_d, e_s = R.rel_l1(dense.cpu().double(), ref), R.rel_l1(sparse.cpu().double(), ref)
        print(f"wgrad C={C} {name}: rel L1 dense {e_d:.3e} sparse {e_s:.3e}")
        assert e_s <= 1.5 * e_d, (name, e_s, e_d)
        assert torch.equal(_wgrad(x, dy, True), sparse), name       # reproducible


def test_training_step_routes_the_two_pose_stems_and_nothing_else(dev):
    """one optimize_parameters with "stem_sparse" 1 and one with 0 (two-block Generator and D_PB at 64 x 64, B = 2; full width,
    since the stem kernels - dense and sparse - are built for 64 output channels): the same fake_p2 and forward losses bit for
    bit, the parameters after the step equal too, and the sparse entry points run for the 44-lane pose stem and the 24-lane
    D_PB stem only (the wgrad for the pose stem alone)"""
    from mmhand_amd import lib as L, ops
    from mmhand_amd.mmhand_model import MMHandModel
    from mmhand_amd.options import default_train_opt
    res = {}
    old = L.get_option("stem_sparse")
    orig = L.call
    try:
        for on in (1, 0):
            L.call = orig
            L.call("mmh_set_option", b"stem_sparse", on)
            opt = default_train_opt(batchSize=B, ngf=64, ndf=64, n_layers_D=2, G_n_blocks=2, norm="instance", pool_size=0,
                                    no_dropout=True, no_dropout_D=True, name="sparse", checkpoints_dir="/tmp/mmh_pytest_ckpt",
                                    local_rank=0)
            model = MMHandModel(opt)
            for tag, net in (("G", model.netG), ("DPB", model.netD_PB), ("DPP", model.netD_PP)):
                shapes = OrderedDict((f"{tag}/{k}", tuple(v.shape)) for k, v in net.state_dict().items())
                sd = RC.recipe_state_dict(shapes)
                net.load_state_dict(OrderedDict((k.split("/", 1)[1], v) for k, v in sd.items()))
            model.vgg.load_state_dict(RC.vgg_recipe())
            random.seed(49)
            ops.set_dropout_seed(1234)
            seen = []

            def spy(name, *a):
                if name in ("mmh_conv7_stem_sparse_fprop", "mmh_conv7_stem_sparse_wgrad"):
                    seen.append((name, a[0]._obj.Cin))
                elif name == "mmh_stem_activity":
                    seen.append((name, a[4]))
                return orig(name, *a)
            L.call = spy
            model.set_input(O.synthetic_batch(B, H, W, seed=100))
            model.optimize_parameters()
            L.call = orig
            losses = [float(v) for v in model.get_current_errors().values()]
            params = [p.detach().clone() for n in (model.netG, model.netD_PB, model.netD_PP) for p in n.parameters()]
            res[on] = (model.fake_p2.detach().clone(), losses, params, seen)
    finally:
        L.call = orig
        L.call("mmh_set_option", b"stem_sparse", old)
    assert torch.equal(res[1][0], res[0][0])
    assert res[1][1] == res[0][1], (res[1][1], res[0][1])
    # the sparse kernels give the dense kernels' bits in both passes, so the step is the same step (the fixture's tolerance of
    # tests/test_model_gpu.py, atol 6e-4 + 1e-3 max|ref|, holds with nothing to spare needed)
    for a, b in zip(res[1][2], res[0][2]):
        assert torch.equal(a, b)
    assert res[0][3] == []
    seen = res[1][3]
    for name in ("mmh_conv7_stem_sparse_fprop", "mmh_stem_activity"):
        assert {c for n, c in seen if n == name} == {24, 44}, (name, seen)
    # the wgrad: only where the dense route is the stem wgrad kernel it reproduces (44 lanes); D_PB keeps mmh_conv2d_wgrad
    assert {c for n, c in seen if n == "mmh_conv7_stem_sparse_wgrad"} == {44}, seen


def test_sparse_wgrad_over_several_tiles_per_split_is_the_dense_stem_wgrad(dev):
    """B = 8 at 64 x 64: 256 tiles of 2 x 64 pixels in 73 splits, four tiles per split (the last split: none) - the list of
    a split's active tiles with ranks above 0, the register prefetch of the next tile and the reuse of the LDS image across
    tiles all run; dw still equals mmh_conv7_stem_wgrad bit for bit, on a fully dense input (every tile listed) and on pose
    maps (some tiles of a split skipped), with accumulate 0 and 1"""
    from mmhand_amd import lib as L, ops
    Bn, C = 8, 44
    d = ops.conv_desc(Bn, H, W, C, 64, 7, 1, 3, True)
    nb = L.load().mmh_conv7_stem_sparse_wgrad_ws_bytes(ctypes.byref(d))
    assert nb == 73 * 49 * C * 64 * 4 and Bn * (H // 2) * (W // 64) == 256        # ceil(256 / 73) = 4 tiles per split
    g = torch.Generator(device="cpu").manual_seed(91)
    dy = torch.randn((Bn, H, W, 64), generator=g).to(dev)
    base = torch.randn((7, 7, C, 64), generator=g).to(dev)
    uv = torch.rand((Bn * 42, 2), generator=g, dtype=torch.float64) * 90 - 13     # some joints outside: all-zero lanes too
    pose = torch.zeros((Bn, H, W, C), device=dev)
    pose[..., :42] = ops.pose_heatmaps(uv.contiguous().to(dev), H, W).reshape(Bn, 42, H, W).permute(0, 2, 3, 1)
    for name, x in (("dense", torch.randn((Bn, H, W, C), generator=g).to(dev)), ("pose", pose.contiguous())):
        m = torch.empty((L.load().mmh_stem_activity_bytes(Bn, H, W) // 8,), dtype=torch.int64, device=dev)
        L.call("mmh_stem_activity", ops._ptr(x), Bn, H, W, C, ops._ptr(m), ops._stream())
        if name == "pose":      # per lane, the tiles of a split are neither all listed nor all skipped
            on = torch.stack([((m.view(Bn, H // 8, W // 16) >> c) & 1).amax(dim=2) for c in range(42)])     # [lane, B, block row]
            assert bool((on == 0).any()) and bool((on == 1).any())
        for acc in (0, 1):
            ops._stem_masks.clear()
            dense = ops.raw_conv_wgrad(x, dy, 7, 1, 3, True, out=base.clone() if acc else None)
            ws = torch.full((nb // 4,), float("nan"), device=dev)
            dw = base.clone() if acc else torch.full((7, 7, C, 64), float("nan"), device=dev)
            L.call("mmh_conv7_stem_sparse_wgrad", ctypes.byref(d), ops._ptr(x), ops._ptr(m), ops._ptr(dy), ops._ptr(dw), ops._ptr(ws),
                   nb, acc, ops._stream())
            assert torch.equal(dw, dense), (name, acc, float((dw - dense).abs().max()))


def test_eager_forward_between_graph_replays_reads_the_mask_of_its_own_batch(dev, monkeypatch):
    """--graph_step at full stem width: set_input refills the captured iteration's static pose buffer through a pack kernel
    that takes a raw pointer (the tensor's version does not move), and model.test() in between runs the stem eagerly on that
    buffer.  test() on probe A, a replay, test() on probe B, test() on A again: every image equals the one the dense
    kernels give ("stem_sparse" 0), so no forward ran on the mask of an earlier batch; the sparse fprop did run in test()"""
    from mmhand_amd import lib as L, ops
    from mmhand_amd.mmhand_model import MMHandModel
    from mmhand_amd.options import default_train_opt
    monkeypatch.setenv("MMH_GRAPH_CAPTURE", "1")
    probes = [O.synthetic_batch(B, H, W, seed=950), O.synthetic_batch(B, H, W, seed=951)]
    old = L.get_option("stem_sparse")
    orig = L.call
    res = {}
    try:
        for on in (1, 0):
            L.call("mmh_set_option", b"stem_sparse", on)
            random.seed(3)
            m = MMHandModel(default_train_opt(batchSize=B, ngf=64, ndf=16, n_layers_D=2, G_n_blocks=2, norm="instance",
                                              pool_size=0, no_dropout=True, no_dropout_D=True, graph_step=True, fineSize=H,
                                              name="sparsegraph", checkpoints_dir="/tmp/mmh_pytest_ckpt", local_rank=0))
            imgs, masks, seen = [], [], []

            def spy(name, *a):
                seen.append(name)
                return orig(name, *a)

            def test_on(probe):
                m.set_input(probe)
                masks.append(_mask(m.x_P).clone())
                L.call = spy
                try:
                    m.test()
                finally:
                    L.call = orig
                imgs.append(m.fake_p2.detach().clone())
            for it in range(5):
                m.set_input(O.synthetic_batch(B, H, W, seed=300 + it))
                m.optimize_parameters()
            assert m.graph_error is None and m.graph_replays >= 1, (m.graph_error, m.graph_replays)
            test_on(probes[0])
            n0 = m.graph_replays
            m.set_input(O.synthetic_batch(B, H, W, seed=305))
            m.optimize_parameters()
            assert m.graph_replays == n0 + 1
            test_on(probes[1])
            test_on(probes[0])
            assert ("mmh_conv7_stem_sparse_fprop" in seen) == bool(on), seen
            # the probes' masks differ both ways: a mask kept from the other probe would drop active (tile, lane) pairs
            assert bool((masks[1] & ~masks[0]).any()) and bool((masks[0] & ~masks[1]).any())
            res[on] = imgs
    finally:
        L.call = orig
        L.call("mmh_set_option", b"stem_sparse", old)
    assert not torch.equal(res[0][0], res[0][1]) and not torch.equal(res[0][0], res[0][2])     # another batch, moved weights
    for i, (a, b) in enumerate(zip(res[1], res[0])):
        assert torch.equal(a, b), f"test() number {i + 1}: max diff {float((a - b).abs().max()):.3e}"
