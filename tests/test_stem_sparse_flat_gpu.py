"""The flat-order sparse stem wgrad (stem_sparse.hip, mmh_conv7_stem_sparse_wgrad_flat) against the generic wgrad it stands in
for (mmh_conv2d_wgrad: conv_wgrad_kernel + slab_reduce): bit for bit on floats, exact on integer operands, the routing in
ops.raw_conv_wgrad, and one whole training step with the route on and off.

Shapes (B, H, W), the smallest at which each way the flat split can go wrong shows:
  (3, 24, 48)   P = 3456: 13 splits of 288 pixels, the 13th empty; W % 32 != 0: steps straddle a row end; 288 % (24 * 48) != 0:
                a split boundary in the middle of an image
  (2, 16, 16)   two rows per 32-pixel step
  (2, 64, 64)   the shape of tests/test_stem_sparse_gpu.py
  (1, 16, 256)  the workload's row length: a split per row, eight splits per row of mask blocks
H % 8 == 0 and W % 16 == 0 make H * W a multiple of 128, so a 32-pixel step never holds pixels of two images (a half on the next
row is the only straddle there is); image boundaries fall between steps and, at (3, 24, 48), inside splits."""
import ctypes
import random
from collections import OrderedDict

import pytest
import torch

from oracle import mmhand_ref as O
from oracle import ops_ref as R
from tests.golden import recipe as RC

pytestmark = pytest.mark.gpu
SHAPES = ((3, 24, 48), (2, 16, 16), (2, 64, 64), (1, 16, 256))
# name -> (Cin, dense lanes, pose lanes); every other lane is all zero
CFGS = {"24lo": (24, (0, 1, 2), tuple(range(3, 24))), "24hi": (24, (21, 22, 23), tuple(range(21))),
        "44": (44, (), tuple(range(42))), "8": (8, tuple(range(6)), (6, 7))}


def _splits(Bn, H, W, C):
    from mmhand_amd import lib as L, ops
    d = ops.conv_desc(Bn, H, W, C, 64, 7, 1, 3, True)
    nb = L.load().mmh_conv7_stem_sparse_wgrad_flat_ws_bytes(ctypes.byref(d))
    assert nb == L.load().mmh_conv2d_wgrad_ws_bytes(ctypes.byref(d)) and nb % (49 * C * 64 * 4) == 0
    return nb // (49 * C * 64 * 4)


def test_the_shapes_hold_the_cases_they_are_here_for():
    for Bn, H, W in SHAPES:
        for C in (24, 44, 8):
            assert _splits(Bn, H, W, C) > 1, (Bn, H, W, C)
    assert _splits(3, 24, 48, 24) == 13                  # 288 pixels each: 12 * 288 = P, the 13th owns nothing
    pps = -(-(-(-3456 // 13)) // 32) * 32
    assert pps == 288 and 12 * pps == 3 * 24 * 48 and 48 % 32 != 0 and pps % (24 * 48) != 0
    assert _splits(2, 16, 16, 24) == 2 and 32 // 16 == 2
    assert _splits(1, 16, 256, 24) == 16                 # 256 pixels each: one row, 8 splits per 8-row mask block


def _pose_lanes(Bn, H, W, n, dev):
    """n pose lanes [Bn, H, W, n]: joints at a corner (the mirror image enters the halo), at the right and the bottom border,
    two joints 4 px apart, twelve joints in one 8 x 16 block of the last image; the rest all zero"""
    from mmhand_amd import ops
    uv = torch.full((Bn, n, 2), -100.0, dtype=torch.float64)
    spots = [(1.5, 1.5), (W - 1.5, H / 2), (W / 2, H - 1.5), (W / 2 - 2.0, H / 3), (W / 2 + 2.0, H / 3)]
    for i, s in enumerate(spots[:n]):
        uv[0, i] = torch.tensor(s)
    bx = 16.0 if W >= 32 else 0.0
    for i in range(max(0, min(12, n - 5))):
        uv[Bn - 1, 5 + i] = torch.tensor([bx + 2.0 + (i % 4) * 3, 8.0 + 1.0 + (i // 4) * 2])
    sigma = 6.0 if H >= 64 else 1.5
    maps = ops.pose_heatmaps(uv.reshape(Bn * n, 2).contiguous().to(dev), H, W, sigma).reshape(Bn, n, H, W)
    return maps.permute(0, 2, 3, 1)


def _inputs(Bn, H, W, cfg, dev, seed):
    C, dense, pose = CFGS[cfg]
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.zeros((Bn, H, W, C), device=dev)
    x[..., list(pose)] = _pose_lanes(Bn, H, W, len(pose), dev)
    if dense:
        x[..., list(dense)] = torch.randn((Bn, H, W, len(dense)), generator=g).to(dev)
    x = x.contiguous()
    e = x.clone()
    e[..., (dense or pose)[0]] = 0.0                    # a lane that was active everywhere: all zero
    e[:, H // 2:, :, pose[0]] = -0.0                    # -0.0 counts as zero in the mask and in the products (before the
    e[..., pose[-1]] = 0.0                              # single pixels: with two pose lanes pose[0] is pose[-2])
    e[0, 0, 0, pose[-1]] = 0.75                         # one pixel at (0, 0)
    e[..., pose[-2]] = 0.0
    e[Bn - 1, H - 1, W - 1, pose[-2]] = -1.25           # one pixel at (H - 1, W - 1) of the last image
    e[0, 2, 5, (dense or pose)[-1]] = -0.0
    return {"pose": x, "dense": torch.randn((Bn, H, W, C), generator=g).to(dev).contiguous(), "edge": e.contiguous()}


def _mask(x):
    from mmhand_amd import lib as L, ops
    m = torch.full((L.load().mmh_stem_activity_bytes(*x.shape[:3]) // 8,), -1, dtype=torch.int64, device=x.device)
    L.call("mmh_stem_activity", ops._ptr(x), *x.shape, ops._ptr(m), ops._stream())
    return m


def _generic(x, dy, out=None):
    """ops.raw_conv_wgrad without a mask, on the generic route (mmh_conv2d_wgrad) also where the stem wgrad kernel would run"""
    from mmhand_amd import lib as L, ops
    ops._stem_masks.clear()
    calls, orig, old = [], L.call, ops.USE_STEM_WGRAD

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)
    L.call, ops.USE_STEM_WGRAD = spy, False
    try:
        dw = ops.raw_conv_wgrad(x, dy, 7, 1, 3, True, out=out)
    finally:
        L.call, ops.USE_STEM_WGRAD = orig, old
    assert [c for c in calls if "wgrad" in c] == ["mmh_conv2d_wgrad"], calls
    return dw


def _flat(x, dy, out=None):
    """the entry point itself, on a workspace and a dw full of NaN"""
    from mmhand_amd import lib as L, ops
    Bn, H, W, C = x.shape
    d = ops.conv_desc(Bn, H, W, C, 64, 7, 1, 3, True)
    assert L.load().mmh_conv7_stem_sparse_wgrad_flat_supported(ctypes.byref(d)) == 1
    nb = L.load().mmh_conv7_stem_sparse_wgrad_flat_ws_bytes(ctypes.byref(d))
    ws = torch.full((nb // 4,), float("nan"), device=x.device)
    dw = out if out is not None else torch.full((7, 7, C, 64), float("nan"), device=x.device)
    L.call("mmh_conv7_stem_sparse_wgrad_flat", ctypes.byref(d), ops._ptr(x), ops._ptr(_mask(x)), ops._ptr(dy), ops._ptr(dw),
           ops._ptr(ws), nb, int(out is not None), ops._stream())
    return dw


@pytest.mark.parametrize("cfg", list(CFGS))
@pytest.mark.parametrize("shape", SHAPES)
def test_flat_wgrad_is_the_generic_wgrad_bit_for_bit(shape, cfg, dev):
    Bn, H, W = shape
    C = CFGS[cfg][0]
    g = torch.Generator(device="cpu").manual_seed(7 + C + H)
    dy = torch.randn((Bn, H, W, 64), generator=g).to(dev)
    base = torch.randn((7, 7, C, 64), generator=g).to(dev)
    for name, x in _inputs(Bn, H, W, cfg, dev, 3 + W).items():
        if name == "pose":          # the pose lanes are neither everywhere nor nowhere: steps are skipped and steps are taken
            m = _mask(x)
            on = torch.stack([(m >> c) & 1 for c in CFGS[cfg][2]])
            assert bool((on == 0).any()) and bool((on == 1).any())
        want, got = _generic(x, dy), _flat(x, dy)
        assert torch.equal(got, want), (name, float((got - want).abs().max()))
        want, got = _generic(x, dy, out=base.clone()), _flat(x, dy, out=base.clone())
        assert torch.equal(got, want), (name, "accumulate", float((got - want).abs().max()))


@pytest.mark.parametrize("cfg", ["24lo", "44"])
@pytest.mark.parametrize("shape", SHAPES)
def test_flat_wgrad_is_exact_on_integer_operands(shape, cfg, dev):
    """x in {0, 1, 2} (pose lanes on the heat maps' supports), dy in {-2 .. 2}: every partial sum is an integer below 2^24, so
    the fp64 oracle, the generic kernel and the flat kernel agree exactly"""
    Bn, H, W = shape
    C, dense, pose = CFGS[cfg]
    g = torch.Generator(device="cpu").manual_seed(21 + C + W)
    dy = torch.randint(-2, 3, (Bn, H, W, 64), generator=g).float().to(dev)
    ins = _inputs(Bn, H, W, cfg, dev, 5)
    xs = {"pose": torch.ceil(ins["pose"].clamp(0, 1) * 2), "dense": torch.randint(0, 3, (Bn, H, W, C), generator=g).float().to(dev)}
    if dense:
        xs["pose"][..., list(dense)] = torch.randint(0, 3, (Bn, H, W, len(dense)), generator=g).float().to(dev)
    for name, x in xs.items():
        x = x.contiguous()
        ref = R.conv2d_grads(x.cpu(), torch.zeros((7, 7, C, 64)), None, dy.cpu(), 1, 3, True)[2].float()
        assert float(ref.abs().max()) < 2 ** 24
        assert torch.equal(_generic(x, dy).cpu(), ref), name
        got = _flat(x, dy).cpu()
        assert torch.equal(got, ref), (name, float((got - ref).abs().max()))
        base = torch.randint(-3, 4, ref.shape, generator=g).float()
        assert torch.equal(_flat(x, dy, out=base.clone().to(dev)).cpu(), ref + base), name


def test_raw_conv_wgrad_routes_the_flat_kernel_where_the_dense_route_is_generic(dev):
    from mmhand_amd import lib as L, ops
    Bn, H, W = 2, 64, 64
    g = torch.Generator(device="cpu").manual_seed(77)
    dy = torch.randn((Bn, H, W, 64), generator=g).to(dev)
    old = L.get_option("stem_sparse_flat")
    orig = L.call
    wgrads = ("mmh_conv7_stem_sparse_wgrad_flat", "mmh_conv7_stem_sparse_wgrad", "mmh_conv7_stem_wgrad", "mmh_conv2d_wgrad")
    try:
        for cfg, opt, ask, want in (("24lo", 1, True, "mmh_conv7_stem_sparse_wgrad_flat"), ("24hi", 1, True, "mmh_conv7_stem_sparse_wgrad_flat"),
                                    ("24lo", 0, True, "mmh_conv2d_wgrad"), ("24lo", 1, False, "mmh_conv2d_wgrad"),
                                    ("44", 1, True, "mmh_conv7_stem_sparse_wgrad"), ("44", 0, True, "mmh_conv7_stem_sparse_wgrad")):
            x = _inputs(Bn, H, W, cfg, dev, 11)["pose"]
            dense = _generic(x, dy) if cfg != "44" else None
            L.call("mmh_set_option", b"stem_sparse_flat", opt)
            ops._stem_masks.clear()
            if ask:
                assert ops.stem_mask_request(x) is not None
            calls = []

            def spy(name, *a):
                calls.append(name)
                return orig(name, *a)
            L.call = spy
            try:
                routed = ops.raw_conv_wgrad(x, dy, 7, 1, 3, True)
            finally:
                L.call = orig
            assert [c for c in calls if c in wgrads] == [want], (cfg, opt, ask, calls)
            if dense is None:       # 44 lanes: the dense route is the stem wgrad kernel
                ops._stem_masks.clear()
                dense = ops.raw_conv_wgrad(x, dy, 7, 1, 3, True)
            assert torch.equal(routed, dense), (cfg, opt, ask)
    finally:
        L.call = orig
        L.call("mmh_set_option", b"stem_sparse_flat", old)
        ops._stem_masks.clear()


def test_training_step_is_the_same_step_with_the_flat_wgrad(dev):
    """one optimize_parameters with "stem_sparse_flat" 1 and one with 0 (two-block Generator and D_PB at 64 x 64, B = 2, full
    width): the losses, fake_p2 and every parameter of the three networks after the step are equal bit for bit, and the new
    entry point ran for D_PB's 24 lanes and for nothing else"""
    from mmhand_amd import lib as L, ops
    from mmhand_amd.mmhand_model import MMHandModel
    from mmhand_amd.options import default_train_opt
    Bn, H, W = 2, 64, 64
    res = {}
    old = L.get_option("stem_sparse_flat")
    orig = L.call
    try:
        for on in (1, 0):
            L.call = orig
            L.call("mmh_set_option", b"stem_sparse_flat", on)
            opt = default_train_opt(batchSize=Bn, ngf=64, ndf=64, n_layers_D=2, G_n_blocks=2, norm="instance", pool_size=0,
                                    no_dropout=True, no_dropout_D=True, name="sparse_flat", checkpoints_dir="/tmp/mmh_pytest_ckpt",
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
                if name == "mmh_conv7_stem_sparse_wgrad_flat":
                    seen.append(a[0]._obj.Cin)
                return orig(name, *a)
            L.call = spy
            model.set_input(O.synthetic_batch(Bn, H, W, seed=100))
            model.optimize_parameters()
            L.call = orig
            losses = [float(v) for v in model.get_current_errors().values()]
            params = [p.detach().clone() for n in (model.netG, model.netD_PB, model.netD_PP) for p in n.parameters()]
            res[on] = (model.fake_p2.detach().clone(), losses, params, seen)
    finally:
        L.call = orig
        L.call("mmh_set_option", b"stem_sparse_flat", old)
    assert torch.equal(res[1][0], res[0][0])
    assert res[1][1] == res[0][1], (res[1][1], res[0][1])
    for a, b in zip(res[1][2], res[0][2]):
        assert torch.equal(a, b)
    assert res[0][3] == [] and res[1][3] and set(res[1][3]) == {24}, (res[0][3], res[1][3])
