"""ops.set_winograd_mode("bwd_f2") / --fp32_exact_grads --fp32_exact_fwd wino2: the gradient-exact fp32 hybrid with the forward
of its eligible 3x3 / stride-1 convs on Winograd F(2x2,3x3) whose 16 GEMMs sum on two levels (mmh_wino_gemm_levels16), in
place of the direct two-level implicit GEMM (models/Generator.py:40-113).  Accuracy against float64 per conv, on the
full-size Generator and on a whole training step; engagement from the C-ABI calls; bit-exactness properties; edges; weight
coherence.  Channel counts are those the path is eligible for (Cin * Cout >= ops.WINO2_FWD_MIN = 256 * 256)."""
import os
import random
import statistics
from collections import Counter, OrderedDict

import numpy as np
import pytest
import torch

from oracle import mmhand_ref as O
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture
def f2(dev):
    """mode bwd_f2 for one test; the suite's default ("all", one-level direct kernels) is put back afterwards"""
    from mmhand_amd import ops
    ops.set_winograd_mode("bwd_f2")
    try:
        yield ops
    finally:
        ops.set_winograd_mode("all")


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _f2_conv(ops, x, w, bias, reflect, act, levels):
    """the composition itself (whatever the eligibility threshold says): input transform, 16 GEMMs, output transform"""
    return ops._wino_conv(x, ops.wino_weights(w, 2), bias, w.shape[3], reflect, act, 2, levels16=levels)


# margin over the direct two-level fprop's own error, per contraction depth Cin: see the docstring below
MARGIN = {512: 1.25, 256: 1.48, 128: 1.68}


@pytest.mark.parametrize("with_bias_relu", [False, True], ids=["plain", "bias_relu"])
@pytest.mark.parametrize("reflect", [True, False], ids=["reflect", "zero"])
@pytest.mark.parametrize("cin,cout,hw", [(512, 512, 64), (256, 256, 64), (512, 256, 64), (128, 128, 128)])
def test_f2_two_level_conv_vs_fp64_and_the_direct_two_level_fprop(cin, cout, hw, reflect, with_bias_relu, f2, dev):
    """Relative L1 against float64 (oracle/ops_ref.py, B = 2, seeded) of the new forward, against the same figure of the
    direct two-level fprop ON THE SAME TENSORS, times a margin.

    The margin.  Both paths sum fresh 32-deep fp32 chains folded into a total.  The direct kernel's error shrinks with the
    contraction depth (9 * Cin elements); the Winograd side carries on top of its own, 9x shorter, chains the fp32 roundings
    of its transforms' additions - a floor near 2e-7 that does not depend on Cin.  So the RATIO of the two errors grows as Cin
    falls.  tools/wino2_error_model.py (numpy on the CPU, nothing of the kernels under test) gives
        Cin 512: 2.226e-7 | 2.381e-7, ratio 1.069      Cin 256: 1.754e-7 | 2.213e-7, 1.262      Cin 128: 1.464e-7 | 2.094e-7, 1.430
    (its direct column is what the GPU kernel measures to three digits).  The bar at Cin 512 is the 1.25 the feature was
    specified with = the model's 1.069 x 1.17 of headroom; the bars at 256 and 128 give the model's ratio the same headroom:
    1.262 x 1.17 = 1.48, 1.430 x 1.17 = 1.68.  (At Cin * Cout < 256 * 256 the mode keeps the direct kernel, for speed:
    128 -> 128 is here for the composition, not because the mode runs it.)
    Measured on MI355X over five seeds (tools/ab_wino2_fwd.py --accuracy; direct | F(2x2) two-level (ratio) | one-level (ratio)):
        512->512  reflect plain  2.23e-7 | 2.29e-7 (1.024-1.028) | 6.58e-7 (2.95)     zero bias+relu (1.051-1.054) | (3.02)
        512->256  reflect plain  2.23e-7 | 2.28e-7 (1.025-1.027) | 6.58e-7 (2.95)     zero bias+relu (1.051-1.054) | (3.02)
        256->256  reflect plain  1.76e-7 | 2.12e-7 (1.200-1.203) | 4.69e-7 (2.66)     zero bias+relu (1.225-1.230) | (2.71)
        128->128  reflect plain  1.46e-7 | 2.03e-7 (1.383-1.391) | 3.41e-7 (2.33)     zero bias+relu (1.391-1.402) | (2.34)
    Seed-to-seed scatter of a ratio is 0.3 %; every measured ratio sits below the model's.  Worst ratio over its bar:
    1.054 / 1.25, 1.230 / 1.48, 1.402 / 1.68.  (Measured-plus-a-third would ask 1.41 at Cin 512; the third is the project's
    allowance for scatter it has not measured, and here it was measured.)
    The one-level 16-plane GEMM (what mmh_wino_gemm_levels runs for 16 planes whatever it is asked) must be measurably worse
    at 512 -> 512: that is the proof that the second level runs."""
    ops = f2
    x, w = _rand((2, hw, hw, cin), 11), _rand((3, 3, cin, cout), 12, 0.05)
    bias = _rand((cout,), 13, 0.1) if with_bias_relu else None
    act = 1 if with_bias_relu else 0
    ref = R.conv2d(x, w, bias, 1, 1, reflect, act)
    xd, wd, bd = x.to(dev), w.to(dev), None if bias is None else bias.to(dev)
    ops.bump_weights_epoch()
    e_new = R.rel_l1(_f2_conv(ops, xd, wd, bd, reflect, act, 2).double().cpu(), ref)
    e_one = R.rel_l1(_f2_conv(ops, xd, wd, bd, reflect, act, 1).double().cpu(), ref)
    ops.set_winograd_mode("bwd")        # the parent's direct two-level fprop
    y_dir = ops.raw_conv_fprop(xd, wd, bd, 1, 1, reflect, act)
    e_dir = R.rel_l1(y_dir.double().cpu(), ref)
    ops.set_winograd_mode("bwd_f2")
    y_mode = ops.raw_conv_fprop(xd, wd, bd, 1, 1, reflect, act)
    print(f"\n{cin}->{cout} {hw}x{hw} reflect={reflect} bias+relu={with_bias_relu}: direct {e_dir:.3e} | F(2x2) two-level {e_new:.3e} "
          f"(ratio {e_new / e_dir:.3f}, bar {MARGIN[cin]}) | one-level {e_one:.3e} (ratio {e_one / e_dir:.3f})")
    if cin * cout >= ops.WINO2_FWD_MIN:     # what the mode runs for this shape is the composition measured above
        assert torch.equal(y_mode, _f2_conv(ops, xd, wd, bd, reflect, act, 2))
    else:
        assert torch.equal(y_mode, y_dir)
    assert e_new <= MARGIN[cin] * e_dir, (e_new, e_dir, e_new / e_dir)
    if cin == 512 and cout == 512:
        assert e_one > 2.0 * e_new, (e_one, e_new)


def test_fullsize_generator_gradients_vs_fp64_sketch_bwd_f2(f2, dev):
    """tests/test_fullsize_gpu.py's protocol (tests/golden/fullsize_grad_sketch.npz, 85 tensors) in mode bwd_f2, under the bars
    of the modes "off" and "bwd": output < 1.6e-6, gradient median < 1.3e-3, max < 1.9e-3."""
    import bench
    from mmhand_amd.networks import Generator, logical_grads
    fix = np.load(os.path.join(os.path.dirname(__file__), "golden", "fullsize_grad_sketch.npz"))
    b = {k: v.to(dev) for k, v in bench.sketch_inputs(2, 256, 256, 49).items()}
    g_in = [b["H1"], torch.cat((b["P1"], b["P2"]), 1), torch.cat((b["D1"], b["D2"]), 1)]
    probe = torch.randn(2, 3, 256, 256, generator=torch.Generator().manual_seed(3)).to(dev)
    net = Generator([3, 42, 6], 3, 64, "instance", False, 9).init_weights("normal", 49).to(dev).train()
    net.flatten_parameters()
    out = net(g_in)
    (out * probe).sum().backward()
    errs, oerr = bench.fp64_sketch_distance(fix, logical_grads(net), out.detach().contiguous())
    v = sorted(errs.values())
    print(f"\n[bwd_f2] output {oerr:.2e}; gradients vs fp64: median {statistics.median(v):.2e} max {v[-1]:.2e}")
    assert len(v) == 85
    assert oerr < 1.6e-6 and v[-1] < 1.9e-3 and statistics.median(v) < 1.3e-3, (oerr, v[-1], statistics.median(v))


def _spy(monkeypatch):
    """the C-ABI call spy of tests/test_winograd_step_gpu.py: name -> count, and the argument tuples of the calls of interest"""
    from mmhand_amd import lib
    calls, args = Counter(), []
    real = lib.call

    def spy(name, *a):
        calls[name] += 1
        if name in ("mmh_wino_gemm_levels16", "mmh_conv2d_fprop", "mmh_conv2d_fprop_stats"):
            args.append((name, a))
        return real(name, *a)
    monkeypatch.setattr(lib, "call", spy)
    return calls, args


def test_engagement_generator_forward_and_backward(f2, dev, monkeypatch):
    """Generator (ngf 64, 2 PATBlocks, 64x64 input -> 16x16 maps with 256 / 512 channels): in bwd_f2 every eligible 3x3
    stride-1 fprop goes through mmh_wino_gemm_levels16 and none of those shapes through the direct fprop; the other convs
    stay on the direct kernels; F(6x6,3x3) dgrad and wgrad run as in "bwd"."""
    from mmhand_amd.networks import Generator
    ops = f2
    calls, args = _spy(monkeypatch)
    b = O.synthetic_batch(2, 64, 64, seed=5)
    g_in = [b["H1"].to(dev), torch.cat((b["P1"], b["P2"]), 1).to(dev), torch.cat((b["D1"], b["D2"]), 1).to(dev)]
    net = Generator([3, 42, 6], 3, 64, "instance", False, 2).init_weights("normal", 49).to(dev).train()
    net.flatten_parameters()
    net(g_in).sum().backward()
    f2_shapes = {(a[4], a[5]) for n, a in args if n == "mmh_wino_gemm_levels16"}           # (K, N) = (Cin, Cout)
    n_f2 = calls["mmh_wino_gemm_levels16"]
    assert n_f2 >= 6 * 2 and f2_shapes and all(k * n >= ops.WINO2_FWD_MIN for k, n in f2_shapes), (n_f2, f2_shapes)
    for n, a in args:       # no direct fprop of an eligible shape
        if n != "mmh_wino_gemm_levels16":
            d = a[0]._obj
            elig = (d.kh == 3 and d.stride == 1 and d.pad == 1 and d.H % 2 == 0 and d.W % 2 == 0 and d.H >= 4 and d.W >= 4
                    and d.Cin % 32 == 0 and d.Cout % 32 == 0 and d.Cout >= 64 and d.Cin * d.Cout >= ops.WINO2_FWD_MIN)
            assert not elig, (d.Cin, d.Cout, d.H, d.W)
    assert calls["mmh_conv2d_fprop"] + calls["mmh_conv2d_fprop_stats"] > 0            # stems / stride-2 convs: direct, as in "bwd"
    assert calls["mmh_wino_gemm"] == 0, calls                                           # no F(6x6) forward GEMM
    assert calls["mmh_wino_gemm_levels"] >= 6 * 2 and calls["mmh_wino_wgrad_gemm"] >= 6 * 2, calls       # F(6x6) dgrad / wgrad
    assert calls["mmh_wino_input_dy"] >= 6 * 2, calls


def test_unknown_mode_still_raises(dev):
    from mmhand_amd import ops
    with pytest.raises(ValueError):
        ops.set_winograd_mode("bwd_f4")


def test_bit_exactness_run_to_run_and_batch_independence(f2, dev):
    ops = f2
    x, w, bias = _rand((3, 16, 24, 256), 1).to(dev), _rand((3, 3, 256, 256), 2, 0.05).to(dev), _rand((256,), 3, 0.1).to(dev)
    y3 = ops.raw_conv_fprop(x, w, bias, 1, 1, True, 1)
    assert torch.equal(y3, ops.raw_conv_fprop(x, w, bias, 1, 1, True, 1))
    y1 = ops.raw_conv_fprop(x[:1].contiguous(), w, bias, 1, 1, True, 1)
    assert torch.equal(y1[0], y3[0])


@pytest.mark.parametrize("B,H,W,cin,cout,reflect", [(2, 12, 20, 256, 256, True), (2, 4, 4, 256, 256, True), (1, 4, 4, 512, 512, False),
                                                     (2, 8, 8, 32, 96, True), (2, 8, 8, 32, 96, False)],
                         ids=["H_ne_W", "4x4", "4x4_zero", "cin32_cout96", "cin32_cout96_zero"])
def test_edges_vs_fp64(B, H, W, cin, cout, reflect, f2, dev, monkeypatch):
    """H != W, the 4x4 minimum, Cin = 32 with Cout = 96 (below the speed threshold: the threshold is lowered for this test so
    that the mode takes them), against float64.  The bar is absolute here: on a 4x4 image with zero padding 12 of 16 pixels
    lose taps, the direct kernel's effective contraction - and with it its error - shrinks (1.94e-7 at Cin 512 against 2.22e-7
    on a 64x64 image), so a ratio to it is not the ratio the model describes.  The bar is the F(2x2) column of
    tools/wino2_error_model.py for that Cin (512: 2.381e-7, 256: 2.213e-7, 32: 1.963e-7) x the per-conv test's 1.17 headroom.
    Measured: H != W 2.03e-7, 4x4 reflect 1.67e-7, 4x4 zero at 512 2.47e-7 (bar 2.79e-7)."""
    model_f2 = {512: 2.381e-7, 256: 2.213e-7, 32: 1.963e-7}
    ops = f2
    monkeypatch.setattr(ops, "WINO2_FWD_MIN", 0)
    calls, _ = _spy(monkeypatch)
    x, w, bias = _rand((B, H, W, cin), 21), _rand((3, 3, cin, cout), 22, 0.05), _rand((cout,), 23, 0.1)
    ref = R.conv2d(x, w, bias, 1, 1, reflect, 1)
    y = ops.raw_conv_fprop(x.to(dev), w.to(dev), bias.to(dev), 1, 1, reflect, 1)
    assert calls["mmh_wino_gemm_levels16"] == 1 and calls["mmh_conv2d_fprop"] == 0, calls
    ops.set_winograd_mode("bwd")
    e_dir = R.rel_l1(ops.raw_conv_fprop(x.to(dev), w.to(dev), bias.to(dev), 1, 1, reflect, 1).double().cpu(), ref)
    e = R.rel_l1(y.double().cpu(), ref)
    print(f"\n{cin}->{cout} {H}x{W}: direct {e_dir:.3e} | F(2x2) two-level {e:.3e}")
    assert e <= 1.17 * model_f2[cin], (e, e_dir)


def test_odd_size_falls_back_to_the_direct_kernel(f2, dev, monkeypatch):
    ops = f2
    calls, _ = _spy(monkeypatch)
    x, w, bias = _rand((2, 9, 16, 256), 1).to(dev), _rand((3, 3, 256, 256), 2, 0.05).to(dev), _rand((256,), 3, 0.1).to(dev)
    y = ops.raw_conv_fprop(x, w, bias, 1, 1, True, 1)
    assert calls["mmh_wino_gemm_levels16"] == 0 and calls["mmh_conv2d_fprop"] == 1, calls
    ops.set_winograd_mode("bwd")
    assert torch.equal(y, ops.raw_conv_fprop(x, w, bias, 1, 1, True, 1))


def test_mode_switch_leaves_all_untouched(dev):
    """all -> bwd_f2 -> all: the "all" results before and after are identical (F(6x6) conv, a stride-2 direct conv)"""
    from mmhand_amd import ops
    ops.set_winograd_mode("all")
    x, w = _rand((2, 16, 16, 256), 1).to(dev), _rand((3, 3, 256, 256), 2, 0.05).to(dev)
    run = lambda: (ops.raw_conv_fprop(x, w, None, 1, 1, True, 1), ops.raw_conv_fprop(x, w, None, 2, 1, False, 0))     # noqa: E731
    a = run()
    try:
        ops.set_winograd_mode("bwd_f2")
        mid = run()
    finally:
        ops.set_winograd_mode("all")
    b = run()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], mid[0])        # the switch did change the kernels in between


# ----------------------------------------------------------------------------- whole training steps
NGF, SIZE, NB, NLD = 64, 64, 2, 3


def _opt(**kw):
    from mmhand_amd.options import default_train_opt
    args = dict(batchSize=2, ngf=NGF, ndf=NGF, n_layers_D=NLD, G_n_blocks=NB, norm="instance", no_dropout=True,
                no_dropout_D=True, pool_size=2, name="wino2step", checkpoints_dir="/tmp/mmh_pytest_ckpt",
                local_rank=0, fineSize=SIZE, opt_level="O0", fp32_exact_grads=True, fp32_exact_fwd="wino2")
    args.update(kw)
    return default_train_opt(**args)


@pytest.fixture
def restore_mode():
    from mmhand_amd import ops
    try:
        yield
    finally:
        ops.set_winograd_mode("all")


@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_optimize_parameters_wino2_vs_fp64_oracle(norm, dev, monkeypatch, restore_mode):
    """One full optimize_parameters() with --fp32_exact_grads --fp32_exact_fwd wino2 against the float64 StepOracle, under the
    bars tests/test_lp16_step_gpu.py applies to the "bwd" path: six losses 1e-3, generated image 2e-5, per Generator gradient
    tensor max(1e-3, 1.5 x PyTorch's own fp32 distance on that tensor, tests/golden/lp16_cond.npz) with all but three below
    1e-3.  The fixture's per-tensor figures were recorded under --norm instance; --norm batch is held to the same ones."""
    from mmhand_amd import ops
    from mmhand_amd.mmhand_model import MMHandModel
    from tests.golden import recipe as RC
    from tests.golden.make_lp16_cond import SEED, nets
    from tests.test_model_gpu import logical_grads
    calls, _ = _spy(monkeypatch)
    model = MMHandModel(_opt(norm=norm))
    assert ops.WINO2_FWD and not ops.WINOGRAD_FPROP and ops.USE_WINOGRAD
    if norm == "instance":      # the fixture's weights (its per-tensor figures belong to them); --norm batch: the seeded init
        for net, sd in zip((model.netG, model.netD_PB, model.netD_PP, model.vgg), nets()):
            net.load_state_dict(sd)
    sds = [OrderedDict((k, v.cpu()) for k, v in n.state_dict().items()) for n in (model.netG, model.netD_PB, model.netD_PP)]
    vgg = OrderedDict((k, v.cpu()) for k, v in model.vgg.state_dict().items())
    f64 = lambda sd: OrderedDict((k, v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items())  # noqa: E731
    o64 = O.StepOracle(f64(sds[0]), f64(sds[1]), f64(sds[2]), f64(vgg), norm, False, False, NB, NLD, pool_size=2,
                       rng=random.Random(49))
    random.seed(49)
    batch = O.synthetic_batch(2, SIZE, SIZE, seed=SEED)
    want = list(o64.step({k: v.double() for k, v in batch.items()}).values())
    model.set_input(batch)
    model.optimize_parameters()
    got = [float(v) for v in model.get_current_errors().values()]
    e_img = R.rel_l1(model.fake_p2, o64.fake_p2.detach())
    og = dict((k, t.grad) for k, t in o64.G.named_parameters())
    errs = sorted((R.rel_l1(g.double(), og[k]), k) for k, g in logical_grads(model.netG).items()
                  if not RC.is_null_grad_bias("G", k, norm) and og.get(k) is not None)
    print(f"\n[wino2, --norm {norm}] image {e_img:.2e}; G gradients vs fp64: median {errs[len(errs) // 2][0]:.2e}, "
          f"max {errs[-1][0]:.2e} ({errs[-1][1]})")
    assert np.allclose(got, want, rtol=1e-3), (got, want)
    assert e_img < 2e-5, e_img
    cond = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lp16_cond.npz"))
    for e, k in errs:
        c = float(cond["fp32/" + k]) if "fp32/" + k in cond else 0.0
        assert e <= max(1e-3, 1.5 * c), (k, e, c)
    assert sum(1 for e, _ in errs if e <= 1e-3) >= len(errs) - 3, errs[-5:]
    assert calls["mmh_wino_gemm_levels16"] >= 6 * NB and calls["mmh_wino_gemm"] == 0, calls
    assert calls["mmh_wino_wgrad_gemm"] >= 6 * NB and calls["mmh_wino_input_dy"] >= 6 * NB, calls


@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_graph_step_replays_the_eager_iteration_bit_for_bit_in_wino2(norm, dev, monkeypatch, restore_mode):
    """--graph_step in the new mode: eight iterations (dropout on, changing batches), captured-and-replayed equal to the eager
    form to the bit - losses, every weight, the generated image; at least three iterations were replays"""
    from tests.test_graph_step_gpu import _run
    kw = dict(ngf=64, ndf=16, n_layers_D=2, fineSize=32, pool_size=3, no_dropout=False, no_dropout_D=False, graph_step=True,
              name="wino2graph", norm=norm)
    calls, _ = _spy(monkeypatch)
    eager, l0, s0 = _run(_opt(**kw), 8, False, monkeypatch)
    assert eager._graph is None and eager.graph_replays == 0 and calls["mmh_wino_gemm_levels16"] > 0
    graph, l1, s1 = _run(_opt(**kw), 8, True, monkeypatch)
    assert graph.graph_error is None, graph.graph_error
    assert graph._graph is not None and graph.graph_replays == 8 - graph._graph_warm >= 3, (graph.graph_replays, graph._graph_warm)
    assert np.array_equal(np.array(l0), np.array(l1)), (l0, l1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
