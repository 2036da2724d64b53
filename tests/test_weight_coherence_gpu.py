"""Which weights do the kernels read?  Every fast path reads a DERIVED copy of the fp32 master weights (16-bit twins, flat-K and
stem copies, Winograd-domain filters, BN-folded weights), kept coherent by hand: whatever writes weights must call
ops.bump_weights_epoch().  A writer that forgets gives a forward on weights one step (or many) old - finite, smooth, inside every
16-bit tolerance of the suite.  These tests walk every route that writes weights and ask one question with no tolerance:

    WARM EQUALS COLD.  The model that lived through the route and a fresh model loaded with its master weights run the same
    kernels on the same weights and the same input: their generated images are equal bit for bit.

Every case proves that it could have failed: the master weights moved across the last mutation, and a fresh model loaded with
the weights from BEFORE it (what a one-step-stale cache computes) gives another image."""
import os
import random
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import mmhand_ref as O

pytestmark = pytest.mark.gpu

NETS = ("netG", "netD_PB", "netD_PP")
# precision / path axis: each has other derived copies.  "fp32_direct" has none (the control group).
PATHS = {"fp32_wino": dict(), "fp32_direct": dict(), "bf16": dict(opt_level="O1"), "fp16": dict(opt_level="O1_FP16")}
NO_DROP = dict(no_dropout=True, no_dropout_D=True)


def _opt(**kw):
    from mmhand_amd.options import default_train_opt
    args = dict(batchSize=2, ngf=8, ndf=8, n_layers_D=2, G_n_blocks=2, norm="instance", pool_size=3, name="coherence",
                checkpoints_dir="/tmp/mmh_coherence", local_rank=0)
    args.update(kw)
    return default_train_opt(**args)


@pytest.fixture(params=list(PATHS))
def path(request, dev):
    """(name, option overrides) of one precision path; the process-wide Winograd mode is set for it and put back"""
    from mmhand_amd import ops
    ops.set_winograd_mode("off" if request.param == "fp32_direct" else "all")
    try:
        yield request.param, dict(PATHS[request.param])
    finally:
        ops.set_winograd_mode("all")


def _model(kw):
    from mmhand_amd.mmhand_model import MMHandModel
    return MMHandModel(_opt(**kw))


def _batch(seed, B=2, size=32):
    return O.synthetic_batch(B, size, size, seed=seed)


def _steps(m, n, seed0, size=32):
    out = []
    for i in range(n):
        m.set_input(_batch(seed0 + i, m.opt.batchSize, size))
        m.optimize_parameters()
        out.append([float(v) for v in m.get_current_errors().values()])
    return out


def _snap(m):
    """the master weights now: the three reference-format state dicts (clones) and the flat buffers"""
    return {"sd": {n: OrderedDict((k, v.detach().clone()) for k, v in getattr(m, n).state_dict().items()) for n in NETS},
            "flat": {n: getattr(m, n).flat_param.detach().clone() for n in NETS}}


def _derived(net):
    """derived copies alive right now of weights inside `net`'s flat buffer: (per-weight cache entries, batch entries)"""
    from mmhand_amd import ops
    lo = net.flat_param.data_ptr()
    hi = lo + net.flat_param.numel() * 4
    single = sum(1 for c in ops._DERIVED_CACHES() for k in c if lo <= k[0] < hi)
    batched = sum(len(b.entries) for bs in (ops._wino_batches, ops._lp16_batches) for k, b in bs.items() if k[0] < hi and lo < k[1])
    return single, batched


def _cold(kw, snap, probe):
    """a fresh model of the same options loaded with clones of `snap`: its image of `probe`"""
    m = _model(kw)
    for n in NETS:
        getattr(m, n).load_state_dict(OrderedDict((k, v.clone()) for k, v in snap["sd"][n].items()))
    m.set_input(probe)
    m.test()
    torch.cuda.synchronize()
    return m.fake_p2.detach().clone()


def _warm(m, probe):
    m.set_input(probe)
    m.test()
    return m.fake_p2.detach().clone()


def _check(m, kw, probe, before, name, what=""):
    """warm equals cold, with both proofs of power.  `before`: _snap() taken before the last mutation of the weights.
    ORDER MATTERS: the warm image is taken FIRST.  Constructing or loading any model calls the GLOBAL ops.bump_weights_epoch(),
    which drops every derived copy of every model - built before the warm forward, the cold twin would repair the very
    staleness this check is looking for."""
    warm = _warm(m, probe)
    single, batched = _derived(m.netG)          # counted before a twin's construction empties the caches
    now = _snap(m)
    assert not torch.equal(before["flat"]["netG"], now["flat"]["netG"]), f"{what}: the generator's weights never moved"
    # the path really has the derived copies it is listed for (and the control group really has none)
    if name == "fp32_direct":
        assert single == 0 and batched == 0, (what, single, batched)
    else:
        assert single > 0, f"{what}: path {name} made no derived copy of a generator weight - nothing could be stale"
    cold = _cold(kw, now, probe)
    stale = _cold(kw, before, probe)
    assert not torch.equal(stale, cold), f"{what}: void case - one step of staleness is invisible in the image"
    assert torch.equal(warm, cold), (f"{what}: the live model does not compute what its master weights say "
                                     f"(max |warm - cold| {float((warm - cold).abs().max()):.3e}; "
                                     f"|warm - one-step-stale twin| {float((warm - stale).abs().max()):.3e})")
    return warm


# ----------------------------------------------------------------------------- R1: the eager optimizer step
def test_r1_eager_optimizer_step(path):
    """FlatAdam.step bumps its own network: three steps, check; one more, check"""
    name, kw = path
    kw.update(NO_DROP)
    random.seed(5)
    m = _model(kw)
    probe = _batch(900)
    _steps(m, 2, 100)
    _warm(m, probe)                      # an eager forward between steps marks the caches valid
    before = _snap(m)
    _steps(m, 1, 102)
    _check(m, kw, probe, before, name, "after 3 steps")
    before = _snap(m)
    _steps(m, 1, 103)
    _check(m, kw, probe, before, name, "after 4 steps")


# ----------------------------------------------------------------------------- R2: graph replay
def _into_replays(m, seed0, size=32):
    it = 0
    while m.graph_replays < 2:
        assert it < m._graph_warm + 4 and m.graph_error is None, (it, m.graph_replays, m.graph_error)
        _steps(m, 1, seed0 + it, size)
        it += 1
    assert m.graph_error is None and m._graph is not None and m.graph_replays >= 2
    return seed0 + it


def _r2(name, kw, size=32):
    random.seed(5)
    m = _model(kw)
    probe = _batch(900, size=size)
    seed = _into_replays(m, 100, size)
    n0 = m.graph_replays
    _steps(m, 1, seed, size)             # replay
    first = _warm(m, probe)              # warm only: the first eager forward after the capture finds everything stale
    before = _snap(m)
    _steps(m, 1, seed + 1, size)         # replay: the weights move, the host state must follow
    assert m.graph_replays == n0 + 2 and m.graph_error is None
    warm = _warm(m, probe)
    derived = _derived(m.netG)
    assert torch.equal(warm, _check(m, kw, probe, before, name, "eager forward, replay, eager forward"))
    assert not torch.equal(first, warm)
    before = _snap(m)
    _steps(m, 1, seed + 2, size)         # a third replay, now behind the global bump of the twins' construction
    assert m.graph_replays == n0 + 3 and m.graph_error is None
    _check(m, kw, probe, before, name, "after a third replay")
    return m, derived


@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_r2_graph_replay(path, norm, monkeypatch):
    """--graph_step: a replay runs the Adam kernels on the flat buffers without any host code of FlatAdam.step; an eager
    forward between replays (model.test(), a validation pass) must still read the weights of the last replay"""
    name, kw = path
    monkeypatch.setenv("MMH_GRAPH_CAPTURE", "1")
    kw.update(NO_DROP, norm=norm, graph_step=True)
    _r2(name, kw)


def test_r2_graph_replay_batched_winograd_filters(dev, monkeypatch):
    """the same with F(6x6,3x3) engaged (ngf 32 at 64x64: 16x16 maps, 128 channels), where the filters of a network are
    transformed by ONE launch into buffers its _WinoBatch keeps - the copies a captured step rewrites in every replay"""
    from mmhand_amd import ops
    monkeypatch.setenv("MMH_GRAPH_CAPTURE", "1")
    ops.set_winograd_mode("all")
    assert ops._wino_tile(2, 16, 16, 128, 128, 3, 1, 1, False) == 6 and ops.USE_WINO_BATCH
    kw = dict(NO_DROP, graph_step=True, ngf=32, ndf=32, fineSize=64)
    m, (single, batched) = _r2("fp32_wino", kw, size=64)
    assert batched > 0, "no _WinoBatch learned a generator filter: this case did not reach the batched transform"


# ----------------------------------------------------------------------------- R3: replays, test() and a short batch
SEQ = (2, 2, 2, 2, 2, "T", 2, "T", 1, 2, "T")


def _trajectory(kw, capture, seq, monkeypatch):
    monkeypatch.setenv("MMH_GRAPH_CAPTURE", "1" if capture else "0")
    random.seed(3)
    m = _model(kw)
    probe = _batch(950)
    losses, tests, it = [], [], 0
    for s in seq:
        if s == "T":
            tests.append(_warm(m, probe))
        else:
            m.set_input(_batch(300 + it, B=s))
            m.optimize_parameters()
            losses.append([float(v) for v in m.get_current_errors().values()])
            it += 1
    m._settle_overflow(drain=True)
    torch.cuda.synchronize()
    return m, np.array(losses), tests, {n: getattr(m, n).flat_param.detach().clone() for n in NETS}


@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_r3_replays_with_test_calls_and_a_short_batch(path, norm, monkeypatch):
    """replays, eager forwards and an eager short-batch iteration interleaved: the whole trajectory equals the same calls
    without any capture (dropout on, both sides make the same calls in the same order) - an eager forward between replays
    neither reads stale copies nor frees or re-points anything the graph uses - and test() has no effect on training"""
    name, kw = path
    kw.update(norm=norm, graph_step=True)
    e, le, te, we = _trajectory(kw, False, SEQ, monkeypatch)
    assert e._graph is None and e.graph_replays == 0
    g, lg, tg, wg = _trajectory(kw, True, SEQ, monkeypatch)
    assert g.graph_error is None and g.graph_replays == 4, (g.graph_error, g.graph_replays)   # iterations 4, 5, 6 and 8
    assert len(tg) == 3 and not torch.equal(tg[0], tg[1]) and not torch.equal(tg[1], tg[2])    # the weights moved between them
    for i, (a, b) in enumerate(zip(te, tg)):
        assert torch.equal(a, b), f"test() number {i + 1}: max diff {float((a - b).abs().max()):.3e}"
    assert np.array_equal(le, lg), (le.tolist(), lg.tolist())
    for n in NETS:
        assert torch.equal(we[n], wg[n]), n
    # test() is free of side effects on training: without dropout (test() draws dropout seeds) the trajectory with the
    # three eager forwards equals the one without them
    kw.update(NO_DROP)
    a, la, ta, wa = _trajectory(kw, True, SEQ, monkeypatch)
    b, lb, tb, wb = _trajectory(kw, True, tuple(s for s in SEQ if s != "T"), monkeypatch)
    assert a.graph_error is None and b.graph_error is None and a.graph_replays == b.graph_replays == 4
    assert np.array_equal(la, lb), (la.tolist(), lb.tolist())
    for n in NETS:
        assert torch.equal(wa[n], wb[n]), n


# ----------------------------------------------------------------------------- R4: loading into a live, warm model
@pytest.mark.parametrize("how", ["load_state_dict", "load_network"])
def test_r4_load_into_a_warm_model(path, how, tmp_path):
    """train (warm caches), load ANOTHER saved state into the same object: it computes what a fresh model of that state does"""
    name, kw = path
    kw.update(NO_DROP, checkpoints_dir=str(tmp_path))
    random.seed(5)
    m = _model(kw)
    probe = _batch(900)
    _steps(m, 1, 100)
    saved = _snap(m)
    m.save("latest")
    _steps(m, 2, 101)
    _warm(m, probe)
    before = _snap(m)                    # the control: a twin of the state the load replaces
    if how == "load_state_dict":
        for n in NETS:
            getattr(m, n).load_state_dict(OrderedDict((k, v.clone()) for k, v in saved["sd"][n].items()))
    else:
        m.load_network()
    for n in NETS:
        assert torch.equal(getattr(m, n).flat_param, saved["flat"][n]), n
    _check(m, kw, probe, before, name, how)


# ----------------------------------------------------------------------------- R5: save / resume
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph_step"])
def test_r5_resume_continues_the_run(path, graph, tmp_path, monkeypatch):
    """train k, save, train j more == a new model that resumes from the files and trains j: weights, Adam moments, step
    counts, loss scalers and losses, bit for bit (pool_size 0 and no dropout: nothing but the files carries state)"""
    name, kw = path
    monkeypatch.setenv("MMH_GRAPH_CAPTURE", "1")
    kw.update(NO_DROP, pool_size=0, graph_step=graph, checkpoints_dir=str(tmp_path))
    k, j = 2, 5

    def end(m):
        m._settle_overflow(drain=True)
        torch.cuda.synchronize()
        if graph:
            assert m.graph_error is None and m.graph_replays >= 2, (m.graph_error, m.graph_replays)
            assert [int(o.dev_state[0]) for o in m.optimizers] == [o.step_count for o in m.optimizers]
        return {"flat": [getattr(m, n).flat_param.clone() for n in NETS], "m": [o.exp_avg.clone() for o in m.optimizers],
                "v": [o.exp_avg_sq.clone() for o in m.optimizers], "steps": [o.step_count for o in m.optimizers],
                "scaler": m._scaler.clone(), "skipped": m.skipped_steps}
    random.seed(5)
    a = _model(kw)
    _steps(a, k, 100)
    a.save("latest")
    at_save = a.netG.flat_param.clone()
    la = _steps(a, j, 100 + k)
    A = end(a)
    assert not torch.equal(at_save, A["flat"][0])
    b = _model(dict(kw, continue_train=True))
    assert torch.equal(b.netG.flat_param, at_save) and [o.step_count for o in b.optimizers] == [k] * 3
    lb = _steps(b, j, 100 + k)
    B = end(b)
    assert A["steps"] == B["steps"] == [k + j] * 3 and A["skipped"] == B["skipped"]
    assert la == lb, (la, lb)
    for key in ("flat", "m", "v"):
        for n, x, y in zip(NETS, A[key], B[key]):
            assert torch.equal(x, y), (key, n)
    assert torch.equal(A["scaler"], B["scaler"])


# ----------------------------------------------------------------------------- R6: set_logical on a warm generator
def test_r6_set_logical_on_a_warm_generator(path):
    name, kw = path
    kw.update(NO_DROP)
    random.seed(5)
    m = _model(kw)
    probe = _batch(900)
    _steps(m, 2, 100)
    _warm(m, probe)
    before = _snap(m)
    cp = m.netG.model["att"][1]["conv_block_stream2"][1]        # 64 -> 64, 3x3: every path with derived copies has one of it
    assert (cp.cin, cp.cout, cp.k) == (64, 64, 3)
    cp.set_logical(weight=cp.logical_weight().clone() * 1.5 + 0.01)
    _check(m, kw, probe, before, name, "set_logical")


# ----------------------------------------------------------------------------- R7: the folded inference generator
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graphed"])
@pytest.mark.parametrize("lp", [False, True], ids=["fp32", "bf16"])
def test_r7_inference_generator_refold(lp, use_graph, dev):
    """BatchNorm folded into the convs (and their derived copies, and a captured graph that reads them by pointer): after a
    training step on the source network and refold(), the generator equals a fresh InferenceGenerator of the same weights"""
    from mmhand_amd import ops
    from mmhand_amd.inference import InferenceGenerator
    ops.set_winograd_mode("all")
    kw = dict(NO_DROP, norm="batch", **({"opt_level": "O1"} if lp else {}))
    random.seed(5)
    m = _model(kw)
    _steps(m, 2, 100)
    b = _batch(900)
    inputs = [b["H1"].to(dev), torch.cat((b["P1"], b["P2"]), 1).to(dev), torch.cat((b["D1"], b["D2"]), 1).to(dev)]
    gen = InferenceGenerator(m.netG, use_graph=use_graph, bf16=lp)
    assert gen.folded
    old = gen(inputs).clone()
    assert torch.equal(gen(inputs), old)                    # (graphed: the second call replays)
    flat0 = m.netG.flat_param.clone()
    m.netG.train()
    _steps(m, 1, 102)
    m.netG.eval()
    assert not torch.equal(flat0, m.netG.flat_param)
    gen.refold()
    warm = gen(inputs).clone()                              # taken before a fresh generator's fold bumps the epoch
    cold = InferenceGenerator(m.netG, use_graph=use_graph, bf16=lp)(inputs).clone()
    torch.cuda.synchronize()
    assert not torch.equal(old, cold), "void case: the image before the re-fold equals the one after"
    assert torch.equal(warm, cold), float((warm - cold).abs().max())


# ----------------------------------------------------------------------------- R8: process-wide kernel choices flipped
def test_r8_winograd_mode_flipped_on_a_warm_model(dev):
    """ops.set_winograd_mode on a warm model: the next forward is that of a model born under the new mode"""
    from mmhand_amd import ops
    kw = dict(NO_DROP)
    ops.set_winograd_mode("all")
    try:
        random.seed(5)
        m = _model(kw)
        probe = _batch(900)
        _steps(m, 2, 100)
        seed = 102
        last = _warm(m, probe)
        for mode, name in (("off", "fp32_direct"), ("all", "fp32_wino")):
            ops.set_winograd_mode(mode)
            flipped = _warm(m, probe)
            assert not torch.equal(flipped, last), f"mode {mode}: the flip changed no bit of the image"
            assert torch.equal(flipped, _cold(kw, _snap(m), probe)), mode
            before = _snap(m)
            _steps(m, 1, seed)
            seed += 1
            last = _check(m, kw, probe, before, name, f"a step under mode {mode}")
    finally:
        ops.set_winograd_mode("all")


def test_r8_lp16_shape_flipped_on_a_warm_model(dev):
    """mmh_set_option("lp16_shape"): the 256-channel 16-bit convs move from the halo kernel (19) to the row tiles (17) and
    back under a warm model (ngf 64 at 64x64: 256 channels on 16x16 maps, the halo kernel's tile)"""
    from mmhand_amd import lib, ops
    ops.set_winograd_mode("all")
    kw = dict(NO_DROP, opt_level="O1", ngf=64, fineSize=64)
    assert ops.lp16_v2_ok(256, 256, 3, 1, 1, 0)
    try:
        random.seed(5)
        m = _model(kw)
        probe = _batch(900, size=64)
        _steps(m, 2, 100, size=64)
        _warm(m, probe)
        seed = 102
        for shape in (17, 19):
            lib.check(lib.load().mmh_set_option(b"lp16_shape", shape), "set")
            assert torch.equal(_warm(m, probe), _cold(kw, _snap(m), probe)), shape
            before = _snap(m)
            _steps(m, 1, seed, size=64)
            seed += 1
            _check(m, kw, probe, before, "bf16", f"a step under lp16_shape {shape}")
    finally:
        lib.check(lib.load().mmh_set_option(b"lp16_shape", 19), "set")


# ----------------------------------------------------------------------------- replay state against host state: two more
def test_short_batch_right_after_the_warm_up_does_not_end_the_replays(dev, monkeypatch):
    """the iteration that would be captured is the short last batch of an epoch: the capture waits for a full batch (a
    graph of the short shape would leave every full batch eager for good, silently) - full batches end up replayed, and the
    sequence equals the same one without capture"""
    seq = (2, 2, 2, 1, 2, 2, 2)
    kw = dict(opt_level="O1", graph_step=True)
    e, le, _, we = _trajectory(kw, False, seq, monkeypatch)
    random.seed(3)
    monkeypatch.setenv("MMH_GRAPH_CAPTURE", "1")
    g = _model(kw)
    lg, full_replays = [], 0
    for it, B in enumerate(seq):
        n0 = g.graph_replays
        g.set_input(_batch(300 + it, B=B))
        g.optimize_parameters()
        lg.append([float(v) for v in g.get_current_errors().values()])
        full_replays += (g.graph_replays - n0) if B == 2 else 0
    g._settle_overflow(drain=True)
    torch.cuda.synchronize()
    assert g.graph_error is None
    assert full_replays >= 2, f"{full_replays} of the three full batches behind the short one were replayed"
    assert tuple(g._static_inputs["input_H1"].shape)[0] == 2
    assert np.array_equal(le, np.array(lg)), (le.tolist(), lg)
    for n in NETS:
        assert torch.equal(we[n], getattr(g, n).flat_param), n


def _force_dp_worker(rank, port, tmp):
    """one rank, gloo, MMH_FORCE_DP=1 and --graph_step: see test_force_dp_with_graph_step"""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      MMH_FORCE_DP="1", GLOO_SOCKET_IFNAME="lo")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        random.seed(0)
        m = _model(dict(graph_step=True, checkpoints_dir=tmp))
        out = {"dp": bool(m.dp), "graph_step": bool(m.graph_step)}
        _steps(m, 2, 100)
        m.save("latest")
        st = torch.load(os.path.join(tmp, "coherence", "latest_net_amp.pth"))
        out["saved_steps"] = [st["optimizers"][n]["step"] for n in ("optimizer_G", "optimizer_D_PB", "optimizer_D_PP")]
        out["moved"] = bool(m.optimizer_G.exp_avg.abs().sum() > 0)
        torch.save(out, os.path.join(tmp, "force_dp.pt"))
    finally:
        dist.destroy_process_group()


def test_force_dp_with_graph_step(dev, tmp_path):
    """MMH_FORCE_DP=1 with an initialised one-rank group and --graph_step (opt.distributed unset): the data-parallel path
    wins and the graph step is off - no DevicePool assertion, and the saved Adam step is the one the device took"""
    import torch.multiprocessing as mp
    mp.spawn(_force_dp_worker, args=(29671, str(tmp_path)), nprocs=1, join=True)
    r = torch.load(os.path.join(str(tmp_path), "force_dp.pt"))
    assert r["dp"] and not r["graph_step"], r
    assert r["saved_steps"] == [2, 2, 2] and r["moved"], r
