"""Weight coherence in mode bwd_f2 (--fp32_exact_grads --fp32_exact_fwd wino2), by the protocol of
tests/test_weight_coherence_gpu.py: after each route that writes weights the live model's image equals, bit for bit, the image
of a fresh model built from its master weights - here with the F(2x2,3x3) filters (ops.wino_weights(w, 2), per-epoch cache)
among the derived copies.  ngf 64 at 32x32: 8x8 maps with 256 / 512 channels, so the new forward is engaged (asserted)."""
import random
from collections import OrderedDict

import pytest
import torch

from tests.test_weight_coherence_gpu import NETS, NO_DROP, _batch, _check, _model, _r2, _snap, _steps, _warm

pytestmark = pytest.mark.gpu
KW = dict(NO_DROP, ngf=64, ndf=8, fp32_exact_grads=True, fp32_exact_fwd="wino2")


@pytest.fixture
def wino2(dev, monkeypatch):
    from mmhand_amd import lib, ops
    n = [0]
    real = lib.call

    def spy(name, *a):
        n[0] += name == "mmh_wino_gemm_levels16"
        return real(name, *a)
    monkeypatch.setattr(lib, "call", spy)
    try:
        yield n
    finally:
        ops.set_winograd_mode("all")


def test_eager_adam_step(wino2):
    from mmhand_amd import ops
    kw = dict(KW)
    random.seed(5)
    m = _model(kw)
    assert ops.WINO2_FWD
    probe = _batch(900)
    _steps(m, 2, 100)
    _warm(m, probe)
    before = _snap(m)
    _steps(m, 1, 102)
    _check(m, kw, probe, before, "fp32_wino2", "after 3 steps")
    assert wino2[0] > 0


def test_load_state_dict(wino2):
    kw = dict(KW)
    random.seed(5)
    m = _model(kw)
    probe = _batch(900)
    _steps(m, 2, 100)
    _warm(m, probe)                      # the derived copies of the current weights are alive and valid
    before = _snap(m)
    other = _model(dict(kw, seed=7))     # other weights, handed over in the reference's format
    for n in NETS:
        getattr(m, n).load_state_dict(OrderedDict((k, v.clone()) for k, v in getattr(other, n).state_dict().items()))
    del other
    _check(m, kw, probe, before, "fp32_wino2", "after load_state_dict")
    assert wino2[0] > 0


@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_graph_replay_then_test(wino2, norm, monkeypatch):
    monkeypatch.setenv("MMH_GRAPH_CAPTURE", "1")
    _r2("fp32_wino2", dict(KW, norm=norm, graph_step=True))
    assert wino2[0] > 0
