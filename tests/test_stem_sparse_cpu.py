"""Host side of the compacted-channel stem kernels (stem_sparse.hip): which shapes the queries accept, the sizes they report,
the "stem_sparse" switch, and the argument checks that come before any launch.  No GPU."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def L():
    from mmhand_amd import lib
    try:
        lib.load()
    except OSError as e:        # the library is built by __graft_entry__.build()
        pytest.fail(f"libmmhand_hip.so is not built: {e}")
    return lib


def _mk(L, B, H, W, Cin, Cout=64, k=7, stride=1, pad=3, refl=True, dt=None, x_cs=None, y_cs=None):
    return L.ConvDesc(B, H, W, Cin, Cout, k, k, stride, pad, L.PAD_REFLECT if refl else L.PAD_ZERO,
                      (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1, x_cs or Cin, y_cs or Cout,
                      L.F32 if dt is None else dt)


def test_activity_bytes(L):
    l = L.load()
    assert l.mmh_stem_activity_bytes(32, 256, 256) == 32 * 32 * 16 * 8
    assert l.mmh_stem_activity_bytes(2, 64, 64) == 2 * 8 * 4 * 8
    assert l.mmh_stem_activity_bytes(1, 8, 16) == 8
    for bad in ((2, 60, 64), (2, 64, 72), (0, 64, 64), (2, 0, 64), (-1, 64, 64)):
        assert l.mmh_stem_activity_bytes(*bad) == 0, bad


def test_supported_and_workspace_across_shapes(L):
    l = L.load()
    by = ctypes.byref
    f, g, ws = l.mmh_conv7_stem_sparse_fprop_supported, l.mmh_conv7_stem_sparse_wgrad_supported, l.mmh_conv7_stem_sparse_wgrad_ws_bytes
    for B, H, W, C in ((32, 256, 256, 44), (64, 256, 256, 24), (2, 64, 64, 44), (2, 64, 64, 24), (2, 64, 64, 48), (1, 16, 64, 4), (3, 32, 128, 8)):
        d = _mk(L, B, H, W, C)
        assert f(by(d)) == 1 and g(by(d)) == 1, (B, H, W, C)
        # the dense stem wgrad's tiles (2 x 64 pixels) and split rule: 512 workgroups over its groups of filter rows
        tiles = B * (H // 2) * (W // 64)
        groups = -(-7 // max(1, min(7, 448 // (7 * C))))
        assert ws(by(d)) == min(max(512 // groups, 1), tiles) * 49 * C * 64 * 4
        # ... which IS the dense kernel's, where that kernel runs: its workspace is the padded input + the same slabs + 256
        if l.mmh_conv7_stem_wgrad_supported(by(d)):
            assert l.mmh_conv7_stem_wgrad_ws_bytes(by(d)) == B * (H + 6) * (W + 6) * C * 4 + ws(by(d)) + 256
    assert ws(by(_mk(L, 2, 64, 64, 44))) == 64 * 49 * 44 * 64 * 4           # one tile per slab at the test shape
    assert ws(by(_mk(L, 32, 256, 256, 44))) == 73 * 49 * 44 * 64 * 4
    assert l.mmh_conv7_stem_wgrad_supported(by(_mk(L, 32, 256, 256, 44))) == 1 and l.mmh_conv7_stem_wgrad_supported(by(_mk(L, 64, 256, 256, 24))) == 0
    d = _mk(L, 2, 64, 48, 44)           # whole 16 x 16 tiles but no whole 2 x 64 tiles: forward only
    assert f(by(d)) == 1 and g(by(d)) == 0 and ws(by(d)) == 0
    no = [_mk(L, 2, 64, 64, 44, Cout=32), _mk(L, 2, 64, 64, 44, k=3, pad=1), _mk(L, 2, 64, 64, 44, refl=False),
          _mk(L, 2, 64, 64, 44, dt=L.BF16), _mk(L, 2, 64, 64, 52), _mk(L, 2, 64, 64, 42), _mk(L, 2, 64, 72, 44),
          _mk(L, 2, 60, 64, 44), _mk(L, 2, 64, 64, 44, x_cs=40)]
    for d in no:
        assert f(by(d)) == 0 and g(by(d)) == 0 and ws(by(d)) == 0, (d.H, d.W, d.Cin, d.Cout, d.kh)
    # the fprop copies the dense kernel's 16 x 16 tile: whole tiles only; the wgrad needs H % 8 == 0 (mask rows), W % 64 == 0
    d = _mk(L, 2, 72, 64, 44)
    assert l.mmh_conv2d_fprop_stats_chunks(by(d)) == 0 and f(by(d)) == 0 and g(by(d)) == 1
    assert f(None) == 0 and g(None) == 0 and ws(None) == 0


def test_switch_and_conv_levels(L):
    l = L.load()
    by = ctypes.byref
    d = _mk(L, 2, 64, 64, 44)
    old = L.get_option("stem_sparse")
    try:
        assert l.mmh_set_option(b"stem_sparse", 0) == 0
        assert l.mmh_conv7_stem_sparse_fprop_supported(by(d)) == 0 and l.mmh_conv7_stem_sparse_wgrad_supported(by(d)) == 0
        assert l.mmh_conv7_stem_sparse_wgrad_ws_bytes(by(d)) > 0        # the size does not depend on the switch
    finally:
        assert l.mmh_set_option(b"stem_sparse", old) == 0
    assert l.mmh_conv7_stem_sparse_fprop_supported(by(d)) == 1
    # two-level summation cuts the dense chain at filter phases the compacted list does not have: forward stays dense
    lv = L.get_option("conv_levels")
    try:
        assert l.mmh_set_option(b"conv_levels", 2) == 0
        assert l.mmh_conv7_stem_sparse_fprop_supported(by(d)) == 0 and l.mmh_conv7_stem_sparse_wgrad_supported(by(d)) == 1
    finally:
        assert l.mmh_set_option(b"conv_levels", lv) == 0
    # the dense stem kernel is the twin: without it the sparse fprop has nothing to be identical to
    sf = L.get_option("stem_f32")
    try:
        assert l.mmh_set_option(b"stem_f32", 0) == 0
        assert l.mmh_conv7_stem_sparse_fprop_supported(by(d)) == 0
    finally:
        assert l.mmh_set_option(b"stem_f32", sf) == 0


def test_null_and_misaligned_arguments_are_rejected(L):
    l = L.load()
    by = ctypes.byref
    p = ctypes.c_void_p
    d = _mk(L, 2, 64, 64, 44)
    ok, odd8, odd4 = p(4096), p(4096 + 8), p(4096 + 4)
    # mmh_stem_activity(x, B, H, W, C, mask, stream)
    for args in ((None, 2, 64, 64, 44, ok), (ok, 2, 64, 64, 44, None), (odd8, 2, 64, 64, 44, ok), (ok, 2, 64, 64, 44, odd4),
                 (ok, 2, 64, 64, 42, ok), (ok, 2, 64, 64, 52, ok), (ok, 2, 64, 64, 0, ok), (ok, 2, 60, 64, 44, ok),
                 (ok, 2, 64, 40, 44, ok), (ok, 0, 64, 64, 44, ok)):
        assert l.mmh_stem_activity(*args, None) != 0, args
        assert b"mmh_stem_activity" in l.mmh_last_error()
    # mmh_conv7_stem_sparse_fprop(d, x, mask, w, bias, y, stats, stream)
    for args in ((None, ok, ok, ok, None, ok, ok), (by(d), None, ok, ok, None, ok, ok), (by(d), ok, None, ok, None, ok, ok),
                 (by(d), ok, ok, None, None, ok, ok), (by(d), ok, ok, ok, None, None, ok), (by(d), ok, odd4, ok, None, ok, ok),
                 (by(d), ok, ok, odd8, None, ok, ok), (by(_mk(L, 2, 64, 72, 44)), ok, ok, ok, None, ok, ok)):
        assert l.mmh_conv7_stem_sparse_fprop(*args, None) != 0
        assert b"mmh_conv7_stem_sparse_fprop" in l.mmh_last_error()
    # mmh_conv7_stem_sparse_wgrad(d, x, mask, dy, dw, ws, ws_bytes, accumulate, stream)
    need = l.mmh_conv7_stem_sparse_wgrad_ws_bytes(by(d))
    for args in ((None, ok, ok, ok, ok, ok, need), (by(d), None, ok, ok, ok, ok, need), (by(d), ok, None, ok, ok, ok, need),
                 (by(d), ok, ok, None, ok, ok, need), (by(d), ok, ok, ok, None, ok, need), (by(d), ok, ok, ok, ok, None, need),
                 (by(d), ok, ok, ok, ok, ok, need - 1), (by(d), ok, odd4, ok, ok, ok, need), (by(d), ok, ok, odd8, ok, ok, need),
                 (by(d), ok, ok, ok, odd8, ok, need), (by(d), ok, ok, ok, ok, odd8, need),
                 (by(_mk(L, 2, 64, 72, 44)), ok, ok, ok, ok, ok, need)):
        assert l.mmh_conv7_stem_sparse_wgrad(*args, 0, None) != 0
        assert b"mmh_conv7_stem_sparse_wgrad" in l.mmh_last_error()
