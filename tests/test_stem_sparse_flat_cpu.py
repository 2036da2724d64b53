"""Host side of the flat-order sparse stem wgrad (stem_sparse.hip, mmh_conv7_stem_sparse_wgrad_flat): its workspace is the
generic wgrad's for the same descriptor (one shared split rule, also after "wgrad_slots" moves), the shapes the query accepts,
its two switches, and the argument checks that come before any launch.  No GPU."""
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


SHAPES = ((64, 256, 256, 24), (32, 256, 256, 24), (3, 24, 48, 24), (2, 16, 16, 24), (2, 64, 64, 24), (1, 16, 256, 24),
          (3, 24, 48, 44), (2, 64, 64, 8), (1, 8, 16, 4), (2, 64, 64, 48))


def test_workspace_is_the_generic_wgrads(L):
    l = L.load()
    by = ctypes.byref
    ok, ws, gen = (l.mmh_conv7_stem_sparse_wgrad_flat_supported, l.mmh_conv7_stem_sparse_wgrad_flat_ws_bytes,
                   l.mmh_conv2d_wgrad_ws_bytes)
    old = L.get_option("wgrad_slots")
    try:
        for slots in (old, 256, 5):         # a changed knob moves both kernels together
            assert l.mmh_set_option(b"wgrad_slots", slots) == 0
            for B, H, W, C in SHAPES:
                d = _mk(L, B, H, W, C)
                assert ok(by(d)) == 1, (B, H, W, C)
                assert ws(by(d)) == gen(by(d)) > 0 and ws(by(d)) % (49 * C * 64 * 4) == 0, (slots, B, H, W, C)
    finally:
        assert l.mmh_set_option(b"wgrad_slots", old) == 0
    # the workload (D_PB, B = 64 at 256 x 256): 230 splits; the smallest GPU test shape: 13 splits of 288 pixels, the last empty
    assert ws(by(_mk(L, 64, 256, 256, 24))) == 230 * 49 * 24 * 64 * 4
    assert ws(by(_mk(L, 3, 24, 48, 24))) == 13 * 49 * 24 * 64 * 4


def test_supported_shapes_and_switches(L):
    l = L.load()
    by = ctypes.byref
    ok, ws = l.mmh_conv7_stem_sparse_wgrad_flat_supported, l.mmh_conv7_stem_sparse_wgrad_flat_ws_bytes
    no = [_mk(L, 2, 64, 64, 24, Cout=32), _mk(L, 2, 64, 64, 24, Cout=128), _mk(L, 2, 64, 64, 24, k=3, pad=1),
          _mk(L, 2, 64, 64, 24, refl=False), _mk(L, 2, 64, 64, 24, dt=L.BF16), _mk(L, 2, 64, 64, 52), _mk(L, 2, 64, 64, 22),
          _mk(L, 2, 64, 72, 24), _mk(L, 2, 60, 64, 24), _mk(L, 2, 64, 64, 24, x_cs=20), _mk(L, 2, 64, 64, 24, x_cs=26),
          _mk(L, 2, 64, 64, 24, y_cs=66), _mk(L, 512, 256, 256, 24), _mk(L, 0, 64, 64, 24)]      # 512 * 256 * 256 = 2^31 / 64
    for d in no:
        assert ok(by(d)) == 0 and ws(by(d)) == 0, (d.B, d.H, d.W, d.Cin, d.Cout, d.kh, d.x_cs, d.y_cs)
    assert ok(None) == 0 and ws(None) == 0
    assert ok(by(_mk(L, 511, 256, 256, 24))) == 1 and ok(by(_mk(L, 2, 64, 64, 24, x_cs=28, y_cs=128))) == 1
    d = _mk(L, 2, 64, 64, 24)
    for key in ("stem_sparse_flat", "stem_sparse"):
        old = L.get_option(key)
        assert old == 1
        try:
            assert l.mmh_set_option(key.encode(), 0) == 0
            assert ok(by(d)) == 0 and ws(by(d)) > 0         # the size does not depend on the switch
            if key == "stem_sparse_flat":                   # its own key: the other sparse kernels stay on
                assert l.mmh_conv7_stem_sparse_fprop_supported(by(d)) == 1 and l.mmh_conv7_stem_sparse_wgrad_supported(by(d)) == 1
        finally:
            assert l.mmh_set_option(key.encode(), old) == 0
        assert ok(by(d)) == 1
    lv = L.get_option("conv_levels")        # two-level summation is the fprop's business only
    try:
        assert l.mmh_set_option(b"conv_levels", 2) == 0
        assert ok(by(d)) == 1
    finally:
        assert l.mmh_set_option(b"conv_levels", lv) == 0


def test_null_and_misaligned_arguments_are_rejected(L):
    l = L.load()
    by = ctypes.byref
    p = ctypes.c_void_p
    d = _mk(L, 2, 64, 64, 24)
    ok, odd8, odd4 = p(4096), p(4096 + 8), p(4096 + 4)
    need = l.mmh_conv7_stem_sparse_wgrad_flat_ws_bytes(by(d))
    # mmh_conv7_stem_sparse_wgrad_flat(d, x, mask, dy, dw, ws, ws_bytes, accumulate, stream)
    for args in ((None, ok, ok, ok, ok, ok, need), (by(d), None, ok, ok, ok, ok, need), (by(d), ok, None, ok, ok, ok, need),
                 (by(d), ok, ok, None, ok, ok, need), (by(d), ok, ok, ok, None, ok, need), (by(d), ok, ok, ok, ok, None, need),
                 (by(d), ok, ok, ok, ok, ok, need - 1), (by(d), odd8, ok, ok, ok, ok, need), (by(d), ok, odd4, ok, ok, ok, need),
                 (by(d), ok, ok, odd8, ok, ok, need), (by(d), ok, ok, ok, odd8, ok, need), (by(d), ok, ok, ok, ok, odd8, need),
                 (by(_mk(L, 2, 64, 72, 24)), ok, ok, ok, ok, ok, need)):
        assert l.mmh_conv7_stem_sparse_wgrad_flat(*args, 0, None) != 0
        assert b"mmh_conv7_stem_sparse_wgrad_flat" in l.mmh_last_error()
