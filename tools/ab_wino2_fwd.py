"""The F(2x2,3x3) two-level forward of ops.set_winograd_mode("bwd_f2") against the direct two-level fprop of mode "bwd", per
stack shape, in one process.

    python tools/ab_wino2_fwd.py                 # speed: interleaved A/B at B=32, medians over alternating repeats
    python tools/ab_wino2_fwd.py --accuracy      # relative L1 against float64 (oracle/ops_ref.py) over --seeds seeds, B=2

Speed: both variants are warmed up, then the variants alternate --rounds times; each visit times --iters back-to-back calls
between two HIP events.  The spread column is (max - min) / median of a variant's visits: a shape belongs to the new path
only where it wins by more than that.  Accuracy: the ratio err(F(2x2) two-level) / err(direct two-level) on the same
tensors, and the one-level 16-plane GEMM beside it (a ratio near 3 would mean the fold is not engaged)."""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
ap = argparse.ArgumentParser()
ap.add_argument("--accuracy", action="store_true"); ap.add_argument("--seeds", type=int, default=5)
ap.add_argument("--batch", type=int, default=32); ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--iters", type=int, default=5)
a = ap.parse_args()
from mmhand_amd import lib as L, ops
dev = torch.device("cuda:0")
SHAPES = [(512, 512, 64), (512, 256, 64), (256, 256, 64), (128, 128, 128), (64, 64, 256)]    # Cin, Cout, H = W


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g) * 2 - 1) * scale)


def f2(x, w, bias, reflect, act, levels):
    return ops._wino_conv(x, ops.wino_weights(w, 2), bias, w.shape[3], reflect, act, 2, levels16=levels)


ops.set_winograd_mode("bwd")            # direct fprop with two-level summation; the F(2x2) path is called explicitly
try:
    if a.accuracy:
        from oracle import ops_ref as R
        print("relative L1 against float64, B=2: direct two-level | F(2x2) two-level (ratio) | F(2x2) one-level (ratio)")
        worst = 0.0
        for cin, cout, hw in SHAPES[:4]:
            for reflect, with_bias in ((True, False), (False, True)):
                for seed in range(a.seeds):
                    x, w = rand((2, hw, hw, cin), 100 + seed), rand((3, 3, cin, cout), 200 + seed, 0.05)
                    bias = rand((cout,), 300 + seed, 0.1) if with_bias else None
                    act = 1 if with_bias else 0
                    ref = R.conv2d(x, w, bias, 1, 1, reflect, act)
                    xd, wd, bd = x.to(dev), w.to(dev), None if bias is None else bias.to(dev)
                    ops.bump_weights_epoch()
                    e = [R.rel_l1(y.double().cpu(), ref) for y in (ops.raw_conv_fprop(xd, wd, bd, 1, 1, reflect, act),
                                                                   f2(xd, wd, bd, reflect, act, 2), f2(xd, wd, bd, reflect, act, 1))]
                    worst = max(worst, e[1] / e[0])
                    print(f"{cin:4d}->{cout:<4d} {hw:3d}x{hw:<3d} {'reflect' if reflect else 'zero   '} {'bias+relu' if with_bias else 'plain    '} "
                          f"seed {seed}: {e[0]:.3e} | {e[1]:.3e} ({e[1] / e[0]:.3f}) | {e[2]:.3e} ({e[2] / e[0]:.3f})", flush=True)
        print(f"worst ratio two-level F(2x2) / direct two-level: {worst:.3f}")
    else:
        print(f"fprop, B={a.batch}, reflect pad, bias + ReLU; us per call: direct two-level | F(2x2) two-level (input / GEMM / output)")
        for cin, cout, hw in SHAPES:
            x, w, bias = rand((a.batch, hw, hw, cin), 1).to(dev), rand((3, 3, cin, cout), 2, 0.05).to(dev), rand((cout,), 3, 0.1).to(dev)
            fns = {"direct": lambda: ops.raw_conv_fprop(x, w, bias, 1, 1, True, 1), "wino2": lambda: f2(x, w, bias, True, 1, 2)}
            for f in fns.values():
                for _ in range(3): f()
            torch.cuda.synchronize()
            res = {k: [] for k in fns}
            for r in range(a.rounds):
                for k, f in fns.items():
                    f()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters): f()
                    e1.record(); torch.cuda.synchronize()
                    res[k].append(e0.elapsed_time(e1) / a.iters * 1e3)
            # the three launches of the new path on their own (same buffers, not interleaved: a breakdown, not the verdict)
            tiles = a.batch * (hw // 2) ** 2
            V = torch.empty((16, tiles, cin), device=dev); M = torch.empty((16, tiles, cout), device=dev); y = torch.empty((a.batch, hw, hw, cout), device=dev)
            U = ops.wino_weights(w, 2); P = ops._ptr; st = ops._stream
            parts = [lambda: L.call("mmh_wino_input", P(x), a.batch, hw, hw, cin, 1, 2, L.F32, P(V), st()),
                     lambda: L.call("mmh_wino_gemm_levels16", P(V), P(U), P(M), tiles, cin, cout, 2, st()),
                     lambda: L.call("mmh_wino_output", P(M), P(y), P(bias), a.batch, hw, hw, cout, 1, 2, L.F32, P(None), 0, st())]
            pt = []
            for f in parts:
                f(); e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters): f()
                e1.record(); torch.cuda.synchronize()
                pt.append(e0.elapsed_time(e1) / a.iters * 1e3)
            del V, M, y
            md = {k: statistics.median(v) for k, v in res.items()}
            sp = {k: (max(v) - min(v)) / md[k] for k, v in res.items()}
            gf = 2.0 * 16 * tiles * cin * cout / (pt[1] * 1e-6) / 1e12
            print(f"{cin:4d}->{cout:<4d} {hw:3d}x{hw:<3d}: {md['direct']:8.1f} (spread {sp['direct'] * 100:.1f} %) | {md['wino2']:8.1f} (spread {sp['wino2'] * 100:.1f} %)"
                  f"  speed-up {md['direct'] / md['wino2']:.2f}x   [{pt[0]:.0f} / {pt[1]:.0f} ({gf:.0f} TFLOP/s) / {pt[2]:.0f}]", flush=True)
finally:
    ops.set_winograd_mode("all")
