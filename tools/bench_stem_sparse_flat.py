"""D_PB's fp32 7x7 stem wgrad (24 -> 64 at 2 B, 256 x 256; 3 dense image lanes + 21 pose lanes, joints in a 90-pixel cluster as
tools/bench_stem_sparse.py builds them): mmh_conv7_stem_sparse_wgrad_flat against the generic mmh_conv2d_wgrad it reproduces,
interleaved, HIP events around single launches (kernel + slab sum), ROUNDS rounds; with the image lanes at 0-2 and at 21-23,
and on a fully dense input.  Prints min / median / max per route, the spread of the generic kernel's own repeats, and whether
dw is bit-identical."""
import ctypes, os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mmhand_amd import ops, lib as L
dev = torch.device("cuda:0"); B0 = int(os.environ.get("B", 32)); H = int(os.environ.get("H", 256)); ROUNDS = int(os.environ.get("ROUNDS", 15))
def pose(Bn, n, g):
    centre = torch.rand((Bn, 1, 2), generator=g, dtype=torch.float64) * (H - 80) + 40
    uv = centre + (torch.rand((Bn, n, 2), generator=g, dtype=torch.float64) - 0.5) * 90
    return ops.pose_heatmaps(uv.reshape(-1, 2).contiguous().to(dev), H, H).reshape(Bn, n, H, H).permute(0, 2, 3, 1)
def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3
g = torch.Generator().manual_seed(3)
Bn, Cin = 2 * B0, 24
d = ops.conv_desc(Bn, H, H, Cin, 64, 7, 1, 3, True)
assert L.load().mmh_conv7_stem_sparse_wgrad_flat_supported(ctypes.byref(d)) == 1
nb = L.load().mmh_conv7_stem_sparse_wgrad_flat_ws_bytes(ctypes.byref(d))
assert nb == L.load().mmh_conv2d_wgrad_ws_bytes(ctypes.byref(d))
ws = torch.empty((nb // 4,), device=dev); dy = torch.randn(Bn, H, H, 64, device=dev)
maps, img = pose(Bn, 21, g), torch.randn(Bn, H, H, 3, device=dev)
for name in ("image lanes 0-2", "image lanes 21-23", "all lanes dense"):
    x = torch.zeros(Bn, H, H, Cin, device=dev)
    if name == "image lanes 0-2": x[..., :3] = img; x[..., 3:] = maps
    elif name == "image lanes 21-23": x[..., 21:] = img; x[..., :21] = maps
    else: x.normal_()
    mask = torch.empty((L.load().mmh_stem_activity_bytes(Bn, H, H) // 8,), dtype=torch.int64, device=dev)
    L.call("mmh_stem_activity", ops._ptr(x), Bn, H, H, Cin, ops._ptr(mask), ops._stream())
    dw = [torch.empty(7, 7, Cin, 64, device=dev) for _ in range(2)]
    gen = lambda: L.call("mmh_conv2d_wgrad", ctypes.byref(d), ops._ptr(x), ops._ptr(dy), ops._ptr(dw[0]), ops._ptr(ws), nb, 0, 0, ops._stream())
    flat = lambda: L.call("mmh_conv7_stem_sparse_wgrad_flat", ctypes.byref(d), ops._ptr(x), ops._ptr(mask), ops._ptr(dy), ops._ptr(dw[1]),
                          ops._ptr(ws), nb, 0, ops._stream())
    gen(); flat(); torch.cuda.synchronize()
    same = torch.equal(dw[0], dw[1])
    t = {"generic": [], "flat": []}
    for _ in range(ROUNDS):
        t["generic"].append(timed(gen)); t["flat"].append(timed(flat))
    s = {k: (min(v), statistics.median(v), max(v)) for k, v in t.items()}
    print(f"D_PB stem wgrad B{Bn} {Cin}->64 @{H}, {name}: generic min/med/max {s['generic'][0]:.0f}/{s['generic'][1]:.0f}/{s['generic'][2]:.0f} us "
          f"(spread {s['generic'][2] - s['generic'][0]:.0f}) | flat {s['flat'][0]:.0f}/{s['flat'][1]:.0f}/{s['flat'][2]:.0f} us | "
          f"bit-identical: {same}", flush=True)
