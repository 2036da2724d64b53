"""fp32 7x7 pose stems @256x256: the compacted-channel kernels (stem_sparse.hip) against the dense ones, on pose maps as the
loader makes them (21 joints per hand, truncated Gaussians): G pose stem 44 -> 64 at B, D_PB 24 -> 64 at 2 B (3 dense image
lanes + 21 pose lanes).  Per shape: the mask pass, fprop and wgrad of both routes (median of 5 rounds of 6 launches), the mean
number of active channels per 16 x 16 tile, and whether the forward is bit-identical.  The wgrad goes through
ops.raw_conv_wgrad: at 24 lanes both routes are the dense kernel (the sparse wgrad is wired for the 44-lane stem only)."""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mmhand_amd import ops, lib
dev = torch.device("cuda:0"); B0 = int(os.environ.get("B", 32)); H = int(os.environ.get("H", 256))
def timeit(fn, iters=6):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters
def pose(Bn, n, g):
    """n maps per image: joints of a hand-sized cluster somewhere in the frame"""
    centre = torch.rand((Bn, 1, 2), generator=g, dtype=torch.float64) * (H - 80) + 40
    uv = centre + (torch.rand((Bn, n, 2), generator=g, dtype=torch.float64) - 0.5) * 90
    return ops.pose_heatmaps(uv.reshape(-1, 2).contiguous().to(dev), H, H).reshape(Bn, n, H, H).permute(0, 2, 3, 1)
g = torch.Generator().manual_seed(3)
for name, Bn, Cin in (("G pose stem", B0, 44), ("D_PB stem", 2 * B0, 24)):
    x = torch.zeros(Bn, H, H, Cin, device=dev)
    if Cin == 44:
        x[..., :21] = pose(Bn, 21, g); x[..., 21:42] = pose(Bn, 21, g)
    else:
        x[..., :3] = torch.randn(Bn, H, H, 3, device=dev); x[..., 3:24] = pose(Bn, 21, g)
    w = torch.randn(7, 7, Cin, 64, device=dev) * 0.05
    bias = torch.randn(64, device=dev)
    dy = torch.randn(Bn, H, H, 64, device=dev)
    def fprop():
        y = ops.raw_conv_fprop(x, w, bias, 1, 3, True, 0, want_stats=True)
        st = ops._take_stats(y)[0]
        return y, st
    wgrad = lambda: ops.raw_conv_wgrad(x, dy, 7, 1, 3, True)
    def mask_pass():
        ops._stem_masks.clear(); return ops.stem_mask_request(x)
    def route(on):
        ops._stem_masks.clear()
        if on: ops.stem_mask_request(x)
    outs = {}
    for on in (0, 1):
        route(on); y, st = fprop(); outs[on] = (y.clone(), st.clone(), wgrad().clone()); torch.cuda.synchronize()
    same = torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    relw = float((outs[1][2].double() - outs[0][2].double()).abs().sum() / outs[0][2].double().abs().sum())
    m = mask_pass().view(Bn, H // 8, H // 16)
    tile = m[:, 0::2] | m[:, 1::2]
    nact = sum(((tile >> c) & 1) for c in range(Cin)).float()
    res = {k: [] for k in ("mask", "f0", "f1", "w0", "w1")}
    for _ in range(5):
        res["mask"].append(timeit(mask_pass))
        for on in (0, 1):
            route(on); res[f"f{on}"].append(timeit(fprop)); res[f"w{on}"].append(timeit(wgrad))
    t = {k: statistics.median(v) * 1e3 for k, v in res.items()}
    print(f"{name} B{Bn} {Cin}->64 @{H}: active channels per tile mean {float(nact.mean()):.2f} max {int(nact.max())} | mask {t['mask']:.0f} us | "
          f"fprop dense {t['f0']:.0f} us sparse {t['f1']:.0f} us (bit-identical: {same}) | wgrad dense {t['w0']:.0f} us sparse {t['w1']:.0f} us "
          f"(rel diff {relw:.1e})", flush=True)
ops._stem_masks.clear(); ops._pending_stats.clear()
