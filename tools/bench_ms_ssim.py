"""What the masked and multi-scale modes of the image-metrics kernel (csrc/metrics.hip) cost, at B = 32 pairs of 3 x 256 x 256
fp32 images in [-1, 1], the C entry points alone, interleaved run by run in one process, HIP events after warm-up:

  (a) mmh_image_metrics                      the plain pass
  (b) mmh_image_metrics_masked               the same pass with the hand-region means (a quarter of the pixels inside)
  (c) mmh_ms_ssim, 5 levels                  with the calls at 1 .. 4 levels beside it: the difference of two neighbours is
                                             what one more level's launch adds
  (d) the same MS-SSIM with torch device ops fp32 F.conv2d of the five moment planes with the 2-D window (grouped, no padding)
                                             and F.avg_pool2d(x, 2, padding=(H % 2, W % 2)), the mapping to [0, 1] included

Two conditions, neither a preset number:
  * (b) < 2 x (a): the masked call also returns the whole-image values, so it has to beat two plain calls;
  * (d) - (c) > spread(c) + spread(d) (spread = max - min over the runs): faster than the torch formulation by more than noise.
Both verdicts are written out, met or not.

    python tools/bench_ms_ssim.py [--runs 30] [--per_event 10] [--out profiles/ms_ssim.txt]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, CH, H, W, WINDOW = 32, 3, 256, 256, 11


def torch_ms_ssim(a, b, win, weights):
    """MS-SSIM as one writes it with torch operators (what (c) is compared with); a, b fp32 [B,C,H,W] in [-1, 1]"""
    from mmhand_amd.metrics import C1, C2
    a, b = a * 0.5 + 0.5, b * 0.5 + 0.5
    n = a.shape[1]
    vals = []
    for l in range(len(weights)):
        m = F.conv2d(torch.cat((a, b, a * a, b * b, a * b), 1), win, groups=5 * n)
        mu1, mu2, e11, e22, e12 = m.split(n, 1)
        s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
        cs = (2 * s12 + C2) / (s1 + s2 + C2)
        if l == len(weights) - 1:
            cs = cs * (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)
        vals.append(cs.double().mean(dim=(2, 3)))
        if l + 1 < len(weights):
            pad = (a.shape[2] % 2, a.shape[3] % 2)
            a, b = F.avg_pool2d(a, 2, padding=pad), F.avg_pool2d(b, 2, padding=pad)
    v = torch.stack(vals, 2).clamp(min=0)
    return torch.prod(v ** torch.tensor(weights, dtype=torch.float64, device=a.device), dim=2).mean(dim=1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=30)
    p.add_argument("--per_event", type=int, default=10)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    assert args.runs >= 20
    from mmhand_amd import lib as L
    from mmhand_amd.metrics import C1, C2, MS_WEIGHTS, _src, gaussian_taps, ms_ssim
    assert torch.cuda.is_available(), "bench_ms_ssim needs cuda:0"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    a = torch.rand((B, CH, H, W), generator=g, device=dev) * 2 - 1
    b = (a + 0.1 * torch.randn((B, CH, H, W), generator=g, device=dev)).clamp(-1, 1)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    mask = (((yy - 128) ** 2 + (xx - 128) ** 2) < 72 ** 2).to(torch.uint8)[None].repeat(B, 1, 1).contiguous()   # 0.25 of the frame
    lib = L.load()
    sa, _ = _src(a, "pm1")
    sb, _ = _src(b, "pm1")
    taps = gaussian_taps(WINDOW)
    tp = taps.ctypes.data_as(C.c_void_p)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())                                                    # noqa: E731
    keep = []

    def buffers(nbytes, *shapes):
        out = [torch.empty(nbytes, dtype=torch.uint8, device=dev)] + [torch.empty(s, dtype=torch.float64, device=dev) for s in shapes]
        keep.append(out)
        return out

    n_plain = lib.mmh_image_metrics_ws_bytes(B, CH, H, W, WINDOW)
    ws, out = buffers(n_plain, (B, 3))
    plain = ("mmh_image_metrics", (C.byref(sa), C.byref(sb), B, CH, H, W, WINDOW, tp, C1, C2, vp(ws), n_plain, vp(out), stream))
    n_mask = lib.mmh_image_metrics_masked_ws_bytes(B, CH, H, W, WINDOW)
    ws, out = buffers(n_mask, (B, 7))
    masked = ("mmh_image_metrics_masked", (C.byref(sa), C.byref(sb), vp(mask), *mask.stride(), B, CH, H, W, WINDOW, tp, C1, C2,
                                           vp(ws), n_mask, vp(out), stream))
    ms_calls = {}
    for levels in range(1, 6):
        w = np.array(MS_WEIGHTS[:levels], dtype=np.float64)
        n = lib.mmh_ms_ssim_ws_bytes(B, CH, H, W, WINDOW, levels)
        ws, scales, out = buffers(n, (B, CH, levels), (B,))
        keep.append(w)
        ms_calls[levels] = ("mmh_ms_ssim", (C.byref(sa), C.byref(sb), B, CH, H, W, WINDOW, tp, C1, C2, levels,
                                            w.ctypes.data_as(C.c_void_p), vp(ws), n, vp(scales), vp(out), stream))
    win = torch.from_numpy(np.outer(taps, taps)).to(dev)[None, None].repeat(5 * CH, 1, 1, 1).contiguous()

    def c_call(call):
        name, argv = call
        return lambda: L.check(getattr(lib, name)(*argv), name)

    cases = {"(a) mmh_image_metrics": c_call(plain), "(b) mmh_image_metrics_masked": c_call(masked)}
    for levels in range(1, 5):
        cases[f"    mmh_ms_ssim, {levels} level{'s' if levels > 1 else ''}"] = c_call(ms_calls[levels])
    cases["(c) mmh_ms_ssim, 5 levels"] = c_call(ms_calls[5])
    cases["(d) MS-SSIM with torch device ops, fp32"] = lambda: torch_ms_ssim(a, b, win, MS_WEIGHTS)

    # the two formulations score the same thing: fp32 moments without the kernel's re-centring are good to ~1e-4 here
    ref = ms_ssim(a, b)["ms_ssim"]
    alt = torch_ms_ssim(a, b, win, MS_WEIGHTS)
    agree = float((ref - alt).abs().max())
    assert agree < 1e-3, agree

    for fn in cases.values():           # warm-up: code objects, MIOpen's choice of algorithm
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(args.runs):          # interleaved: every case once per round
        for k, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()                        # keeps the stream busy while e0 and the timed calls are enqueued
            e0.record()
            for _ in range(args.per_event):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / args.per_event)

    stat = {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in times.items()}
    ka, kb, kc, kd = (k for k in cases if k[:3] in ("(a)", "(b)", "(c)", "(d)"))
    lines = [f"--- image metrics modes, B = {B}, {CH} x {H} x {W} fp32 pm1, window {WINDOW}, HIP events, {args.runs} interleaved runs of "
             f"{args.per_event} calls: median [min .. max]"]
    for k, (med, lo, hi) in stat.items():
        lines.append(f"{k:<44s}{med:9.1f} us  [{lo:9.1f} .. {hi:9.1f}]   {med / stat[ka][0]:5.2f} x (a)")
    cum = [stat[k][0] for k in cases if "mmh_ms_ssim" in k]
    lines.append("one more level adds (medians of neighbouring calls): " +
                 ", ".join(f"level {l}: {cum[l] - (cum[l - 1] if l else 0.0):.1f} us" + (" (with the finishing launch)" if l == 0 else "")
                           for l in range(5)))
    ratio = stat[kb][0] / stat[ka][0]
    lines.append(f"masked call = {ratio:.2f} x the plain call; the condition is < 2 x (it returns the whole-image values too): "
                 f"{'met' if ratio < 2 else 'NOT met'}")
    spread_c, spread_d = stat[kc][2] - stat[kc][1], stat[kd][2] - stat[kd][1]
    gain = stat[kd][0] - stat[kc][0]
    lines.append(f"mmh_ms_ssim is {gain:.1f} us faster than the torch formulation ({stat[kd][0] / stat[kc][0]:.2f} x); spreads {spread_c:.1f} us "
                 f"(c) + {spread_d:.1f} us (d) = {spread_c + spread_d:.1f} us; the condition is a gain above the combined spread: "
                 f"{'met' if gain > spread_c + spread_d else 'NOT met'}")
    lines.append(f"the two formulations agree to {agree:.1e} on these pairs (fp32 moments without re-centring in (d))")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(json.dumps({"us": {k.strip(): round(v[0], 2) for k, v in stat.items()}, "masked_over_plain": round(ratio, 3),
                      "masked_condition_met": bool(ratio < 2), "ms_gain_us": round(gain, 2),
                      "combined_spread_us": round(spread_c + spread_d, 2), "ms_condition_met": bool(gain > spread_c + spread_d)}))


if __name__ == "__main__":
    main()
