"""Times the input decode pass with the resize inside it (mmh_decode_inputs_resized, csrc/pointwise.hip) next to the plain
pass (mmh_decode_inputs), the C entry points alone, with HIP events after warm-up: `per_event` launches back to back between
one event pair (one launch enqueued ahead, so the stream is busy when the first event fires and host enqueue time is not
counted), the median over `runs` pairs, per launch, in us; GB/s = bytes written (240 per output pixel) + source bytes read
once, over that time.  Three cases:

    256 x 256 -> 512 x 512 at B = 4       (the size512_bf16_b4 configuration fed from files)
    256 x 256 -> 128 x 128 at B = 32      (a quick small-size run on real data)
    256 x 256 -> 256 x 256 at B = 32      through the OLD entry point: the yardstick (the identity size never reaches the new one)

Prints one JSON line.

    python tools/bench_decode_resize.py [--runs 30] [--per_event 10]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("256_to_512_b4", 4, 256, 512), ("256_to_128_b32", 32, 256, 128), ("256_plain_b32", 32, 256, 256)]


def bench_case(B, src, dst, runs, per_event):
    from mmhand_amd import lib as L
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    raw = [torch.randint(0, 256, (B, src, src, 3), generator=g, device=dev, dtype=torch.uint8) for _ in range(4)]
    uv = [torch.rand((B, 21, 2), generator=g, device=dev, dtype=torch.float64) * (dst - 40) + 20 for _ in range(2)]
    outs = [torch.empty((B, dst, dst, c), dtype=torch.float32, device=dev) for c in (4, 4, 44, 8)]
    lib = L.load()
    p = lambda t: C.c_void_p(t.data_ptr())                        # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if src == dst:
        name = "mmh_decode_inputs"
        args = [p(t) for t in raw + uv] + [B, src, src, 6.0] + [p(t) for t in outs] + [stream]
    else:
        name = "mmh_decode_inputs_resized"
        args = [p(t) for t in raw + uv] + [B, src, src, dst, dst, 6.0] + [p(t) for t in outs] + [stream]
    fn = getattr(lib, name)

    def launch():
        L.check(fn(*args), name)

    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        launch()                                   # keeps the stream busy while e0 and the timed launches are enqueued
        e0.record()
        for _ in range(per_event):
            launch()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / per_event)
    med = float(np.median(times))
    nbytes = B * dst * dst * 240 + 4 * B * src * src * 3
    return {"entry_point": name, "B": B, "src": src, "dst": dst, "median_us": round(med, 2),
            "min_us": round(float(np.min(times)), 2), "max_us": round(float(np.max(times)), 2),
            "GBps": round(nbytes / med / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--per_event", type=int, default=10)
    a = ap.parse_args()
    assert a.runs >= 20
    torch.cuda.set_device(0)
    res = {"runs": a.runs, "launches_per_event_pair": a.per_event}
    for tag, B, src, dst in CASES:
        res[tag] = bench_case(B, src, dst, a.runs, a.per_event)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
