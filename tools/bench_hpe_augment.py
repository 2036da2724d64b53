"""Measures the estimators' augmenting normalisation (csrc/hpe_augment.hip, train_hpe --augment_geom / --augment_color) on one
MI355X and writes profiles/hpe_augment.txt:

* mmh_hpe_normalize on a uint8 BGR batch (what train_hpe launches without the flags) against mmh_hpe_augment_normalize with
  identity arguments, with default-range geometry, and with geometry + colour matrix + gamma - interleaved round by round, at
  B = 32, 256 x 256;
* one Hpm2dTrainer step without the flags (step) and with both (hpe_augment_normalize -> step_normalized), the host's matrix
  maths and the three small uploads included, interleaved as well.

The bytes each form moves are computed from the shapes: both passes of either kernel read the source (3 bytes per source pixel
each, neighbouring taps sharing cache lines) and the second writes 16 bytes per output pixel; keeping the three float64 values in
the workspace between the passes instead of recomputing them would add a 24-byte write and a 24-byte read per output pixel.

The weights are generated (tests/_hpe_oracle.py): the rates do not depend on them.  These are recorded measurements; nothing here
is a bar, and nothing about training quality was measured.

    python tools/bench_hpe_augment.py [--batch 32] [--size 256] [--rounds 7] [--inner 20] [--out profiles/hpe_augment.txt]"""
import argparse
import json
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, inner):
    """ms per call: `inner` calls between one pair of device events (a single call is a few tens of microseconds)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--inner", type=int, default=20)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpe_augment.txt"))
    a = p.parse_args()
    from mmhand_amd import data, hpe_train, ops, train_hpe
    from tests import _hpe_oracle as O
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    B, S = a.batch, a.size
    g = torch.Generator(device=dev).manual_seed(0)
    img = torch.randint(0, 256, (B, S, S, 3), generator=g, device=dev, dtype=torch.uint8)
    uv = np.random.RandomState(0).uniform(0, S - 1, (B, 21, 2))

    # default-range draws for B items, as the driver makes them
    opt = types.SimpleNamespace(augment_geom=True, augment_color=True, dataroot="-", aug_seed=0)
    aug = train_hpe.Augment(opt, B)
    aug.set_epoch(1)
    ids = list(range(B))
    fwd = aug.forward_maps(ids, (S, S))
    xf = torch.from_numpy(data.affine_inverse(fwd, (S, S)).reshape(B, 6)).to(dev)
    c = aug.color
    cm = torch.from_numpy(data.color_matrix(c[:, 0], c[:, 1], c[:, 2:5]).reshape(B, 9)).to(dev)
    gamma = torch.from_numpy(np.ascontiguousarray(c[:, 5])).to(dev)
    eye_xf = torch.tensor([1.0, 0, 0, 0, 1, 0], dtype=torch.float64, device=dev).repeat(B, 1)

    forms = OrderedDict([
        ("hpe_normalize", lambda: ops.hpe_normalize(img, "bgr_hwc")),
        ("augment_null", lambda: ops.hpe_augment_normalize(img)),
        ("augment_identity", lambda: ops.hpe_augment_normalize(img, eye_xf, None, None)),
        ("augment_geom", lambda: ops.hpe_augment_normalize(img, xf)),
        ("augment_geom_color_gamma", lambda: ops.hpe_augment_normalize(img, xf, cm, gamma)),
    ])
    # one check before anything is timed: the identity forms are the plain pass, bit for bit
    want = forms["hpe_normalize"]()
    assert torch.equal(forms["augment_null"](), want) and torch.equal(forms["augment_identity"](), want)
    for fn in forms.values():
        timed(fn, 3)
    ms = {k: [] for k in forms}
    for _ in range(a.rounds):                       # interleaved: every form once per round
        for k, fn in forms.items():
            ms[k].append(timed(fn, a.inner))

    tr = hpe_train.Hpm2dTrainer(dev).load_state_dict(OrderedDict((k, v.float()) for k, v in O.state_dict("2d", O.FULL).items()))

    def plain_step():
        return tr.step(img, uv, layout="bgr_hwc", lr=0.0)

    def augmented_step():
        return tr.step_normalized(aug.normalize(img, ids), aug.joints(uv, ids, (S, S)), lr=0.0)

    steps = OrderedDict([("step_plain", plain_step), ("step_augmented", augmented_step)])
    for fn in steps.values():
        timed(fn, 1)
    sms = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            sms[k].append(timed(fn, 1))

    med = lambda v: float(np.median(v))            # noqa: E731
    src, out = B * S * S * 3, B * S * S * 16
    res = {"batch": B, "size": S, "rounds": a.rounds, "inner": a.inner,
           "ms": {k: round(med(v), 4) for k, v in ms.items()},
           "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
           "over_hpe_normalize": {k: round(med(v) / med(ms["hpe_normalize"]), 3) for k, v in ms.items()},
           "bytes": {"source_per_pass": src, "passes_over_source": 2, "output_write": out, "two_pass_total": 2 * src + out,
                     "one_pass_with_values_in_ws_total": src + 2 * B * S * S * 24 + out},
           "two_pass_GBps": {k: round((2 * src + out) / med(v) / 1e6, 1) for k, v in ms.items()},
           "step_ms": {k: round(med(v), 2) for k, v in sms.items()},
           "step_ms_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in sms.items()},
           "step_img_s": {k: round(B / med(v) * 1e3, 1) for k, v in sms.items()},
           "training_quality": "not measured", "weights": "generated (tests/_hpe_oracle.py)",
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("# tools/bench_hpe_augment.py: the estimators' input pass without and with augmentation, and one 2D training step\n"
                 "# without and with --augment_geom --augment_color (generated weights; lr 0).  ms = medians over the rounds of HIP-event\n"
                 "# pairs, host enqueue included (`inner` calls per pair for the passes, one step per pair for the steps); the forms are\n"
                 "# interleaved round by round.  bytes = what each form moves, from the shapes (both kernels read the source twice).\n"
                 "# Recorded measurements, not bars; nothing about training quality was measured.\n"
                 + line + "\n")


if __name__ == "__main__":
    main()
