"""Writes tests/golden/hpe.npz and tests/golden/hpe_keys.json from the reference's own hand-pose estimator code (imported
unmodified from a reference checkout; nothing of it is copied - only name lists and recorded outputs are stored):

* hpe_keys.json: the state-dict keys and shapes of Hpm2d(21, 3, False) and Hpm3d(21, 21);
* hpe.npz, on tests/_hpe_oracle.py's generated weights (full width, seed SEED) and images (B = 2, 32 x 32), in float64:
  - heat, up, xy: the reference Hpm2d's last-stage heat maps (the output of its stage6), its last output (their x8 upsample)
    and the pixel hpe_estimator.py:131-133 takes from each map (y = index // H, x = index % W);
  - depth: the reference Hpm3d on `up`, its depth_fc_1 replaced on the instance by a Linear of 21*4*4 inputs (a 32 x 32 input
    leaves 4 x 4 maps), everything else its own;
  - ev_gt, ev_pred, ev_30_20, ev_10_7: a table of points fed to EvalUtil and its get_measures(0, 30, 20) / (0, 10, 7),
    flattened as [epe_mean, epe_median, auc, *curve].

    python tests/golden/make_hpe.py <reference checkout>"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SEED = 0


def main(ref):
    base = os.path.join(ref, "baselines", "quantitative_on_benchmarks")
    sys.path.insert(0, base)
    # the package's __init__ imports training-only dependencies; its two network modules need none of them
    pkg = types.ModuleType("networks")
    pkg.__path__ = [os.path.join(base, "networks")]
    sys.modules["networks"] = pkg
    if not hasattr(np, "trapz"):
        np.trapz = np.trapezoid
    from hpe_estimator import EvalUtil
    from networks.net_hpm2d import Hpm2d
    from networks.net_hpm3d import Hpm3d
    from tests import _hpe_oracle as O

    net2, net3 = Hpm2d(21, 3, False).double().eval(), Hpm3d(21, 21).double().eval()
    with open(os.path.join(ROOT, "tests", "golden", "hpe_keys.json"), "w") as fh:
        json.dump({"hpm2d": O.keys_and_shapes(net2.state_dict()), "hpm3d": O.keys_and_shapes(net3.state_dict())}, fh)

    x = torch.from_numpy(O.normalize(O.images(2, 32, 32, SEED))[..., :3]).permute(0, 3, 1, 2).double()
    net2.load_state_dict(O.state_dict("2d", O.FULL, seed=SEED))
    kept = {}
    net2.stage6.register_forward_hook(lambda m, i, o: kept.__setitem__("heat", o.detach().clone()))
    with torch.no_grad():
        up = net2(x)[-1]
    KP, H, W = 21, up.shape[2], up.shape[3]
    xy = np.zeros((2, KP, 2), dtype=np.int64)
    for b in range(2):
        for j, heatmap in enumerate(up[b].reshape(KP, -1)):
            index = int(torch.max(heatmap, 0)[-1])
            xy[b, j] = [index % W, index // H]

    net3.depth_fc_1 = torch.nn.Linear(21 * 4 * 4, 512).double()
    net3.load_state_dict(O.state_dict("3d", O.FULL, head_hw=4, seed=SEED))
    # the CPU's conv may return a strided tensor, which the reference's .view refuses: same values, made contiguous
    net3.depth.register_forward_hook(lambda m, i, o: o.contiguous())
    with torch.no_grad():
        depth = net3(up)

    ev = {}
    gt = O.hashed(7001, 6 * 21 * 2, SEED).reshape(6, 21, 2) * 16 + 16
    pred = np.floor(O.hashed(7002, 6 * 21 * 2, SEED).reshape(6, 21, 2) * 16 + 16)
    for max_px, steps in ((30, 20), (10, 7)):
        e = EvalUtil(21)
        for g, p in zip(gt, pred):
            e.feed(g, np.ones(21), p)
        mean, median, auc, curve, _ = e.get_measures(0, max_px, steps)
        ev[f"ev_{max_px}_{steps}"] = np.concatenate([[mean, median, auc], curve])
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "hpe.npz"), heat=kept["heat"].numpy(), up=up.numpy(), xy=xy,
                        depth=depth.numpy(), ev_gt=gt, ev_pred=pred, **ev)
    print("heat", tuple(kept["heat"].shape), "up", tuple(up.shape), "depth", tuple(depth.shape))


if __name__ == "__main__":
    main(sys.argv[1])
