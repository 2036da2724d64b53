"""Writes tests/golden/hpe3d_train.npz from the reference's own 3D estimator (networks/net_hpm3d.py imported unmodified from a
reference checkout; nothing of it is copied - only recorded numbers are stored), in float64:

* the instance's layers are replaced by nn.Conv2d / nn.Linear modules of tests/_hpe_oracle.NARROW's widths, depth_fc_1 for
  4 x 4 maps (the class hard-codes the full widths and 32 x 32 maps; its forward - the trunk, the cat((heat, out_0), 1) of every
  stage, `depth`, the three Linear layers, stage6 left out - is its own) and loaded with the generated NARROW weights of seed
  SEED; the input and the depth targets are tests/_hpe3d_train_oracle.inputs(): B = 2, the sigma-5 Gaussian maps at 32 x 32;
* out: the 42 outputs; loss: torch.nn.SmoothL1Loss()(out, z) * 10 (hpm3d_model.py:73,105); grad_<key>: its gradient for every
  parameter that has one, with the low 12 bits of each float64 cleared (a relative 2^-41 = 4.5e-13 at most) so that the file
  stays under 1 MB compressed; no_grad: the keys whose gradient is None (stage6.*).

    python tests/golden/make_hpe3d_train.py <reference checkout>"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SEED = 0


def clear_low_bits(a, bits=12):
    v = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    return (v & ~np.uint64((1 << bits) - 1)).view(np.float64)


def main(ref):
    base = os.path.join(ref, "baselines", "quantitative_on_benchmarks")
    sys.path.insert(0, base)
    pkg = types.ModuleType("networks")          # the package's __init__ imports training-only dependencies
    pkg.__path__ = [os.path.join(base, "networks")]
    sys.modules["networks"] = pkg
    from networks.net_hpm3d import Hpm3d
    from tests import _hpe_oracle as O
    from tests import _hpe3d_train_oracle as T3

    sd = O.state_dict("3d", O.NARROW, head_hw=4, seed=SEED)
    net = Hpm3d(21, 21).double()
    for key, w in sd.items():
        if key.endswith(".weight"):
            mod, _, leaf = key[:-len(".weight")].rpartition(".")
            new = (torch.nn.Linear(w.shape[1], w.shape[0]) if w.dim() == 2 else
                   torch.nn.Conv2d(w.shape[1], w.shape[0], kernel_size=w.shape[2], padding=w.shape[2] // 2))
            setattr(net.get_submodule(mod) if mod else net, leaf, new.double())
    net.load_state_dict(sd, strict=True)

    heat, z = T3.inputs(SEED)
    out = net(T3.nchw(heat).double())
    loss = torch.nn.SmoothL1Loss()(out, torch.from_numpy(z)) * 10
    loss.backward()
    rec = {"out": out.detach().numpy(), "loss": np.array(float(loss.detach())),
           "no_grad": np.array([k for k, p in net.named_parameters() if p.grad is None])}
    for key, p in net.named_parameters():
        if p.grad is not None:
            rec["grad_" + key] = clear_low_bits(p.grad.numpy())
    path = os.path.join(ROOT, "tests", "golden", "hpe3d_train.npz")
    np.savez_compressed(path, **rec)
    d = np.abs(out.detach().numpy() - z)
    print("loss", rec["loss"], "outputs in +-%.3f" % np.abs(rec["out"]).max(), "terms on the linear branch:", int((d >= 1.0).sum()),
          "gradient elements", sum(v.size for k, v in rec.items() if k.startswith("grad_")), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1])
