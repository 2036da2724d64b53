"""Writes tests/golden/hpe_train.npz from the reference's own 2D estimator (networks/net_hpm2d.py imported unmodified from a
reference checkout; nothing of it is copied - only recorded numbers are stored), in float64:

* the instance's convolutions are replaced by nn.Conv2d modules of tests/_hpe_oracle.NARROW's widths (the class hard-codes the
  full widths; its forward - the trunk, the cat((heat, out_0), 1) of every stage, the six x8 upsampled outputs - is its own) and
  loaded with the generated NARROW weights of seed SEED; the input is the normalised generated images, B = 2, 32 x 32;
* target: fp32 [2,21,32,32], the target of tests/_hpe_train_oracle.target for tests/_hpe_train_oracle.poses at sigma 5 (the
  reference's data/RHD_dataset.py needs OpenCV to import, which is not installed where this was written: the formula is pinned
  by citation - RHD_dataset.py:245-277 - and not by running that module);
* loss: nn.MSELoss() of each of the six outputs against it; grad_<key>: the gradient of their sum for every parameter, with
  the low 12 bits of each float64 cleared (a relative 2^-41 = 4.5e-13 at most) so that the file stays under 1 MB compressed.

    python tests/golden/make_hpe_train.py <reference checkout>"""
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
    from networks.net_hpm2d import Hpm2d
    from tests import _hpe_oracle as O
    from tests import _hpe_train_oracle as T

    sd = O.state_dict("2d", O.NARROW, seed=SEED)
    net = Hpm2d(21, 3, True).double()
    for key, w in sd.items():
        if key.endswith(".weight"):
            mod, _, leaf = key[:-len(".weight")].rpartition(".")
            k = w.shape[2]
            setattr(net.get_submodule(mod) if mod else net, leaf,
                    torch.nn.Conv2d(w.shape[1], w.shape[0], kernel_size=k, padding=k // 2).double())
    net.load_state_dict(sd, strict=True)

    x = torch.from_numpy(O.normalize(O.images(2, 32, 32, SEED))[..., :3]).permute(0, 3, 1, 2).double()
    tgt = torch.from_numpy(T.target(T.poses(2, 32, 32, SEED), 32, 32, 5.0)).permute(0, 3, 1, 2).contiguous()
    crit = torch.nn.MSELoss()
    ls = [crit(o, tgt.double()) for o in net(x)]
    sum(ls).backward()
    out = {"target": tgt.numpy(), "loss": np.array([float(l.detach()) for l in ls])}
    for key, p in net.named_parameters():
        out["grad_" + key] = clear_low_bits(p.grad.numpy())
    path = os.path.join(ROOT, "tests", "golden", "hpe_train.npz")
    np.savez_compressed(path, **out)
    print("losses", out["loss"], "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1])
