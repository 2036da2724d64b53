"""Writes tests/golden/inception.npz and tests/golden/inception_keys.json from the reference's own Inception-v3 and score code
(imported unmodified from a reference checkout; nothing of it is copied - only name lists and recorded outputs are stored):

* inception_keys.json: the state-dict keys and shapes of the reference's Inception3() (with its aux head, as the pretrained
  file has them);
* inception.npz, on tests/_inception_oracle.py's generated weights (seed SEED), in float64:
  - logits_a, logits_b: the reference module (eval, transform_input=False) on net_inputs([2,3,75,75]) and
    net_inputs([1,3,107,91], index=1) - the second ends on a 2 x 1 grid with 5 x 4 in Mixed_6;
  - is_logits: a table of logits; is_ref: the reference's inception_score(rows, identity model, splits=1)[0] on its fp32 rows
    (its softmax is fp32); is_f64: the same formula with a float64 softmax.

    python tests/golden/make_inception.py <reference checkout>"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SEED = 0


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def main(ref):
    base = os.path.join(ref, "baselines", "quantitative_on_benchmarks")
    sys.path.insert(0, base)
    # inception.py wants torchvision only for the download helper; utils.py imports the other metrics' modules at its top
    tv = sys.modules.get("torchvision") or _stub("torchvision")
    tv.models = _stub("torchvision.models")
    tv.models.utils = _stub("torchvision.models.utils", load_state_dict_from_url=None)
    from inception import Inception3
    tv.transforms = _stub("torchvision.transforms")
    for name in ("cv2", "pytorch_ssim", "hpe_estimator"):
        if name not in sys.modules:
            _stub(name, ssim=None, HPEstimator=None)
    from utils import inception_score
    from scipy.stats import entropy
    from tests import _inception_oracle as O

    with open(os.path.join(ROOT, "tests", "golden", "inception_keys.json"), "w") as fh:
        json.dump({"inception_v3": O.keys_and_shapes(Inception3(init_weights=False).state_dict())}, fh)

    net = Inception3(aux_logits=True, transform_input=False, init_weights=False).double().eval()
    net.load_state_dict(O.state_dict(SEED, aux=True))
    out = {}
    with torch.no_grad():
        out["logits_a"] = net(torch.from_numpy(O.net_inputs((2, 3, 75, 75), SEED))).numpy()
        out["logits_b"] = net(torch.from_numpy(O.net_inputs((1, 3, 107, 91), SEED, index=1))).numpy()

    from tests._hpe_oracle import hashed
    table = hashed(9300, 70 * 1000, SEED).reshape(70, 1000) * 6.0
    rows = [torch.from_numpy(r.astype(np.float32)) for r in table]
    out["is_logits"] = table.astype(np.float32)
    out["is_ref"] = np.float64(inception_score(rows, torch.nn.Identity(), splits=1)[0])
    z = out["is_logits"].astype(np.float64)
    p = np.exp(z - z.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    py = np.mean(p, axis=0)
    out["is_f64"] = np.float64(np.exp(np.mean([entropy(p[i], py) for i in range(len(p))])))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "inception.npz"), **out)
    print({k: (v.shape if hasattr(v, "shape") and v.shape else float(v)) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
