"""Writes tests/golden/ssim.npz from the reference's own SSIM (pytorch_ssim, imported unmodified from a reference
checkout; nothing of it is copied): per case of tests/ssim_cases.py, ssim(a01, b01, window_size=w, size_average=False)
on the images mapped to [0, 1] ((x + 1) / 2), in float64 ("f64") and in float32 ("f32", the reference's own fp32 error).

    python tests/golden/make_ssim_golden.py <reference checkout>"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(ref):
    sys.path.insert(0, os.path.join(ref, "baselines", "quantitative_on_benchmarks"))
    import pytorch_ssim
    from tests.ssim_cases import cases
    names, f64, f32 = [], [], []
    for name, a, b, w in cases():
        a01 = (torch.from_numpy(a).double() + 1) / 2
        b01 = (torch.from_numpy(b).double() + 1) / 2
        names.append(name)
        f64.append(pytorch_ssim.ssim(a01, b01, window_size=w, size_average=False).numpy())
        f32.append(pytorch_ssim.ssim(a01.float(), b01.float(), window_size=w, size_average=False).double().numpy())
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ssim.npz"), names=np.array(names), f64=np.stack(f64),
                        f32=np.stack(f32))
    err = np.abs(np.stack(f64) - np.stack(f32)).max(1)
    for n, e in zip(names, err):
        print(f"{n:28s} reference fp32 - fp64: {e:.2e}")


if __name__ == "__main__":
    main(sys.argv[1])
