#!/usr/bin/env python3
"""Writes tests/golden/reference_finn.npz: outputs of the REFERENCE's own utils.finn_ssim, utils.finn_psnr and
utils.mse_metric (utils.py:215-218, 259-301) on the seeded inputs of tests/finn_ref.py.

Run in the build container only (needs the reference tree; CPU, numpy and scipy.signal are enough):

    python tests/golden/make_golden_finn.py [path of the reference, default: the one make_golden.py uses]

The reference's utils.py is imported as make_golden_viz.py imports it (modules it does not need here are replaced by empty
stand-ins).  utils.finn_eval_seq as a whole does not run under a current torch / numpy: it hands tensors to mse_metric, whose
np.sum raises TypeError.  So its three ingredients are called per image -
  * finn_ssim with tensor arguments (it converts to float64 itself), the map's mean stored, NaN kept;
  * finn_psnr and mse_metric with numpy arguments, float64 views of the same float32 values (finn_ssim's own precision) -
and the (bs, T) assembly (channel mean, NaN -> -1) is restated in tests/finn_ref.py.  The file holds outputs only: per case
`<name>/ssim` (N,C), `<name>/psnr` (N,C), `<name>/mse` (N,)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)


def main():
    from make_golden_viz import REF, reference_utils
    from tests import finn_ref
    ref = reference_utils(sys.argv[1] if len(sys.argv) > 1 else REF)
    out = {}
    for name in finn_ref.CASES:
        gt, pred = finn_ref.case(name)
        n, c = gt.shape[:2]
        ssim, psnr, mse = np.zeros((n, c)), np.zeros((n, c)), np.zeros(n)
        g64, p64 = gt.astype(np.float64), pred.astype(np.float64)
        for i in range(n):
            for k in range(c):
                ssim[i, k] = ref.finn_ssim(torch.from_numpy(gt[i, k]), torch.from_numpy(pred[i, k])).mean()
                psnr[i, k] = ref.finn_psnr(g64[i, k], p64[i, k])
            mse[i] = ref.mse_metric(g64[i], p64[i])
        out[name + "/ssim"], out[name + "/psnr"], out[name + "/mse"] = ssim, psnr, mse
    path = os.path.join(HERE, "reference_finn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(finn_ref.CASES), "cases")


if __name__ == "__main__":
    main()
