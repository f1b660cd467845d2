#!/usr/bin/env python3
"""Time per call of the frame-loss kernels on the training shape (S = 19 steps, K = 3 decoder calls, 64 planes of 64 x 64: vgg_64 /
dcgan_64 at batch 64, one channel; GPU only, device events, rounds interleaved in one process):

  ext_l1_gdl   dvg_frame_losses_ext, l1, G = 1: the pixel term, the four edge terms per pixel and their gradient
  ext_l1       the same kernel with G = 0: no halo rows, no edge work
  mse          dvg_frame_losses - the yardstick: the plain streaming kernel of the same build on the same box
  ssim         dvg_frame_ssim_loss, accumulate = 1 (the training use: dpred read, the DSSIM gradient added, written back): the
               separable fp64 window passes forward and transposed, ~SSIM_FMAS_PER_PIXEL fp64 FMAs per pixel of pred

The first three move the same algorithmic bytes: pred read and dpred written (2 x S K n floats) and target read once (S n); `ssim`
reads dpred as well (3 x S K n + S n).  `before`
every timed call 1 GB of other traffic goes through the caches (the 89 MB working set would otherwise sit in the Infinity Cache).
Per leg the line lists (median, min, max) ms of every round; the derived figures use the SMALLEST of a leg's round medians."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_gradguard import HBM_BYTES_PER_S, timed  # noqa: E402
from dvg_amd import ops  # noqa: E402

# fp64 FMAs per pixel of one call, whole-image form, borders ignored: row pass 11 taps x 3 moments, column pass 11 x 3, the a, b, c
# maps ~30, transposed column pass 11 x 3, transposed row pass 11 x 3 + 3; the target's two moments (22 + 22) are shared by the K calls
SSIM_FMAS_PER_PIXEL = 4 * 33 + 30 + 3
FP64_VECTOR_FMAS_PER_S = 78.6e12 / 2       # MI355X: 78.6 TFLOP/s fp64 vector


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=5, default=[19, 3, 64, 64, 64], metavar=("S", "K", "PLANES", "H", "W"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    S, K, planes, H, W = a.shape
    torch.manual_seed(1)
    target = torch.rand(S, planes, H, W, device=dev)
    pred = (target.unsqueeze(1) + 0.1 * torch.randn(S, K, planes, H, W, device=dev)).contiguous()
    n = planes * H * W
    w = [0.001 / n, 1000.0 / n, 0.001 / n][:K]
    trash = torch.empty(1 << 28, device=dev)                    # 1 GB: more than the 256 MB Infinity Cache
    flat_p, flat_t = pred.view(S, K, -1), target.view(S, -1)
    legs = {"ext_l1_gdl": lambda: ops.frame_losses_ext(pred, target, "l1", w, gdl=1.0),
            "ext_l1": lambda: ops.frame_losses_ext(pred, target, "l1", w, gdl=0.0),
            "mse": lambda: ops.frame_losses(flat_p, flat_t, w)}
    if H >= 11 and W >= 11:
        m = planes * (H - 10) * (W - 10)
        w_s = [0.2 * x * n / m for x in w]
        d_acc = torch.zeros_like(pred)                          # stays finite: the weights are ~1e-9 ... 1e-3 per call
        legs["ssim"] = lambda: ops.frame_ssim_loss(pred, target, w_s, dpred=d_acc)
    for fn in legs.values():                                    # warm-up: code objects loaded, weights cached, allocator settled
        trash.zero_()
        fn()
    res = {k: [] for k in legs}
    for _ in range(a.rounds):                                   # interleaved rounds
        for k, fn in legs.items():
            res[k].append(timed(fn, a.iters, trash.zero_))
    nbytes = 4.0 * (2 * pred.numel() + target.numel())
    best = {k: min(r[0] for r in v) for k, v in res.items()}
    ssim = {}
    if "ssim" in legs:
        sbytes, fmas = nbytes + 4.0 * pred.numel(), float(SSIM_FMAS_PER_PIXEL) * pred.numel() + 44.0 * target.numel()
        ssim = {"workgroups_ssim": ops.lib().dvg_frame_ssim_loss_blocks(S, planes, H, W), "ssim_algorithmic_MB": round(sbytes / 1e6, 1),
                "ssim_fp64_GFMA": round(fmas / 1e9, 3), "ssim_floor_ms_bytes": round(sbytes / HBM_BYTES_PER_S * 1e3, 5),
                "ssim_floor_ms_fp64": round(fmas / FP64_VECTOR_FMAS_PER_S * 1e3, 5), "ssim_over_mse_time": round(best["ssim"] / best["mse"], 2)}
    print(json.dumps({"shape": a.shape, "algorithmic_MB": round(nbytes / 1e6, 1), "floor_ms_at_8TBps": round(nbytes / HBM_BYTES_PER_S * 1e3, 5),
                      "workgroups_ext": ops.lib().dvg_frame_losses_ext_blocks(S, planes, H, W),
                      **{k + "_ms_median_min_max": [[round(x, 5) for x in r] for r in v] for k, v in res.items()},
                      **{k + "_TBps": round(nbytes / best[k] / 1e9, 2) for k in best if k != "ssim"},
                      **{k + "_fraction_of_8TBps": round(nbytes / HBM_BYTES_PER_S * 1e3 / best[k], 3) for k in best if k != "ssim"}, **ssim,
                      "ext_l1_gdl_over_mse_time": round(best["ext_l1_gdl"] / best["mse"], 3),
                      "ext_l1_over_mse_time": round(best["ext_l1"] / best["mse"], 3)}), flush=True)


if __name__ == "__main__":
    main()
