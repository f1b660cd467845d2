#!/usr/bin/env python3
"""Time per call of the two metric kernels on 64x64, C = 1 frames: dvg_eval_frames (utils.eval_seq, 7x7 uniform window) and
dvg_eval_frames_finn (utils.finn_eval_seq, 11x11 Gaussian window), at one step's 64 frames and at a rollout's 64 x 15,
interleaved, device events (GPU only)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvg_amd import ops  # noqa: E402


def time_fn(fn, iters=200):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    for n in (64, 64 * 15):
        gt = torch.rand(n, 1, 64, 64, device=dev)
        pred = (gt + 0.05 * torch.randn_like(gt)).contiguous()
        fns = {"eval_frames": lambda: ops.eval_frames(gt, pred), "eval_frames_finn": lambda: ops.eval_frames_finn(gt, pred)}
        us = {k: [] for k in fns}
        for _ in range(5):                      # interleaved rounds
            for k, fn in fns.items():
                us[k].append(time_fn(fn))
        print(json.dumps({"frames": n, **{k: {"us_min": round(min(v), 1), "us_max": round(max(v), 1)} for k, v in us.items()}}),
              flush=True)


if __name__ == "__main__":
    main()
