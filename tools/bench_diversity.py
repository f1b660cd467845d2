#!/usr/bin/env python3
"""Time per call of dvg_pairwise_frame_mse (ops.pairwise_frame_mse) on the predicted half of a make_gifs sample tensor, beside
two plain-torch forms on the same frames, rounds interleaved in one process, device events (GPU only):

  direct   (x[:, None] - x[None]).square().mean(-1) per frame, a few frames at a time (it materialises S x S x D per frame)
  gram     torch.cdist(x, x)^2 / D, the norm expansion - inexact where samples coincide: its error at identical rows is printed

The kernel is timed over --iters calls (default 200), the torch forms over --torch_iters (default 3: the direct form moves
hundreds of GB per call).  The floor quoted is 2 lane-operations (subtract, multiply-add) per pair-element of the S (S - 1) / 2
pairs at the fp32 vector rate without packing: 256 CUs x 64 lanes x 2.4 GHz."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvg_amd import ops  # noqa: E402

LANE_OPS_PER_S = 256 * 64 * 2.4e9
SHAPES = ((100, 10, 64, 1, 64), (30, 10, 64, 1, 64), (100, 10, 16, 3, 128))      # S, predicted steps, B, C, width


def time_fn(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def torch_direct(x, lo, chunk_bytes=2 << 30):
    s, t, b = x.shape[:3]
    xs = x[:, lo:].reshape(s, (t - lo) * b, -1).transpose(0, 1)               # (frames, S, D) view
    step = max(1, chunk_bytes // (4 * s * s * xs.shape[-1]))
    return torch.cat([(c[:, :, None] - c[:, None]).square().mean(-1) for c in xs.split(step)])


def torch_gram(x, lo):
    s, t, b = x.shape[:3]
    xs = x[:, lo:].reshape(s, (t - lo) * b, -1).transpose(0, 1)
    return torch.cdist(xs, xs).square() / xs.shape[-1]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--torch_iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    for s, steps, b, c, w in SHAPES:
        torch.manual_seed(1)
        x = torch.rand(s, 2 * steps, b, c, w, w, device=dev)                  # n_past = steps conditioning frames in front
        x[1] = x[0]                                                           # one identical pair: what the Gram form makes of it
        d, frames = c * w * w, steps * b
        fns = {"kernel": (lambda: ops.pairwise_frame_mse(x, steps), a.iters, 20),
               "torch_direct": (lambda: torch_direct(x, steps), a.torch_iters, 1),
               "torch_gram": (lambda: torch_gram(x, steps), a.torch_iters, 1)}
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):                                             # interleaved rounds
            for k, (fn, iters, warm) in fns.items():
                ms[k].append(time_fn(fn, iters, warm))
        ours = ops.pairwise_frame_mse(x, steps).view(frames, s, s)
        direct, gram = torch_direct(x, steps), torch_gram(x, steps)
        off = ~torch.eye(s, dtype=torch.bool, device=dev)
        rel = ((ours - direct).abs()[:, off] / direct[:, off].clamp_min(1e-30)).max()
        floor_ms = 2.0 * frames * d * (s * (s - 1) // 2) / LANE_OPS_PER_S * 1e3
        print(json.dumps({"S": s, "steps": steps, "B": b, "C": c, "width": w, "floor_ms": round(floor_ms, 4),
                          **{k + "_ms": [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
                          "kernel_over_floor": round(min(ms["kernel"]) / floor_ms, 2),
                          "identical_pair": {"kernel": float(ours[:, 0, 1].abs().max()), "torch_direct": float(direct[:, 0, 1].abs().max()),
                                             "torch_gram_max": float(gram[:, 0, 1].abs().max())},
                          "typical_entry": float(direct[:, 0, 2].mean()),
                          "kernel_vs_torch_direct_max_rel": float(rel)}), flush=True)
        del x, ours, direct, gram


if __name__ == "__main__":
    main()
