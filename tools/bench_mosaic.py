#!/usr/bin/env python3
"""Times the make_gifs mosaic at the reference's shape (S = 100 samples, T = 30 frames, B = 64, 64 x 64, six columns, all 64
batch rows: 1920 frames of 96 x 396 pixels) under hipGraph replay, alternating

  (a) kernel: ops.frame_mosaic (dvg_frame_mosaic, one launch), and
  (b) torch:  the same mosaic with torch device ops - gather by index, clamp, mul, to(uint8), copy_ into a canvas that is
              first refilled with the borders - i.e. what the repository could do without the kernel.

Both without text labels (torch has no counterpart for them) and both checked to give the same bytes.  Prints one JSON line:
times in ms (median and spread over the repeats), the kernel's algorithmic bytes (every selected source image read once,
the mosaic written once) and its share of the 8 TB/s HBM peak.  No test asserts these numbers."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvg_amd import ops, viz  # noqa: E402

HBM_PEAK = 8e12


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--nsample", type=int, default=100)
    p.add_argument("--n_eval", type=int, default=30)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--width", type=int, default=64)
    p.add_argument("--n_past", type=int, default=5)
    p.add_argument("--replays", type=int, default=20, help="graph replays per timed window")
    p.add_argument("--repeats", type=int, default=7)
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "bench_mosaic.py needs a GPU"
    dev = torch.device("cuda", 0)
    S, T, B, H = a.nsample, a.n_eval, a.batch, a.width
    g = torch.Generator(device=dev).manual_seed(0)
    samples = torch.rand((S, T, B, 1, H, H), device=dev, generator=g) * 1.2 - 0.1
    post = torch.rand((T, B, 1, H, H), device=dev, generator=g) * 1.2 - 0.1
    gt = torch.rand((T, B, 1, H, H), device=dev, generator=g)
    best = torch.randint(0, S, (B,), device=dev, generator=g)
    picks = torch.from_numpy(viz.random_picks(1, B, 3, S)).to(dev)
    lay = viz.make_gifs_layout(T, a.n_past, B, H, rows=B)
    cells, _ = lay.upload(dev, with_labels=False)
    kw = dict(nc=1, H=H, W=H, F=lay.F, R=1, Cc=6, cell_h=lay.cell_h, cell_w=lay.cell_w, oy=1, ox=1, best=best, picks=picks,
              quant=viz.QUANT_TRUNC)

    def kernel():
        return ops.frame_mosaic([gt, post, samples], cells, **kw)

    # (b): background canvas (borders by column and time) built once; per call: refill, gather, convert, paste
    ch, cw = lay.cell_h, lay.cell_w
    bg = torch.zeros((B, T, ch, 6 * cw, 3), dtype=torch.uint8, device=dev)
    bg[:, :, :, :cw, 1] = 178
    bg[:, :a.n_past, :, cw:, 1] = 178
    bg[:, a.n_past:, :, cw:, 0] = 178
    canvas = torch.empty_like(bg)
    rows = torch.arange(B, device=dev)

    def torch_way():
        canvas.copy_(bg)
        cols = [gt.transpose(0, 1), post.transpose(0, 1), samples[best, :, rows]] + \
               [samples[picks[:, k].long(), :, rows] for k in range(3)]               # each (B,T,1,H,H)
        for c, col in enumerate(cols):
            q = col.clamp(0, 1).mul(255).to(torch.uint8).squeeze(2).unsqueeze(-1)
            canvas[:, :, 1:1 + H, c * cw + 1:c * cw + 1 + H, :] = q.expand(-1, -1, -1, -1, 3)
        return canvas

    same = torch.equal(kernel().view(B, T, ch, 6 * cw, 3), torch_way())
    graphs = {}
    for name, fn in (("kernel", kernel), ("torch", torch_way)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            keep = fn()                                                             # noqa: F841 - output lives in the pool
        graphs[name] = (gr, keep)
    times = {"kernel": [], "torch": []}
    for _ in range(a.repeats):
        for name in ("kernel", "torch"):                                            # alternating
            gr = graphs[name][0]
            gr.replay()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.replays):
                gr.replay()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.replays)
    out_bytes = lay.F * lay.grid_h * lay.grid_w * 3
    read_bytes = lay.F * 6 * H * H * 4
    km, tm = statistics.median(times["kernel"]), statistics.median(times["torch"])
    print(json.dumps({
        "bench": "frame_mosaic", "shape": {"S": S, "T": T, "B": B, "HxW": H, "frames": lay.F, "frame": [lay.grid_h, lay.grid_w]},
        "same_bytes": bool(same), "kernel_ms": round(km, 4), "kernel_ms_min_max": [round(min(times["kernel"]), 4), round(max(times["kernel"]), 4)],
        "torch_ms": round(tm, 4), "torch_ms_min_max": [round(min(times["torch"]), 4), round(max(times["torch"]), 4)],
        "torch_over_kernel": round(tm / km, 2), "algorithmic_bytes": read_bytes + out_bytes,
        "kernel_share_of_hbm_peak": round((read_bytes + out_bytes) / (km * 1e-3) / HBM_PEAK, 4),
        "replays": a.replays, "repeats": a.repeats}))


if __name__ == "__main__":
    main()
