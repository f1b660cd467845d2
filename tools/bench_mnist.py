#!/usr/bin/env python3
"""The Moving-MNIST input path over real digits in numbers (GPU only).  Recorded values, not pass bars; no test asserts them.

  scale    ops.mnist_scale_u8 (dvg_mnist_scale_u8) over 60 000 digits 28x28 -> 32x32, the train split's one-off, under
           hipGraph replay; algorithmic bytes = digits read + digits written.
  compose  ops.moving_mnist_compose_u8 (uint8 pool of 60 000 digits) against ops.moving_mnist_compose (the float32 pool of the
           same digits) at B = 64, T = 20, S = 64, two digits, the same trajectories: both under hipGraph replay, alternating in
           one process, and checked to give the same bits.  Algorithmic bytes = the frames written (the digits read are 1/8 of
           that and served from cache).
  batch    the device half of a batch as train.py gets it: `load()` of make_batch_generator's MNIST branch - the upload of
           ids / pos from pageable host memory plus the compose launch - timed on the host clock around a device synchronise
           (an upload from pageable memory cannot be captured in a graph).

Digits are seeded noise of MNIST's shape and count: the kernels' time does not depend on the bytes.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvg_amd import data, mnist, ops  # noqa: E402

HBM_PEAK = 8e12


def graph_of(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        keep = fn()
    return gr, keep


def replay_ms(gr, replays):
    gr.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / replays


def stats(ms):
    return {"ms": round(statistics.median(ms), 5), "ms_min_max": [round(min(ms), 5), round(max(ms), 5)]}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--digits", type=int, default=60000)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--seq_len", type=int, default=20)
    p.add_argument("--width", type=int, default=64)
    p.add_argument("--replays", type=int, default=200, help="graph replays per timed window")
    p.add_argument("--repeats", type=int, default=7)
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "bench_mnist.py needs a GPU"
    dev = torch.device("cuda", 0)
    N, B, T, S = a.digits, a.batch, a.seq_len, a.width
    rng = np.random.default_rng(0)
    raw = torch.from_numpy(rng.integers(0, 256, (N, 28, 28), dtype=np.uint8)).to(dev)
    tables = [torch.from_numpy(t).to(dev) for t in mnist.resize_tables(28, 32)]

    sprites = ops.mnist_scale_u8(raw, 32)
    sample = rng.integers(0, N, 64)
    scale_ok = np.array_equal(sprites[sample].cpu().numpy(), mnist.resize_u8(raw[sample].cpu().numpy(), 32))
    gr_scale, _ = graph_of(lambda: ops.mnist_scale_u8(raw, 32, tables))
    scale = [replay_ms(gr_scale, max(1, a.replays // 4)) for _ in range(a.repeats)]
    scale_bytes = N * (28 * 28 + 32 * 32)

    ids, pos = mnist.MovingMnistSampler(N, T, 2, S, 1).draw(B)
    dids, dpos = torch.from_numpy(ids).to(dev), torch.from_numpy(pos).to(dev)
    fsprites = (sprites.cpu().float() / 255).to(dev)      # divided on the host: torch's device tensor / scalar multiplies by 1/255
    fns = {"u8": lambda: ops.moving_mnist_compose_u8(sprites, dids, dpos, T, S),
           "f32": lambda: ops.moving_mnist_compose(fsprites, dids, dpos, T, S)}
    same = torch.equal(fns["u8"](), fns["f32"]())
    graphs = {k: graph_of(f) for k, f in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(a.repeats):
        for k in fns:                                                          # alternating
            times[k].append(replay_ms(graphs[k][0], a.replays))
    out_bytes = T * B * S * S * 4

    # the device half of a batch through make_batch_generator: a tree with the noise digits as both splits
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        blob = (0x803).to_bytes(4, "big") + N.to_bytes(4, "big") + (28).to_bytes(4, "big") * 2 + raw.cpu().numpy().tobytes()
        for name in mnist.FILES.values():
            with open(os.path.join(tmp, name), "wb") as f:
                f.write(blob)
        opt = types.SimpleNamespace(dataset="smmnist", data_root=tmp, image_width=S, channels=1, local_batch=B, rank=0,
                                    num_digits=2, synthetic_data=False)
        t0 = time.perf_counter()
        gen = data.make_batch_generator(opt, T, 1, dev)
        torch.cuda.synchronize()
        setup_s = time.perf_counter() - t0
    loads = [next(gen) for _ in range(8 + 50 * a.repeats)]
    for ld in loads[:8]:
        ld()
    torch.cuda.synchronize()
    batch = []
    for r in range(a.repeats):
        t0 = time.perf_counter()
        for ld in loads[8 + 50 * r:8 + 50 * (r + 1)]:
            ld()
        torch.cuda.synchronize()
        batch.append((time.perf_counter() - t0) * 1e3 / 50)
    t0 = time.perf_counter()
    mnist.MovingMnistSampler(N, T, 2, S, 1).draw(B)
    draw_ms = (time.perf_counter() - t0) * 1e3

    su, sf = stats(times["u8"]), stats(times["f32"])
    print(json.dumps({
        "bench": "mnist", "shape": {"digits": N, "B": B, "T": T, "S": S, "num_digits": 2},
        "scale": dict(stats(scale), equals_numpy_restatement=bool(scale_ok), algorithmic_bytes=scale_bytes,
                      share_of_hbm_peak=round(scale_bytes / (statistics.median(scale) * 1e-3) / HBM_PEAK, 4)),
        "compose_u8": dict(su, share_of_hbm_peak=round(out_bytes / (su["ms"] * 1e-3) / HBM_PEAK, 4)),
        "compose_f32": dict(sf, share_of_hbm_peak=round(out_bytes / (sf["ms"] * 1e-3) / HBM_PEAK, 4)),
        "compose_same_bits": bool(same), "f32_over_u8": round(sf["ms"] / su["ms"], 3), "compose_bytes_written": out_bytes,
        "pool_bytes": {"u8": sprites.numel(), "f32": fsprites.numel() * 4},
        "batch_device_half": dict(stats(batch), what="upload of ids / pos + compose, host clock, 50 batches per window"),
        "host_draw_ms_per_batch": round(draw_ms, 3), "read_upload_scale_s": round(setup_s, 3),
        "replays": a.replays, "repeats": a.repeats}))


if __name__ == "__main__":
    main()
