#!/usr/bin/env python3
"""The KTH / BAIR / UCF input path in numbers (GPU only): dvg_clip_gather_u8's bandwidth, the time to deliver a batch
(`load()` of make_batch_generator) from a dataset tree against --synthetic_data at the same shape, a training iteration fed by
either, and the pool build time.  The tree is the tiny one of tests/clip_tree.py, written to a temporary directory.

    python tools/bench_clips.py [--no_train] [--rounds 5] [--iters 20]

Recorded values, not pass bars.  The kernel figure is (bytes in + bytes out) / time of back-to-back `ops.clip_gather` calls
against the 8 TB/s of HBM: at the training shapes a call moves 12 - 26 MB and takes what the host needs to issue it (output
allocation + ctypes), so the fraction of peak is small; the last, large shape shows the kernel itself."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import train  # noqa: E402
from dvg_amd import datasets, ops  # noqa: E402
from dvg_amd.data import make_batch_generator  # noqa: E402
from tests import clip_tree  # noqa: E402

HBM_BYTES_PER_S = 8e12


def event_us(fn, iters=200, warm=50):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def kernel_leg(dev):
    rows = []
    # the three shapes training uses, and one large enough (63 MB in, 252 MB out) for the launch cost not to matter
    for B, T, S, pc, C in ((64, 20, 64, 1, 1), (16, 12, 64, 3, 3), (4, 16, 128, 3, 3), (64, 20, 128, 3, 3)):
        n = (4 if B * T * S * S < 1 << 24 else 2) * B * T
        pool = torch.randint(0, 256, (n, S, S, pc), dtype=torch.uint8, device=dev)
        first = torch.randint(0, n - T + 1, (B,), dtype=torch.int64, device=dev)
        us = event_us(lambda: ops.clip_gather(pool, first, T, C))
        moved = B * T * S * S * (pc + 4 * C)
        rows.append({"B": B, "T": T, "size": S, "pool_c": pc, "C": C, "us": round(us, 2), "MB": round(moved / 1e6, 2),
                     "GB_per_s": round(moved / us / 1e3, 1), "of_hbm_peak": round(moved / (us * 1e-6) / HBM_BYTES_PER_S, 4)})
    return rows


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no_train", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"kernel": kernel_leg(dev)}
    with tempfile.TemporaryDirectory() as tmp:
        clip_tree.build(tmp, 0)
        # the C4 shape: dcgan_64, nc = 3, 16 clips per GPU, 2 frames in / 10 out, on the BAIR tree
        argv = ["--model", "dcgan", "--batch_size", "16", "--n_past", "2", "--n_future", "10", "--channels", "3",
                "--dataset", "bair", "--no_save", "--data_root", clip_tree.data_root(tmp, "bair")]
        real, synth = train.options(argv), train.options(argv + ["--synthetic_data"])
        index = datasets.open_index("bair", real.data_root, True)
        t0 = time.perf_counter()
        pool = datasets.build_pool(index, 64, dev, real.data_threads)
        torch.cuda.synchronize()
        out["pool_build"] = {"frames": int(pool.shape[0]), "threads": real.data_threads,
                             "s": round(time.perf_counter() - t0, 3)}
        gens = {"tree": make_batch_generator(real, 12, 1, dev), "synthetic": make_batch_generator(synth, 12, 1, dev)}
        # batch delivery: the device half alone (the host half runs ahead on train.py's prefetch thread), then both halves
        loads = {k: [next(g) for _ in range(a.iters)] for k, g in gens.items()}
        deliver = {k: [] for k in gens}
        both = {k: [] for k in gens}
        for _ in range(a.rounds):                       # interleaved: both paths see the same state of the machine
            for k, g in gens.items():
                it = iter(loads[k])
                deliver[k].append(wall_ms(lambda: next(it)(), a.iters))
                both[k].append(wall_ms(lambda: next(g)(), a.iters))
        out["load_ms"] = {k: {"device_half_median": round(statistics.median(v), 3), "device_half_all": [round(x, 3) for x in v],
                              "host_and_device_median": round(statistics.median(both[k]), 3)} for k, v in deliver.items()}
        if not a.no_train:
            torch.manual_seed(1)
            tr = train.Trainer(real, dev)
            tr.train_mode()
            step = train.GraphedIteration(tr, warmup=2)
            for _ in range(4):
                step(next(gens["tree"])())
            iters = {k: [] for k in gens}
            for _ in range(a.rounds):
                for k, g in gens.items():
                    pf = train.BatchPrefetcher(g_take(g, a.iters))
                    iters[k].append(wall_ms(lambda: step(next(pf)()), a.iters))
            out["train_iter_ms"] = {k: {"median": round(statistics.median(v), 2), "all": [round(x, 2) for x in v],
                                        "frames_per_s": round(16 * 11 / statistics.median(v) * 1e3, 1)}
                                    for k, v in iters.items()}
    print(json.dumps(out))


def g_take(gen, n):
    for _ in range(n):
        yield next(gen)


if __name__ == "__main__":
    main()
