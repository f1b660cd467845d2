#!/usr/bin/env python3
"""`--augment` in numbers (GPU only): dvg_clip_gather_aug_u8 against dvg_clip_gather_u8 at the four shapes of
docs/DESIGN_NOTES_clips.md - the plain gather, the augmented gather with identity parameters and with every transform on,
interleaved in one process - and `load()` of make_batch_generator with and without `--augment` on the trees of
tests/clip_tree.py.

    python tools/bench_clip_augment.py [--rounds 7] [--iters 200] [--load_iters 50]

Recorded values, not pass bars (docs/DESIGN_NOTES_augment.md holds the table).  A kernel figure is the event time of `iters`
back-to-back calls of the op, device-resident parameters, after a warm-up; per shape the three forms alternate round by round so
that they see the same state of the machine, and the median and the spread over the rounds are reported.  All three move the
same bytes: pool_c in, 4 C out per pixel."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import train  # noqa: E402
from dvg_amd import ops  # noqa: E402
from dvg_amd.data import make_batch_generator  # noqa: E402
from tests import clip_tree  # noqa: E402

HBM_BYTES_PER_S = 8e12
SHAPES = ((64, 20, 64, 1, 1), (16, 12, 64, 3, 3), (4, 16, 128, 3, 3), (64, 20, 128, 3, 3))     # B, T, size, pool_c, C
FULL = "hflip,reverse,shift=4,jitter=0.2"


def event_us(fn, iters):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def spread(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def kernel_leg(dev, rounds, iters):
    rows = []
    rng = np.random.RandomState(3)
    for B, T, S, pc, C in SHAPES:
        n = (4 if B * T * S * S < 1 << 24 else 2) * B * T
        pool = torch.randint(0, 256, (n, S, S, pc), dtype=torch.uint8, device=dev)
        first = torch.randint(0, n - T + 1, (B,), dtype=torch.int64, device=dev)
        ident = (torch.zeros((B, 4), dtype=torch.int32, device=dev), torch.tensor([[1.0, 0.0]] * B, device=dev))
        geom = np.stack([rng.randint(0, 2, B), rng.randint(0, 2, B), rng.randint(-16, 17, B), rng.randint(-16, 17, B)], 1)
        gain = 1 + rng.uniform(-0.2, 0.2, B)
        photo = np.stack([gain, 0.5 - 0.5 * gain + rng.uniform(-0.1, 0.1, B)], 1)
        full = (torch.from_numpy(geom.astype(np.int32)).to(dev), torch.from_numpy(photo.astype(np.float32)).to(dev))
        forms = {"plain": lambda: ops.clip_gather(pool, first, T, C),
                 "aug_identity": lambda: ops.clip_gather_aug(pool, first, ident[0], ident[1], T, C),
                 "aug_full": lambda: ops.clip_gather_aug(pool, first, full[0], full[1], T, C)}
        assert torch.equal(forms["plain"](), forms["aug_identity"]())        # the same result before the same bytes are timed
        for fn in forms.values():
            event_us(fn, max(iters // 4, 10))                               # warm-up of every form at this shape
        us = {k: [] for k in forms}
        for _ in range(rounds):                                              # interleaved
            for k, fn in forms.items():
                us[k].append(event_us(fn, iters))
        moved = B * T * S * S * (pc + 4 * C)
        med = {k: statistics.median(v) for k, v in us.items()}
        rows.append({"B": B, "T": T, "size": S, "pool_c": pc, "C": C, "MB": round(moved / 1e6, 2),
                     "us": {k: spread(v) for k, v in us.items()},
                     "of_hbm_peak": {k: round(moved / (m * 1e-6) / HBM_BYTES_PER_S, 4) for k, m in med.items()},
                     "aug_identity_over_plain": round(med["aug_identity"] / med["plain"], 3),
                     "aug_full_over_plain": round(med["aug_full"] / med["plain"], 3)})
    return rows


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def load_leg(dev, tmp, rounds, iters):
    """The device half of a batch (upload + launch, the host half drawn beforehand as train.py's prefetch thread does) and both
    halves, with and without --augment, at training shapes on the tiny trees."""
    out = {}
    for dataset, channels, batch, seq in (("bair", 3, 16, 12), ("kth", 1, 64, 12)):
        argv = ["--model", "dcgan", "--batch_size", str(batch), "--n_past", "2", "--n_future", str(seq - 2), "--channels",
                str(channels), "--dataset", dataset, "--no_save", "--data_root", clip_tree.data_root(tmp, dataset)]
        gens = {}
        for name, extra in (("plain", []), ("augment", ["--augment", FULL])):
            o = train.options(argv + extra)
            gens[name] = make_batch_generator(o, seq, 1, dev)
        for g in gens.values():
            wall_ms(lambda: next(g)(), 10)
        device_half, both = {k: [] for k in gens}, {k: [] for k in gens}
        for _ in range(rounds):                                              # interleaved
            for k, g in gens.items():
                it = iter([next(g) for _ in range(iters)])
                device_half[k].append(wall_ms(lambda: next(it)(), iters) * 1e3)
                both[k].append(wall_ms(lambda: next(g)(), iters) * 1e3)
        out[f"{dataset} B={batch} T={seq} C={channels}"] = {
            k: {"device_half_us": spread(device_half[k]), "host_and_device_us": spread(both[k])} for k in gens}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--load_iters", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_clip_augment.py needs a GPU"
    dev = torch.device("cuda:0")
    out = {"kernel": kernel_leg(dev, a.rounds, a.iters)}
    with tempfile.TemporaryDirectory() as tmp:
        clip_tree.build(tmp, 0)
        out["load"] = load_leg(dev, tmp, a.rounds, a.load_iters)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
