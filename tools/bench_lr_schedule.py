#!/usr/bin/env python3
"""What `train.py --lr_schedule` costs per training iteration (GPU only): the dcgan_64 and vgg_64 iteration under hipGraph
(train.GraphedIteration), B = 64, T = 20, with and without `--lr_schedule cosine`, both in ONE process on one box, rounds
interleaved.

  plain    the iteration as it is without the flag: dvg_adam_step at its six step sites
  cosine   the same iteration with dvg_lr_schedule_tick in front (one thread) and dvg_adam_step_scheduled at the step sites (one
           4-byte read more per launch)
  plain_b  a SECOND Trainer and capture of the plain leg: what two instances of the same iteration differ by in one process
           (another private pool, other addresses) - the yardstick for the difference between plain and cosine

All legs train from the same seed on the same batch; a call is timed on the host around the replay and the read-back of its
losses, as train.py's loop pays it.  Per leg the line lists the median ms per iteration of every round; `cosine_minus_plain_ms` is
the difference of the legs' medians over the rounds, `plain_spread_ms` the distance between the smallest and the largest round
median of the plain leg, `plain_b_minus_plain_ms` the same difference between the two unscheduled instances - a difference inside
either is not resolved by this run."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import train  # noqa: E402
import utils  # noqa: E402
from dvg_amd.data import SyntheticMovingMNIST  # noqa: E402

MODELS = ("dcgan", "vgg")


def make_leg(model, batch, frames, extra):
    o = train.options(["--model", model, "--batch_size", str(batch), "--n_past", str(frames // 2),
                       "--n_future", str(frames - frames // 2), "--no_save"] + extra)
    torch.manual_seed(1)
    tr = train.Trainer(o, torch.device("cuda:0"))
    tr.train_mode()
    x, _ = utils.normalize_data(o, torch.cuda.FloatTensor, SyntheticMovingMNIST(seq_len=frames, seed=1).batch(batch))
    step = train.GraphedIteration(tr, warmup=2)
    for _ in range(4):                     # two eager iterations, the capture and its replay, one more replay
        step(x)
    assert step.graph is not None and not step.failed, "the iteration was not captured"
    return tr, step, x


def timed_round(step, x, iters):
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(x)                            # replays and reads the losses back: synchronous
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10, help="iterations per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--models", nargs="+", default=list(MODELS), choices=MODELS)
    a = ap.parse_args(argv)
    total = str(4 + 2 * a.rounds * a.iters)                 # the decay spans the run: the multiplier moves at every replay
    for model in a.models:
        legs = {"plain": make_leg(model, a.batch, a.frames, []),
                "cosine": make_leg(model, a.batch, a.frames, ["--lr_schedule", "cosine", "--lr_warmup", "2", "--lr_total", total]),
                "plain_b": make_leg(model, a.batch, a.frames, [])}
        graphs = {k: leg[1].graph for k, leg in legs.items()}
        res = {k: [] for k in legs}
        for _ in range(a.rounds):                           # interleaved rounds
            for k, (_, step, x) in legs.items():
                res[k].append(timed_round(step, x, a.iters))
        assert all(legs[k][1].graph is graphs[k] for k in legs), "a leg re-captured while it was timed"
        med = {k: statistics.median(v) for k, v in res.items()}
        sched = legs["cosine"][0].lr_schedule.read()
        print(json.dumps({"model": f"{model}_64", "batch": a.batch, "T": a.frames, "launch": "hipGraph replay",
                          "iters_per_round": a.iters,
                          **{k + "_ms_round_medians": [round(v, 3) for v in r] for k, r in res.items()},
                          "plain_ms": round(med["plain"], 3), "cosine_ms": round(med["cosine"], 3), "plain_b_ms": round(med["plain_b"], 3),
                          "cosine_minus_plain_ms": round(med["cosine"] - med["plain"], 3),
                          "plain_spread_ms": round(max(res["plain"]) - min(res["plain"]), 3),
                          "plain_b_minus_plain_ms": round(med["plain_b"] - med["plain"], 3),
                          "schedule_iters": sched["iters"], "schedule_multiplier": sched["scale"]}), flush=True)
        del legs, graphs
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
