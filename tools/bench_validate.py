#!/usr/bin/env python3
"""What `train.py --val_every` costs: one validation at the defaults (--val_batches 8, --val_nsample 4) against one training epoch
of the same configuration, for dcgan_64 and vgg_64 at batch 64, n_past 10, n_eval 20 on synthetic Moving-MNIST (GPU only).

  validation_ms     wall time of Validator.run on the live weights, host-synchronised (median, min, max over --rounds)
  iteration_ms      one replayed training iteration (GraphedIteration), median over --iters after the capture
  epoch_ms          iteration_ms x --epoch_size (default 300, train.py's)
  validation_over_epoch

One JSON line per model.  Nothing is gated on these numbers (docs/DESIGN_NOTES_validation.md records them)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import train  # noqa: E402
from dvg_amd.data import make_batch_generator  # noqa: E402

MODELS = ("dcgan", "vgg")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epoch_size", type=int, default=300)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--models", default=",".join(MODELS))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    for model in a.models.split(","):
        opt = train.options(["--model", model, "--batch_size", str(a.batch_size), "--n_past", "10", "--n_future", "10", "--n_eval",
                             "20", "--dataset", "smmnist", "--synthetic_data", "--val_every", "1", "--no_save"])
        torch.manual_seed(1)
        torch.cuda.manual_seed_all(1)
        tr = train.Trainer(opt, dev)
        tr.train_mode()
        gen = make_batch_generator(opt, opt.n_past + opt.n_future, 1, dev)
        step = train.GraphedIteration(tr)
        for _ in range(4):                                   # eager warm-up, capture, first replays
            step(next(gen)())
        x = next(gen)()
        its = []
        for _ in range(a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(x)
            torch.cuda.synchronize()
            its.append(1e3 * (time.perf_counter() - t0))
        val = tr.validation.validator
        val.run(tr.modules, tr)                              # first-call work: eval-mode folds, LDS attributes
        vals = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = val.run(tr.modules, tr)
            vals.append(1e3 * (time.perf_counter() - t0))     # run() ends with the readback: host-synchronised
        its.sort()
        vals.sort()
        it_ms, v_ms = its[len(its) // 2], vals[len(vals) // 2]
        print(json.dumps({"model": f"{model}_64", "batch": a.batch_size, "val_batches": val.batches, "val_nsample": val.nsample,
                          "clips": res["clips"], "steps": res["steps"],
                          "validation_ms_median_min_max": [round(v_ms, 2), round(vals[0], 2), round(vals[-1], 2)],
                          "iteration_ms": round(it_ms, 3), "epoch_size": a.epoch_size,
                          "epoch_ms": round(it_ms * a.epoch_size, 1),
                          "validation_over_epoch": round(v_ms / (it_ms * a.epoch_size), 4),
                          "score": res["score"]}), flush=True)
        del tr, step, gen, val


if __name__ == "__main__":
    main()
