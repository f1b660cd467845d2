#!/usr/bin/env python3
"""What the GP scores cost and, on untrained weights, what they read (GPU only; docs/DESIGN_NOTES_gp_score.md records the output).

  launch      microseconds per dvg_gp_score launch at (R, B) = (90, 64) - one step of a batch - and (14 * 90, 64) - a rollout
              track's 14 steps as the scorer launches them -, HIP events around --launches back-to-back launches, median of --rounds
  validation  wall time of one validation (Validator.run, host-synchronised: it ends with the readback) with and without
              --val_gp, dcgan_64 at batch 64, n_past 10, n_eval 20, --val_batches 8, --val_nsample 4 on synthetic Moving-MNIST
  kernels     the pooled numbers of both tracks for a synthetic (untrained) dcgan_64 checkpoint and each --gp_kernel: they show
              that the instrument runs, and say nothing about which covariance is better

One JSON line per measurement.  Nothing is gated on these numbers."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import generate_frames  # noqa: E402
import train  # noqa: E402
import utils  # noqa: E402
from dvg_amd import gp_score, ops, rollout  # noqa: E402
from dvg_amd.data import SyntheticMovingMNIST  # noqa: E402

SHAPES = ((90, 64), (14 * 90, 64))


def launch_times(launches, rounds, dev):
    for R, B in SHAPES:
        g = torch.Generator(device=dev).manual_seed(R)
        mean, target = (torch.randn(R, B, device=dev, generator=g) for _ in range(2))
        var = torch.rand(R, B, device=dev, generator=g) + 0.1
        noise = torch.rand(90, device=dev, generator=g) + 0.01
        acc, cnt = ops.gp_score_accumulators(R, dev)
        tgt = target.t().contiguous().t()      # a strided target, as the scorer passes it
        run = lambda: ops.gp_score(mean, var, tgt, acc, cnt, noise=noise, noise_period=90)   # noqa: E731
        for _ in range(10):
            run()
        us = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                run()
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / launches)
        us.sort()
        print(json.dumps({"what": "launch", "R": R, "B": B, "launches": launches,
                          "us_per_launch_median_min_max": [round(us[len(us) // 2], 2), round(us[0], 2), round(us[-1], 2)]}), flush=True)


def validation_times(rounds, dev):
    base = ["--model", "dcgan", "--batch_size", "64", "--n_past", "10", "--n_future", "10", "--n_eval", "20", "--dataset", "smmnist",
            "--synthetic_data", "--val_every", "1", "--no_save"]
    out = {}
    for name, extra in (("val_every", []), ("val_every_val_gp", ["--val_gp"])):
        torch.manual_seed(1)
        torch.cuda.manual_seed_all(1)
        tr = train.Trainer(train.options(base + extra), dev)
        val = tr.validation.validator
        val.run(tr.modules, tr)                              # first-call work: eval-mode folds, LDS attributes, the GP's initialisation
        ms = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            val.run(tr.modules, tr)
            ms.append(1e3 * (time.perf_counter() - t0))
        ms.sort()
        out[name] = ms
        del tr, val
    a, b = (out[k][len(out[k]) // 2] for k in ("val_every", "val_every_val_gp"))
    print(json.dumps({"what": "validation", "model": "dcgan_64", "batch": 64, "val_batches": 8, "val_nsample": 4, "rounds": rounds,
                      "ms_val_every": [round(v, 2) for v in out["val_every"]],
                      "ms_val_every_val_gp": [round(v, 2) for v in out["val_every_val_gp"]],
                      "added_ms_median": round(b - a, 2), "added_over_validation": round((b - a) / a, 4)}), flush=True)


def kernel_numbers(dev):
    args = ["--synthetic_ckpt", "--model", "dcgan", "--dataset", "smmnist", "--batch_size", "16", "--n_past", "5", "--n_eval", "15",
            "--n_future", "10"]
    for kernel in ops.GP_KERNELS:
        opt = generate_frames.build_parser().parse_args(args + ["--gp_kernel", kernel])
        torch.manual_seed(1)
        torch.cuda.manual_seed_all(1)
        gen = generate_frames.Generator(opt, generate_frames.synthetic_checkpoint(opt), dev)
        ds = SyntheticMovingMNIST(seq_len=opt.n_eval, image_size=opt.image_width, seed=opt.seed + 7919)
        scorer = gen.gp_scorer()
        for _ in range(4):
            x = utils.normalize_data(opt, torch.cuda.FloatTensor, ds.batch(opt.batch_size))[0]
            state = rollout.condition(gen.encoder, gen.frame_predictor, x, opt.n_past, False, decoder=gen.decoder)
            post = rollout.posterior_from(state, gen.encoder, gen.decoder, gen.frame_predictor, gen.gp_layer, gen.likelihood,
                                          opt.n_past, opt.n_eval, False)
            gen.score_gp(scorer, x, post)
        rep = scorer.read()
        for track in gp_score.TRACKS:
            p = rep[track]["pooled"]
            print(json.dumps({"what": "untrained weights", "gp_kernel": kernel, "track": track,
                              **{k: (round(v, 5) if isinstance(v, float) else v) for k, v in p.items() if k != "pit"},
                              "pit": [round(v, 3) for v in p["pit"]]}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--what", default="launch,validation,kernels")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    what = a.what.split(",")
    "launch" in what and launch_times(a.launches, a.rounds, dev)
    "validation" in what and validation_times(a.rounds, dev)
    "kernels" in what and kernel_numbers(dev)


if __name__ == "__main__":
    main()
