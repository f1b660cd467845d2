#!/usr/bin/env python3
"""What the sampler's per-row variance trigger costs (GPU only; docs/DESIGN_NOTES_trigger_rows.md records the output).

  launch     microseconds per dvg_gp_trigger_rows launch (a deciding step, window 12) at (D, B) = (90, 50) and (90, 64), beside the
             three launches the per-index path spends on the same bookkeeping for ONE row - gp_var_norms + gp_trigger_step +
             gp_trigger_select (no recurrent state).  The two alternate in one process, the new launch timed twice per round:
             `spread` = |first - again| / first is what two timings of the SAME launch differ by in this run.  HIP events around
             --launches back-to-back launches, median of --rounds.
  make_gifs  delivered frames/s (B x n_future x nsample / wall time of the whole call) of Generator.make_gifs at B = 64, 10-in /
             20-out, nsample 12, for both backbone families: --trigger period and --trigger variance (window 12, the default
             coefficient) alternating in one process, the period rule timed twice per round (the same spread column).

One JSON line per measurement.  Nothing is gated on these numbers."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import generate_frames  # noqa: E402
from dvg_amd import benchlib, ops, rollout  # noqa: E402
from dvg_amd.data import SyntheticMovingMNIST  # noqa: E402

SHAPES = ((90, 50), (90, 64))
WINDOW = 12


def _event_us(run, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        run()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / launches


def _median(v):
    return sorted(v)[len(v) // 2]


def launch_times(launches, rounds, dev):
    for D, B in SHAPES:
        g = torch.Generator(device=dev).manual_seed(D + B)
        var = torch.rand(D, B, device=dev, generator=g) + 0.1
        sample, h_pred = torch.randn(D, B, device=dev, generator=g), torch.randn(B, D, device=dev, generator=g)
        trig = rollout.VarianceTrigger(WINDOW)
        st = trig.new_state(B, 2, dev)
        st["win"].copy_(torch.rand(B, WINDOW, device=dev, generator=g))
        ctx, log = torch.rand(WINDOW, device=dev, generator=g), rollout.trigger_log(2, dev)

        def rows():     # a deciding step: pos = window, a slide (step = slot = 1)
            return ops.gp_trigger_rows(var, st["win"], st["last"], st["values"], st["thresholds"], st["flags"], pos=WINDOW, step=1,
                                       slot=1, decide=True, coef=trig.coef, sample_db=sample, h_pred=h_pred)

        def three():
            ops.gp_var_norms(var)
            ops.gp_trigger_step(var, 3, ctx, trig.coef, log["flag"], log["values"], log["thresholds"], log["flags"], 1)
            ops.gp_trigger_select(log["flag"], sample, h_pred, [], [])
        for _ in range(10):
            rows(), three()
        t = {"rows": [], "three_launches": [], "rows_again": []}
        for _ in range(rounds):
            t["rows"].append(_event_us(rows, launches))
            t["three_launches"].append(_event_us(three, launches))
            t["rows_again"].append(_event_us(rows, launches))
        a, b, c = (_median(t[k]) for k in ("rows", "three_launches", "rows_again"))
        print(json.dumps({"what": "launch", "D": D, "B": B, "window": WINDOW, "launches": launches, "rounds": rounds,
                          "us_rows": round(a, 2), "us_rows_again": round(c, 2), "spread": round(abs(a - c) / a, 4),
                          "us_three_launches": round(b, 2), "three_over_rows": round(b / a, 3)}), flush=True)


def make_gifs_times(rounds, dev, batch=64, n_past=10, n_future=20, nsample=12):
    n_eval = n_past + n_future
    for model in ("dcgan", "vgg"):
        base = ["--synthetic_ckpt", "--batch_size", str(batch), "--model", model, "--n_past", str(n_past), "--n_eval", str(n_eval)]
        gens = {}
        for rule in ("period", "variance"):
            opt = generate_frames.parse_args(base + ["--trigger", rule])
            torch.manual_seed(1)
            gens[rule] = generate_frames.Generator(opt, generate_frames.synthetic_checkpoint(opt), dev)
        x = SyntheticMovingMNIST(seq_len=n_eval, seed=1).batch_device(batch, dev)
        for g in gens.values():
            benchlib.calibrate_batchnorm(g.encoder, g.decoder, x[0])
            g.make_gifs(x, 3)                  # weight packs, the captures
        torch.cuda.synchronize()

        def timed(g):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = g.make_gifs(x, nsample)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, res
        t = {"period": [], "variance": [], "period_again": []}
        for _ in range(rounds):
            t["period"].append(timed(gens["period"])[0])
            dt, res = timed(gens["variance"])
            t["variance"].append(dt)
            t["period_again"].append(timed(gens["period"])[0])
        fps = lambda s: round(batch * n_future * nsample / s, 1)   # noqa: E731
        a, b, c = (_median(t[k]) for k in ("period", "variance", "period_again"))
        mean, lo, hi, never, first = generate_frames.trigger_summary(res["trigger"]["flags"], n_past)
        print(json.dumps({"what": "make_gifs", "model": model + "_64", "batch": batch, "n_past": n_past, "n_future": n_future,
                          "nsample": nsample, "rounds": rounds, "fps_period": fps(a), "fps_period_again": fps(c),
                          "spread": round(abs(a - c) / a, 4), "fps_variance": fps(b), "variance_over_period_time": round(b / a, 3),
                          "ms_period": round(1e3 * a, 2), "ms_variance": round(1e3 * b, 2),
                          "draws_per_sequence_mean_min_max": [round(mean, 3), lo, hi], "never_drew": round(never, 4)}), flush=True)
        del gens


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--what", default="launch,make_gifs")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    what = a.what.split(",")
    "launch" in what and launch_times(a.launches, a.rounds, dev)
    "make_gifs" in what and make_gifs_times(a.rounds, dev)


if __name__ == "__main__":
    main()
