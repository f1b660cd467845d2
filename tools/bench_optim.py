#!/usr/bin/env python3
"""Time per call of dvg_optim_step under every rule at the arena sizes of the two model families (GPU only, device events,
rounds interleaved in one process), with dvg_adam_step over the same range as the yardstick: a streaming kernel of the same build
on the same box.

  adam            dvg_adam_step                                       28 n bytes (p, m, v read and written, g read)
  rule0           dvg_optim_step rule 0, no mask                      28 n
  rule0_mask      the same with a decay mask                          28 n + n / 16
  adamw_mask      rule 1 with a decay mask                            28 n + n / 16
  sgd             rule 2, momentum 0.9                                20 n (p, m read and written, g read)
  sgd_plain       rule 2, no momentum                                 12 n
  rmsprop         rule 3, no momentum                                 20 n (p, v read and written, g read)
  rmsprop_mom     rule 3, momentum 0.9                                28 n

Every leg is timed cold - 1 GB of other traffic goes through the caches before each call - and warm, back to back.  Per leg the
line lists (median, min, max) ms of every round; `*_over_adam` divides the SMALLEST of a leg's round medians by adam's."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_gradguard import MODELS, arena_floats, timed  # noqa: E402
from dvg_amd import ops  # noqa: E402

BYTES = {"adam": 28.0, "rule0": 28.0, "rule0_mask": 28.0625, "adamw_mask": 28.0625, "sgd": 20.0, "sgd_plain": 12.0, "rmsprop": 20.0,
         "rmsprop_mom": 28.0}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    for model in MODELS:
        n = arena_floats(model)
        torch.manual_seed(1)
        p, g, m = (torch.randn(n, device=dev) * 1e-2 for _ in range(3))
        v = torch.rand(n, device=dev) * 1e-4
        mask = (torch.rand((n + 3) // 4, device=dev) < 0.9).to(torch.uint8)       # most of an arena is weight matrices
        trash = torch.empty(1 << 28, device=dev)                # 1 GB: more than the 256 MB Infinity Cache

        def rule(r, a_, b_, wd, mk):
            return lambda: ops.optim_step(r, p, g, m, None if r == ops.SGD else v, 2e-5, a_, b_, 1e-8, wd, 0, mk, 10, None)
        legs = {"adam": lambda: ops.adam_step(p, g, m, v, 2e-5, 0.9, 0.999, 1e-8, 0.0, 10, None),
                "rule0": rule(ops.ADAM, 0.9, 0.999, 0.0, None), "rule0_mask": rule(ops.ADAM, 0.9, 0.999, 0.01, mask),
                "adamw_mask": rule(ops.ADAMW, 0.9, 0.999, 0.01, mask), "sgd": rule(ops.SGD, 0.9, 0.0, 0.0, None),
                "sgd_plain": rule(ops.SGD, 0.0, 0.0, 0.0, None), "rmsprop": rule(ops.RMSPROP, 0.99, 0.0, 0.0, None),
                "rmsprop_mom": rule(ops.RMSPROP, 0.99, 0.9, 0.0, None)}
        for fn in legs.values():                                 # warm-up: code objects loaded, allocator settled
            trash.zero_()
            fn()
        res = {(k, how): [] for k in legs for how in ("cold", "warm")}
        for _ in range(a.rounds):                                # interleaved rounds
            for k, fn in legs.items():
                res[k, "cold"].append(timed(fn, a.iters, trash.zero_))
                res[k, "warm"].append(timed(fn, a.iters))
        best = {key: min(r[0] for r in rounds) for key, rounds in res.items()}
        out = {"model": model, "arena_floats": n, "arena_MB": round(4e-6 * n, 1)}
        for how in ("cold", "warm"):
            for k in legs:
                out[f"{k}_{how}_ms_median_min_max"] = [[round(x, 5) for x in r] for r in res[k, how]]
            for k in legs:
                out[f"{k}_{how}_TBps"] = round(BYTES[k] * n / best[k, how] / 1e9, 2)
                if k != "adam":
                    out[f"{k}_{how}_over_adam"] = round(best[k, how] / best["adam", how], 3)
        assert bool(torch.isfinite(p).all())
        print(json.dumps(out), flush=True)
        del p, g, m, v, mask, trash


if __name__ == "__main__":
    main()
