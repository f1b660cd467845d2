#!/usr/bin/env python3
"""Time per call of the weight average's kernel at the arena sizes of the two model families (GPU only, device events, rounds
interleaved in one process):

  ema_cold   dvg_ema_update after 1 GB of other traffic has gone through the caches
  ema_warm   the same right after dvg_adam_step has written the parameters: what the end of an iteration sees
  adam       dvg_adam_step over the same range - the yardstick: a streaming kernel of the same build on the same box

dvg_ema_update moves 12 n bytes (p and e read, e written), the Adam step 28 n (p, m, v read and written, g read).  Per leg the line
lists (median, min, max) ms of every round; the derived figures (`*_fraction_of_8TBps`, `*_TBps`, `ema_over_adam_byte_rate`) use
the SMALLEST of a leg's round medians."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_gradguard import HBM_BYTES_PER_S, MODELS, arena_floats, timed  # noqa: E402
from dvg_amd import ops  # noqa: E402
from dvg_amd._lib import check, lib  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--decay", type=float, default=0.999)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    for model in MODELS:
        n = arena_floats(model)
        torch.manual_seed(1)
        p, g, m, e = (torch.randn(n, device=dev) * 1e-2 for _ in range(4))
        v = torch.rand(n, device=dev) * 1e-4
        trash = torch.empty(1 << 28, device=dev)                # 1 GB: more than the 256 MB Infinity Cache
        nb = ops.ema_update_blocks(n)
        part = torch.zeros(2 * nb, dtype=torch.float64, device=dev)
        updates = torch.full((1,), 100000, dtype=torch.int32, device=dev)      # past the warm-up: the weight is 1 - decay
        hyper = (2e-3, 0.9, 0.999, 1e-8, 0.0)

        def ema():
            ops.ema_update(e, p, a.decay, updates, part)

        def adam():
            check(lib().dvg_adam_step(ops._p(p), ops._p(g), ops._p(m), ops._p(v), n, *hyper, 10, None, ops._stream()), "adam")
        legs = {"ema_cold": (ema, trash.zero_), "ema_warm": (ema, adam), "adam": (adam, None)}
        for fn, before in legs.values():                         # warm-up: code objects loaded, allocator settled
            before and before()
            fn()
        res = {k: [] for k in legs}
        for _ in range(a.rounds):                                # interleaved rounds
            for k, (fn, before) in legs.items():
                res[k].append(timed(fn, a.iters, before))
        floor_ms = 12.0 * n / HBM_BYTES_PER_S * 1e3
        best = {k: min(r[0] for r in v_) for k, v_ in res.items()}
        rate = {k: (28.0 if k == "adam" else 12.0) * n / best[k] / 1e9 for k in best}      # TB/s
        s = part.view(-1, 2).sum(0).tolist()
        print(json.dumps({"model": model, "arena_floats": n, "arena_MB": round(4e-6 * n, 1), "partial_pairs": nb,
                          "ema_floor_ms_at_8TBps": round(floor_ms, 5),
                          **{k + "_ms_median_min_max": [[round(x, 5) for x in r] for r in v_] for k, v_ in res.items()},
                          "ema_cold_fraction_of_8TBps": round(floor_ms / best["ema_cold"], 3),
                          "ema_warm_fraction_of_8TBps": round(floor_ms / best["ema_warm"], 3),
                          "ema_cold_TBps": round(rate["ema_cold"], 2), "ema_warm_TBps": round(rate["ema_warm"], 2),
                          "adam_TBps": round(rate["adam"], 2),
                          "ema_over_adam_byte_rate": [round(rate["ema_cold"] / rate["adam"], 3),
                                                      round(rate["ema_warm"] / rate["adam"], 3)],
                          "lag": (s[0] / s[1]) ** 0.5}), flush=True)
        del p, g, m, v, e, trash


if __name__ == "__main__":
    main()
