#!/usr/bin/env python3
"""Time per call of the gradient guard's kernels at the arena sizes of the two model families (GPU only, device events, rounds
interleaved in one process):

  sumsq_cold   dvg_grad_sumsq + dvg_grad_guard_finish after 1 GB of other traffic has gone through the caches
  sumsq_warm   the same right after a kernel that wrote the range (dvg_zero_tick + a copy into it): what a step site sees
  adam         dvg_adam_step over the range
  adam_guarded dvg_adam_step_guarded over the same buffers (clip factor 1, no skip)

The floor quoted for the reduction is its 4 n bytes at 8 TB/s (HBM3E peak); the Adam steps move 28 n bytes (p, m, v read and
written, g read).  Per leg the line lists (median, min, max) ms of every round; the derived figures (`*_fraction_of_8TBps`,
`adam_guarded_over_adam`, `adam_TBps`) use the SMALLEST of a leg's round medians."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvg_amd import ops  # noqa: E402
from dvg_amd._lib import check, lib  # noqa: E402
from dvg_amd.optim import GradGuard  # noqa: E402

HBM_BYTES_PER_S = 8e12
MODELS = ("dcgan_64", "vgg_64")


def arena_floats(model):
    """The Trainer's arena size for a family, from the modules (no training state is built)."""
    import importlib
    import train  # noqa: F401  (puts models/ on the path the way train.py does)
    from dvg_amd.models.gp_models import GaussianLikelihood, GPRegressionLayer1
    from dvg_amd.optim import FlatArena
    import models.lstm as lstm_models
    m = importlib.import_module(f"models.{model}")
    mods = [m.encoder(90, 1), m.decoder(90, 1), lstm_models.lstm(90, 90, 256, 2, 4), GPRegressionLayer1(num_dims=90),
            GaussianLikelihood(batch_size=90)]
    return FlatArena.size_for([p for mod in mods for p in mod.parameters()])


def timed(fn, iters, before=None):
    """(median, min, max) ms per call over `iters` calls, each bracketed by its own events; `before()` runs untimed ahead of
    every call."""
    evs = []
    for _ in range(iters):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in evs)
    return ms[len(ms) // 2], ms[0], ms[-1]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    for model in MODELS:
        n = arena_floats(model)
        torch.manual_seed(1)
        p, g, m = (torch.randn(n, device=dev) * 1e-2 for _ in range(3))
        v = torch.rand(n, device=dev) * 1e-4
        src = torch.randn(n, device=dev) * 1e-2
        trash = torch.empty(1 << 28, device=dev)                # 1 GB: more than the 256 MB Infinity Cache
        guard = GradGuard(1e30, True, dev)
        nb = ops.grad_sumsq_blocks(n)
        part = guard.reserve(nb)
        skips = torch.zeros(1, dtype=torch.int32, device=dev)
        hyper = (2e-3, 0.9, 0.999, 1e-8, 0.0)

        def norm():
            ops.grad_sumsq(g, part)
            ops.grad_guard_finish(part, nb, guard.max_norm, True, guard.stat, guard.counters)

        def write_range():
            check(lib().dvg_zero_tick(ops._p(g), n, None, None, None, None, ops._stream()), "dvg_zero_tick")
            g.copy_(src)

        def adam():
            check(lib().dvg_adam_step(ops._p(p), ops._p(g), ops._p(m), ops._p(v), n, *hyper, 10, None, ops._stream()), "adam")

        def adam_guarded():
            ops.adam_step_guarded(p, g, m, v, *hyper, 10, None, guard.stat, skips)
        legs = {"sumsq_cold": (norm, trash.zero_), "sumsq_warm": (norm, write_range), "adam": (adam, None),
                "adam_guarded": (adam_guarded, None)}
        for fn, before in legs.values():                         # warm-up: code objects loaded, allocator settled
            before and before()
            fn()
        res = {k: [] for k in legs}
        for _ in range(a.rounds):                                # interleaved rounds
            for k, (fn, before) in legs.items():
                res[k].append(timed(fn, a.iters, before))
        floor_ms = 4.0 * n / HBM_BYTES_PER_S * 1e3
        best = {k: min(r[0] for r in v_) for k, v_ in res.items()}
        print(json.dumps({"model": model, "arena_floats": n, "arena_MB": round(4e-6 * n, 1), "partials": nb,
                          "sumsq_floor_ms_at_8TBps": round(floor_ms, 5),
                          **{k + "_ms_median_min_max": [[round(x, 5) for x in r] for r in v_] for k, v_ in res.items()},
                          "sumsq_cold_fraction_of_8TBps": round(floor_ms / best["sumsq_cold"], 3),
                          "sumsq_warm_fraction_of_8TBps": round(floor_ms / best["sumsq_warm"], 3),
                          "adam_guarded_over_adam": round(best["adam_guarded"] / best["adam"], 4),
                          "adam_TBps": round(28.0 * n / best["adam"] / 1e9, 2),
                          "norm": float(guard.stat[0]), "skips": int(skips)}), flush=True)
        del p, g, m, v, src, trash


if __name__ == "__main__":
    main()
