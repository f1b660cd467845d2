#!/usr/bin/env python3
"""Per-call time of the GP kernels by covariance family (--gp_kernel) at the shapes of tools/bench_gp.py: train-mode predict +
KL, eval-mode predict + sample and the backward at B = 64, and the time-batched closure shape C4 (B = 16, S = 11 steps side by
side).  The kinds alternate inside one process - round after round, `rbf` timed TWICE per round, so the spread between two
timings of the same kernel (A against A) stands beside every difference between kinds.  GPU only.

    python tools/bench_gp_kernels.py [--rounds 5] [--iters 100]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvg_amd import ops  # noqa: E402
from oracle import params  # noqa: E402
from tools.bench_small import time_fn  # noqa: E402


def cases(dev):
    """name -> (callable of the kernel name) for every timed launch."""
    D, M = 90, 40
    gsd, _ = params.gp_state(3, D, M)
    g = {k: v.to(dev) for k, v in gsd.items()}
    z = g["variational_strategy.inducing_points"]
    m = g["variational_strategy.variational_distribution.variational_mean"]
    ls = g["variational_strategy.variational_distribution.chol_variational_covar"]
    s = F.softplus(g["covar_module.raw_outputscale"]).reshape(-1)
    ell = F.softplus(g["covar_module.base_kernel.raw_lengthscale"]).reshape(-1)
    c = g["mean_module.constant"].reshape(-1)
    par = (z, m, ls, c, s, ell)
    gen = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda *shape: torch.randn(*shape, device=dev, generator=gen)     # noqa: E731
    out = {}
    B = 64
    h, gm, gv, gk, eps = torch.tanh(rnd(B, D)), rnd(D, B), rnd(D, B), rnd(D), rnd(D, B)
    out["B=64 predict(train, KL)"] = lambda k: ops.gp_predict(h, *par, train_mode=True, want_kl=True, kernel=k)
    out["B=64 predict(eval, sample)"] = lambda k: ops.gp_predict(h, *par, noise=s, eps=eps, kernel=k)
    out["B=64 train_bwd"] = lambda k: ops.gp_train_bwd(h, *par, gm, gv, gk, kernel=k)
    B, S = 16, 11
    grp = ops.gp_step_group(B, S, D, M)
    hs, gms, gvs, gks = torch.tanh(rnd(B, S * D)), rnd(S * D, B), rnd(S * D, B), rnd(S * D)
    out[f"C4 B=16 S=11 k={grp} predict(train, KL)"] = lambda k: ops.gp_predict(hs, *par, train_mode=True, want_kl=True, param_period=D,
                                                                              step_group=grp, kernel=k)
    out[f"C4 B=16 S=11 k={grp} train_bwd"] = lambda k: ops.gp_train_bwd(hs, *par, gms, gvs, gks, param_period=D, step_group=grp,
                                                                       kernel=k)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--kernel", action="append", choices=tuple(ops.GP_KERNELS), help="kinds to time (default: all); rbf always runs")
    args = ap.parse_args()
    kinds = ["rbf"] + [k for k in (args.kernel or list(ops.GP_KERNELS)) if k != "rbf"]
    order = kinds + ["rbf"]          # rbf first AND last in every round: A against A
    dev = torch.device("cuda:0")
    print(f"us per launch, median of {args.rounds} rounds x {args.iters} launches (min .. max); spread = |rbf - rbf again| / rbf")
    for name, call in cases(dev).items():
        t = {k: [] for k in kinds}
        again = []
        for _ in range(args.rounds):
            for pos, k in enumerate(order):
                us = time_fn(lambda: call(k), iters=args.iters, warm_s=0.05)
                (again if pos == len(order) - 1 else t[k]).append(us)
        base = statistics.median(t["rbf"])
        spread = max(abs(a - b) for a, b in zip(t["rbf"], again)) / base
        cols = [f"{k} {statistics.median(v):7.1f} ({min(v):.1f}..{max(v):.1f}, {statistics.median(v) / base - 1:+.1%})" for k, v in t.items()]
        print(f"{name:38s} " + "  ".join(cols) + f"  rbf again {statistics.median(again):7.1f}  spread {spread:.1%}")


if __name__ == "__main__":
    main()
