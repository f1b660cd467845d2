#!/usr/bin/env python3
"""The GRU predictor's kernels beside their LSTM counterparts, same box, same process, rounds interleaved (GPU only):

  cell      dvg_gru_cell / dvg_rnn_cell against dvg_lstm_cell at B = 64, H = 256, device events per call
  sequence  the teacher-forced S = 19 sequence of a 2-layer (90, 90, 256) predictor, forward and backward, each as ONE hipGraph
            replay (what a captured training iteration pays: kernel time, no launch overhead) and eager (launch-bound)
  train     one train.py iteration (dcgan_64, B = 64, T = 20) as a hipGraph replay, --predictor gru against lstm (--no_train skips it)

Bytes a cell must move (weights once + x, h (c) in + state out, fp32): lstm 8 H^2 + 5 B H, gru 6 H^2 + 3 B H, rnn 2 H^2 + 3 B H floats.
One JSON line per leg; figures are (median, min, max) per round, the derived ratios use the smallest round median."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_gradguard import timed  # noqa: E402
from dvg_amd import ops  # noqa: E402


def cell_leg(a):
    dev = torch.device("cuda:0")
    B, H = a.batch, a.hidden
    torch.manual_seed(1)
    x, h, c = (torch.randn(B, H, device=dev) * 0.5 for _ in range(3))
    w = {g: [torch.randn(g * H, H, device=dev) * H ** -0.5 for _ in range(2)] + [torch.randn(g * H, device=dev) * 0.1 for _ in range(2)]
         for g in (1, 3, 4)}
    legs = {"lstm_cell": lambda: ops.lstm_cell(x, h, c, *w[4]), "gru_cell": lambda: ops.gru_cell(x, h, *w[3]),
            "rnn_cell": lambda: ops.rnn_cell(x, h, *w[1]), "lstm_cell_b": lambda: ops.lstm_cell(x, h, c, *w[4])}
    floats = {"lstm_cell": 8 * H * H + 5 * B * H, "gru_cell": 6 * H * H + 3 * B * H, "rnn_cell": 2 * H * H + 3 * B * H}
    floats["lstm_cell_b"] = floats["lstm_cell"]
    for fn in legs.values():
        for _ in range(5):
            fn()
    res = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            res[k].append(timed(fn, a.iters))
    best = {k: min(r[0] for r in v) for k, v in res.items()}
    print(json.dumps({"leg": "cell", "B": B, "H": H, "timing": "device events per call, eager launches",
                      **{k + "_us_median_min_max": [[round(1e3 * t, 2) for t in r] for r in v] for k, v in res.items()},
                      **{k + "_us": round(1e3 * v, 2) for k, v in best.items()},
                      **{k + "_MB": round(4e-6 * v, 3) for k, v in floats.items()},
                      "gru_over_lstm_time": round(best["gru_cell"] / best["lstm_cell"], 3),
                      "gru_over_lstm_bytes": round(floats["gru_cell"] / floats["lstm_cell"], 3),
                      "lstm_b_over_lstm_time": round(best["lstm_cell_b"] / best["lstm_cell"], 3)}), flush=True)


def sequence_leg(a):
    import dvg_amd.models.lstm as models
    from dvg_amd import graphs
    dev = torch.device("cuda:0")
    B, S, H = a.batch, a.steps, a.hidden
    out = {"leg": "sequence", "B": B, "S": S, "H": H, "layers": 2}
    runs = {}
    for kind in ("lstm", "gru"):
        torch.manual_seed(1)
        net = models.PREDICTORS[kind](90, 90, H, 2, B).to(dev)
        xs = (torch.randn(S, B, 90, device=dev) * 0.5).requires_grad_(True)
        ws = torch.randn(S, B, 90, device=dev)
        assert models.sequence_applies(net)

        def fwd(net=net, xs=xs):
            return models.forward_sequence(net, xs)

        def fwd_bwd(net=net, xs=xs, ws=ws):
            y = models.forward_sequence(net, xs)
            y.backward(ws)
            return y
        for _ in range(3):
            fwd_bwd()
        runs[kind] = (fwd, fwd_bwd)
    graphed = {}
    for kind, (fwd, fwd_bwd) in runs.items():
        for name, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
            graphs.warm_up(fn, 2)
            g, _, keep = graphs.capture(fn)
            graphed[f"{kind}_{name}"] = (g, keep)
    legs = {f"{k}_graph": v[0].replay for k, v in graphed.items()}
    legs.update({f"{kind}_{name}_eager": fn for kind, fns in runs.items() for name, fn in zip(("fwd", "fwd_bwd"), fns)})
    res = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            res[k].append(timed(fn, a.iters))
    best = {k: min(r[0] for r in v) for k, v in res.items()}
    out.update({k + "_us_median_min_max": [[round(1e3 * t, 1) for t in r] for r in v] for k, v in res.items()})
    out.update({k + "_us": round(1e3 * v, 1) for k, v in best.items()})
    for form in ("graph", "eager"):
        for kind in ("lstm", "gru"):
            out[f"{kind}_bwd_{form}_us"] = round(1e3 * (best[f"{kind}_fwd_bwd_{form}"] - best[f"{kind}_fwd_{form}"]), 1)
        out[f"gru_over_lstm_fwd_{form}"] = round(best[f"gru_fwd_{form}"] / best[f"lstm_fwd_{form}"], 3)
        out[f"gru_over_lstm_fwd_bwd_{form}"] = round(best[f"gru_fwd_bwd_{form}"] / best[f"lstm_fwd_bwd_{form}"], 3)
    # launches per sequence (forward: embed, head, per layer 1 input-half GEMM + S cells; backward per step and layer: lstm 1, gru 2)
    out["launches_fwd"] = {"lstm": 2 + 2 * (1 + S) + 2, "gru": 2 + 2 * (1 + S) + 4}
    out["launches_bwd_recurrence"] = {"lstm": 2 * S, "gru": 2 * (2 * S - 1)}
    print(json.dumps(out), flush=True)


def train_leg(a):
    import train
    import utils
    from dvg_amd.data import SyntheticMovingMNIST
    legs = {}
    for name, extra in (("lstm", []), ("gru", ["--predictor", "gru"]), ("lstm_b", [])):
        o = train.options(["--model", "dcgan", "--batch_size", str(a.batch), "--n_past", "10", "--n_future", "10", "--no_save"] + extra)
        torch.manual_seed(1)
        tr = train.Trainer(o, torch.device("cuda:0"))
        tr.train_mode()
        x, _ = utils.normalize_data(o, torch.cuda.FloatTensor, SyntheticMovingMNIST(seq_len=20, seed=1).batch(a.batch))
        step = train.GraphedIteration(tr, warmup=2)
        for _ in range(4):
            step(x)
        assert step.graph is not None and not step.failed, "the iteration was not captured"
        legs[name] = (tr, step, x)
    res = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, (_, step, x) in legs.items():
            ms = []
            for _ in range(a.train_iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step(x)                    # replays and reads the losses back: synchronous
                ms.append((time.perf_counter() - t0) * 1e3)
            res[k].append(statistics.median(ms))
    med = {k: statistics.median(v) for k, v in res.items()}
    print(json.dumps({"leg": "train", "model": "dcgan_64", "batch": a.batch, "T": 20, "launch": "hipGraph replay",
                      **{k + "_ms_round_medians": [round(v, 3) for v in r] for k, r in res.items()},
                      **{k + "_ms": round(v, 3) for k, v in med.items()},
                      "gru_minus_lstm_ms": round(med["gru"] - med["lstm"], 3),
                      "lstm_b_minus_lstm_ms": round(med["lstm_b"] - med["lstm"], 3),
                      "predictor_params": {k: sum(p.numel() for p in legs[k][0].frame_predictor.parameters()) for k in ("lstm", "gru")}}),
          flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--train_iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--steps", type=int, default=19)
    ap.add_argument("--no_train", action="store_true")
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_gru.py needs a GPU"
    cell_leg(a)
    sequence_leg(a)
    if not a.no_train:
        train_leg(a)


if __name__ == "__main__":
    main()
