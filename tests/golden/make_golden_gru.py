#!/usr/bin/env python3
"""Generate tests/golden/reference_gru.npz and reference_pickled_gru.pth.gz by RUNNING THE REFERENCE's own `gru` and `rnn`
modules (models/lstm.py:75-136), imported unmodified through make_golden.ref_import with the same `torch.Tensor.cuda` shim
(lstm.py:94,126 hard-call `.cuda()`).  Run where make_golden.py runs (CPU is enough):

    python tests/golden/make_golden_gru.py

Weights and inputs come from oracle/params.py seeds, so only the reference's OUTPUTS are stored: data, never reference source.
"""
import gzip
import io
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the repository root on sys.path)

from oracle import params  # noqa: E402

SHAPE = (90, 90, 64, 2)      # in, out, hidden, layers
B, STEPS = 5, 3
SEEDS = {"gru": 500, "rnn": 520}


def run(mod, out: dict):
    import dvg_amd.models.lstm as ours
    for cls, seed in SEEDS.items():
        net = getattr(mod, cls)(*SHAPE, B)
        assert list(getattr(ours, cls)(*SHAPE, B).state_dict().keys()) == list(net.state_dict().keys()), cls
        net.load_state_dict(params.fill_state_dict(net.state_dict(), seed))
        net.hidden = net.init_hidden()
        with torch.no_grad():
            ys = [net(params.normal(seed + 10 + t, B, 90, scale=0.5)).numpy() for t in range(STEPS)]
        out[f"{cls}/y"] = np.stack(ys)
        for i in range(SHAPE[3]):
            out[f"{cls}/h{i}"] = net.hidden[i].detach().numpy()
        # 3-step BPTT: loss = sum_t sum(y_t * G_t), the reference's own .backward()
        net.zero_grad()
        net.hidden = net.init_hidden()
        xs = [params.normal(seed + 10 + t, B, 90, scale=0.5).requires_grad_(True) for t in range(STEPS)]
        loss = sum((net(xs[t]) * params.normal(seed + 15 + t, B, 90)).sum() for t in range(STEPS))
        loss.backward()
        out[f"{cls}_grad/loss"] = np.array([float(loss)])
        for k, p_ in net.named_parameters():
            out[f"{cls}_grad/{k}"] = mg.summarize(p_.grad)
        for t in range(STEPS):
            out[f"{cls}_grad/x{t}"] = xs[t].grad.numpy()
        print(f"{cls}: y std {np.stack(ys).std():.4f} loss {float(loss):.6f}")


def write_pickles(mod):
    """The reference's own gru / rnn objects pickled WHOLE by class path `models.lstm.<class>` (train.py:380-388 stores the
    frame predictor that way), every tensor zeroed so that the file is a few KB, beside their state_dict key lists."""
    fixture = {}
    for cls in SEEDS:
        net = getattr(mod, cls)(*SHAPE, B)
        with torch.no_grad():
            for t in net.parameters():
                t.zero_()
            net.hidden = net.init_hidden()
        fixture[cls] = {"module": net, "keys": list(net.state_dict().keys()), "shape": SHAPE, "batch": B}
    saved = {k: v for k, v in sys.modules.items() if k == "models" or k.startswith("models.")}
    for k in saved:
        del sys.modules[k]
    pkg = types.ModuleType("models")
    pkg.__path__ = [os.path.join(mg.REF, "models")]
    sys.modules.update({"models": pkg, "models.lstm": mod})
    try:
        buf = io.BytesIO()
        torch.save(fixture, buf)
    finally:
        for k in ("models", "models.lstm"):
            sys.modules.pop(k, None)
        sys.modules.update(saved)
    path = os.path.join(HERE, "reference_pickled_gru.pth.gz")
    with gzip.GzipFile(path, "wb", compresslevel=9, mtime=0) as f:
        f.write(buf.getvalue())
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self  # harness-only shim for lstm.py:94,126
    mod = mg.ref_import("lstm")
    out = OrderedDict()
    run(mod, out)
    path = os.path.join(HERE, "reference_gru.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")
    write_pickles(mod)


if __name__ == "__main__":
    main()
