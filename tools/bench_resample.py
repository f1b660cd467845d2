#!/usr/bin/env python3
"""`--resize` in numbers (GPU only): dvg_resample_u8 alone, the host design it replaces, and the build of a frame pool with and
without it.

    python tools/bench_resample.py [--rounds 7] [--iters 20] [--frames 4096] [--clips 32]

Recorded values, not pass bars (docs/DESIGN_NOTES_frames.md holds the table).
  kernel  ops.resample_u8 over `frames` frames of 240 x 320 x 3 and of 120 x 160 x 1 -> 64 x 64, bilinear and bicubic, the crop
          box: the event time of `iters` back-to-back calls after a warm-up, per round; the median and the spread over the
          rounds, the bytes moved (src + dst) and their rate as a fraction of the HBM peak.
  pillow  the same frames through Image.resize on 16 host threads (wall time; 3 rounds): what the converters' scaling costs.
  pool    datasets.build_pool of a synthetic `frames` tree (`clips` clips of 16 PNG frames, 240 x 320 RGB) with
          --resize bilinear, against the same tree scaled to 64 x 64 beforehand and built without the flag; and the share of
          the resized build that is PNG decoding on the host (the same decode loop without upload or kernel)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dvg_amd import datasets, ops, resample  # noqa: E402

HBM_BYTES_PER_S = 8e12
SHAPES = ((240, 320, 3), (120, 160, 1))
FILTERS = ("bilinear", "bicubic")
S = 64


def event_us(fn, iters):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def spread(v, digits=1):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def kernel_leg(dev, frames, rounds, iters):
    rows = []
    for H, W, C in SHAPES:
        src = torch.randint(0, 256, (frames, H, W, C), dtype=torch.uint8, device=dev)
        out = torch.empty((frames, S, S, C), dtype=torch.uint8, device=dev)
        box = resample.fit_box(W, H, S, S, "crop")
        forms = {f: (lambda f=f: ops.resample_u8(src, (S, S), f, box=box, out=out)) for f in FILTERS}
        for fn in forms.values():
            event_us(fn, 3)                                                  # warm-up: tables uploaded, clocks up
        us = {f: [] for f in forms}
        for _ in range(rounds):                                              # interleaved
            for f, fn in forms.items():
                us[f].append(event_us(fn, iters))
        host = src.cpu().numpy()
        pil = {f: [] for f in forms}
        with ThreadPoolExecutor(16) as ex:
            for f in forms:
                flt = resample.pil_filter(f)

                def one(a, flt=flt):
                    return Image.fromarray(a[:, :, 0] if C == 1 else a).resize((S, S), flt, box=box)
                for _ in range(3):
                    t0 = time.perf_counter()
                    res = list(ex.map(one, host))
                    pil[f].append((time.perf_counter() - t0) * 1e3)
                got = forms[f]()[:8].cpu().numpy()                           # the two designs agree on what they time
                assert np.array_equal(got, np.stack([np.asarray(r).reshape(S, S, C) for r in res[:8]]))
        moved = src.numel() + out.numel()
        for f in forms:
            med = statistics.median(us[f])
            rows.append({"frames": frames, "H": H, "W": W, "C": C, "filter": f, "band_span": ops.resample_band(H, W, S, S, C, f, box),
                         "MB": round(moved / 1e6, 1), "kernel_us": spread(us[f]),
                         "GB_per_s": round(moved / (med * 1e-6) / 1e9, 1), "of_hbm_peak": round(moved / (med * 1e-6) / HBM_BYTES_PER_S, 4),
                         "pillow_16_threads_ms": spread(pil[f]), "pillow_over_kernel": round(statistics.median(pil[f]) * 1e3 / med, 1)})
        del src, out
    return rows


def write_tree(root, clips, hw):
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(0)
    for c in range(clips):
        d = os.path.join(root, "train", "clip%03d" % c)
        os.makedirs(d)
        for k in range(16):
            base = 127.5 + 100.0 * np.sin((xx + 3 * k + 7 * c) / 9.0) * np.cos((yy - 2 * k) / 7.0)
            img = np.clip(base[..., None] + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(d, "%d.png" % k))


def pool_leg(dev, tmp, clips, rounds):
    native, small = os.path.join(tmp, "native"), os.path.join(tmp, "small")
    write_tree(native, clips, (240, 320))
    idx = datasets.open_index("frames", native, True)
    for seq in idx.sequences:                                                # the converter's output: the same frames at 64 x 64
        for f in seq:
            dst = f.replace(native, small)
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            with Image.open(f) as im:
                resample.pil_resize(im, S, "bilinear", "crop").save(dst)
    idx_small = datasets.open_index("frames", small, True)
    files = [f for seq in idx.sequences for f in seq]

    def decode_only():
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(lambda f: np.asarray(Image.open(f)), files))
    forms = {"resize_bilinear_gpu": lambda: datasets.build_pool(idx, S, dev, 16, ("bilinear", "crop")),
             "prescaled_no_resize_gpu": lambda: datasets.build_pool(idx_small, S, dev, 16),
             "resize_bilinear_host_pillow": lambda: datasets.build_pool(idx, S, None, 16, ("bilinear", "crop")),
             "decode_only_native_size": decode_only}
    assert torch.equal(forms["resize_bilinear_gpu"]().cpu(), forms["resize_bilinear_host_pillow"]())
    ms = {k: [] for k in forms}
    for _ in range(rounds):                                                  # interleaved; the files are in the page cache by now
        for k, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {"frames": len(files), "native": "240x320x3 PNG", "threads": 16, "ms": {k: spread(v) for k, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--clips", type=int, default=32)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resample.py needs a GPU"
    dev = torch.device("cuda:0")
    out = {"kernel": kernel_leg(dev, a.frames, a.rounds, a.iters)}
    with tempfile.TemporaryDirectory() as tmp:
        out["pool"] = pool_leg(dev, tmp, a.clips, a.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
