#!/usr/bin/env python3
"""Writes tests/golden/reference_clips.npz: what the REFERENCE's own data/kth.py, data/ucf.py and data/bair.py return on the
tiny tree of tests/clip_tree.py.

Run in the build container only (needs the reference tree and Pillow, CPU is enough):

    python tests/golden/make_golden_clips.py [path of the reference, default: the one make_golden.py uses]

The loaders import `scipy.misc` for imread / imresize, which scipy no longer has: a stand-in module whose imread is
np.array(PIL.Image.open(f)) is installed BEFORE the import (the stub_missing pattern of make_golden_viz.py).  os.listdir is
wrapped in sorted() while they run: bair.py lists its directories in file-system order, dvg_amd/datasets.py sorted.  Each
loader is seeded through its first __getitem__(SEED), as a DataLoader worker does.

Per dataset and split, for DRAWS consecutive draws at T = 8: the label (-1: bair returns none) and the CRC32 of the clip as
float32 bytes in (T,H,W,C) order; plus the whole float32 clip of draw 0.  Recorded results only: data, never reference source."""
import importlib.util
import os
import sys
import tempfile
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"          # as in make_golden.py

TREE_SEED, SEED, T, DRAWS = 0, 1234, 8, 40


def stub_scipy_misc():
    from PIL import Image
    m = types.ModuleType("scipy.misc")
    m.imread = lambda f: np.array(Image.open(f))
    m.imresize = lambda *a, **k: None            # imported by bair.py, never called
    sys.modules["scipy.misc"] = m
    import scipy
    scipy.misc = m


def reference_module(ref, name):
    spec = importlib.util.spec_from_file_location("reference_data_" + name, os.path.join(ref, "data", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record(ds, has_label):
    labels, crcs, clip0 = [], [], None
    for k in range(DRAWS):
        item = ds[SEED if k == 0 else k]         # only the first index seeds (kth.py:58-62, bair.py:34-37)
        x, y = item if has_label else (item, -1)
        x = np.asarray(x, dtype=np.float64).astype(np.float32)
        assert x.shape[:3] == (T, 64, 64), x.shape
        labels.append(int(y))
        crcs.append(zlib.crc32(np.ascontiguousarray(x).tobytes()))
        clip0 = x if k == 0 else clip0
    return np.array(labels, np.int64), np.array(crcs, np.uint32), clip0


def main():
    from tests import clip_tree
    ref = sys.argv[1] if len(sys.argv) > 1 else REF
    stub_scipy_misc()
    kth, ucf, bair = (reference_module(ref, n) for n in ("kth", "ucf", "bair"))
    out = {"tree_seed": np.int64(TREE_SEED), "seed": np.int64(SEED), "T": np.int64(T)}
    listdir = os.listdir
    with tempfile.TemporaryDirectory() as tmp:
        clip_tree.build(tmp, TREE_SEED)
        os.listdir = lambda p: sorted(listdir(p))
        try:
            for train in (True, False):
                split = "train" if train else "test"
                sets = {"kth": (kth.KTH(train, clip_tree.data_root(tmp, "kth"), seq_len=T, image_size=64), True),
                        "ucf": (ucf.UCF(train, clip_tree.data_root(tmp, "ucf"), seq_len=T, image_size=64), True),
                        "bair": (bair.RobotPush(clip_tree.data_root(tmp, "bair"), train=train, seq_len=T, image_size=64), False)}
                for name, (ds, has_label) in sets.items():
                    labels, crcs, clip0 = record(ds, has_label)
                    out[f"{name}/{split}/labels"], out[f"{name}/{split}/crc"], out[f"{name}/{split}/clip0"] = labels, crcs, clip0
        finally:
            os.listdir = listdir
    path = os.path.join(HERE, "reference_clips.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
