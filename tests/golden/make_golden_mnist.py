#!/usr/bin/env python3
"""Writes tests/golden/reference_mnist.npz: what the REFERENCE's own data/moving_mnist.py returns on the tiny MNIST tree of
tests/mnist_tree.py.

Run in the build container only (needs the reference tree and Pillow, CPU is enough):

    python tests/golden/make_golden_mnist.py [path of the reference, default: the one make_golden.py uses]

moving_mnist.py imports `torchvision` for the MNIST files and the transforms: a stand-in module is installed BEFORE the import
(the stub_scipy_misc pattern of make_golden_clips.py).  Its datasets.MNIST reads the tree's IDX files and returns
(transform(PIL 'L' image), 0); transforms.Scale(n) = img.resize((n, n), Image.BILINEAR), what torchvision's Scale did to a
square image; ToTensor = float().div(255)[None]; Compose chains them.  The dataset is seeded through its first
__getitem__(SEED), as a DataLoader worker does.

Per split and per (num_digits, image_size) in COMBOS, for DRAWS consecutive draws at T = 8 and deterministic=False
(utils.py:35,42): the CRC32 of the clip as float32 bytes in (T,H,W,1) order, plus the whole float32 clip of draw 0; and the
scaled digits of both splits as uint8, round(255 * tensor) of the stand-in's output.  Recorded results only: data, never
reference source."""
import gzip
import importlib.util
import os
import sys
import tempfile
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"          # as in make_golden.py

TREE_SEED, SEED, T, DRAWS = 0, 7920, 8, 40        # 7920: the test-split seed of a run with the default --seed 1 (1 + 7919)
COMBOS = ((2, 64), (3, 64), (2, 128))


def stub_torchvision():
    from PIL import Image
    from tests import mnist_tree

    class MNIST:
        def __init__(self, root, train=True, download=False, transform=None):
            raw = os.path.join(root, "MNIST", "raw", mnist_tree.NAMES[bool(train)])
            data = gzip.open(raw + ".gz", "rb").read() if os.path.exists(raw + ".gz") else open(raw, "rb").read()
            n = int.from_bytes(data[4:8], "big")
            self.images = np.frombuffer(data, np.uint8, offset=16).reshape(n, 28, 28)
            self.transform = transform

        def __len__(self):
            return len(self.images)

        def __getitem__(self, i):
            return self.transform(Image.fromarray(self.images[i])), 0

    class Scale:
        def __init__(self, n):
            self.n = n

        def __call__(self, img):
            return img.resize((self.n, self.n), Image.BILINEAR)

    class ToTensor:
        def __call__(self, img):
            return torch.from_numpy(np.array(img)).float().div(255)[None]

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    tv = types.ModuleType("torchvision")
    tv.datasets = types.ModuleType("torchvision.datasets")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.datasets.MNIST = MNIST
    tv.transforms.Scale, tv.transforms.ToTensor, tv.transforms.Compose = Scale, ToTensor, Compose
    sys.modules.update({"torchvision": tv, "torchvision.datasets": tv.datasets, "torchvision.transforms": tv.transforms})


def reference_module(ref):
    spec = importlib.util.spec_from_file_location("reference_data_moving_mnist", os.path.join(ref, "data", "moving_mnist.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def both_kinds_of_overlap(sprites, clip0, seed, num_digits, image_size):
    """Does clip 0 hold sums of two or more digits above 1 (clipped) AND below 1?  The unclipped sums come from the
    repository's restatement of the draws, which must give this very clip."""
    from dvg_amd import mnist
    ids, pos = mnist.MovingMnistSampler(len(sprites), T, num_digits, image_size, seed).draw(1)
    assert np.array_equal(mnist.compose_host(sprites, ids, pos, image_size)[0], clip0)
    f = sprites.astype(np.float32) / np.float32(255)
    total = np.zeros((T, image_size, image_size), np.float32)
    hits = np.zeros((T, image_size, image_size), np.int32)
    for n in range(num_digits):
        for t in range(T):
            sy, sx = pos[0, n, t]
            total[t, sy:sy + 32, sx:sx + 32] += f[ids[0, n]]
            hits[t, sy:sy + 32, sx:sx + 32] += f[ids[0, n]] > 0
    return bool(((hits >= 2) & (total > 1)).any()), bool(((hits >= 2) & (total < 1)).any())


def main():
    from tests import mnist_tree
    ref = sys.argv[1] if len(sys.argv) > 1 else REF
    stub_torchvision()
    mm = reference_module(ref)
    out = {"tree_seed": np.int64(TREE_SEED), "seed": np.int64(SEED), "T": np.int64(T),
           "combos": np.array(COMBOS, np.int64)}
    with tempfile.TemporaryDirectory() as tmp:
        mnist_tree.build(tmp, TREE_SEED)
        for train in (True, False):
            split = "train" if train else "test"
            for nd, size in COMBOS:
                ds = mm.MovingMNIST(train, tmp, seq_len=T, num_digits=nd, image_size=size, deterministic=False)
                crcs, clip0 = [], None
                for k in range(DRAWS):
                    x = ds[SEED if k == 0 else k]            # only the first index seeds (moving_mnist.py:30-33)
                    assert x.shape == (T, size, size, 1) and x.dtype == np.float32
                    crcs.append(zlib.crc32(np.ascontiguousarray(x).tobytes()))
                    clip0 = x.copy() if k == 0 else clip0
                out[f"{split}/{nd}x{size}/crc"], out[f"{split}/{nd}x{size}/clip0"] = np.array(crcs, np.uint32), clip0
            sprites = np.stack([ds.data[i][0][0].numpy() for i in range(len(ds.data))])
            u8 = np.round(sprites * 255).astype(np.uint8)
            assert np.array_equal(u8.astype(np.float32) / np.float32(255), sprites)
            out[f"{split}/sprites"] = u8
            kinds = [both_kinds_of_overlap(u8, out[f"{split}/{nd}x{size}/clip0"], SEED, nd, size) for nd, size in COMBOS]
            print(split, "clip 0 (saturated, unsaturated) overlap per combination:", kinds)
            assert any(k[0] for k in kinds) and any(k[1] for k in kinds), "clip 0 must show clipped and unclipped sums of digits"
    path = os.path.join(HERE, "reference_mnist.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
