"""A tiny deterministic MNIST tree: the two IDX image files that data/moving_mnist.py reads through torchvision, written at
test time.  Not a test: tests/test_mnist_host.py, tests/test_gpu_mnist.py and tests/golden/make_golden_mnist.py build it.

    <root>/MNIST/raw/train-images-idx3-ubyte.gz    48 digits, gzipped (torchvision's layout as downloaded)
    <root>/MNIST/raw/t10k-images-idx3-ubyte        24 digits, a raw file (as torchvision unpacks it)

A digit is 28x28 uint8: thick strokes with soft edges, so that two overlapping digits give sums above 1 (clipped) in their cores
and below 1 where their edges meet; every sixth digit is full-range noise instead, so that every byte value goes through the
resize and the division by 255.  No two digits are equal: a clip's CRC names its digits and its trajectory."""
import gzip
import os
import struct

import numpy as np

SIZE = 28
N_TRAIN, N_TEST = 48, 24
MAGIC = 0x00000803
NAMES = {True: 'train-images-idx3-ubyte', False: 't10k-images-idx3-ubyte'}


def digit(seed, train, i):
    rng = np.random.default_rng([seed, int(train), i])
    if i % 6 == 5:
        return rng.integers(0, 256, (SIZE, SIZE), dtype=np.uint8)
    yy, xx = np.mgrid[0:SIZE, 0:SIZE]
    img = np.zeros((SIZE, SIZE), np.float64)
    p = rng.uniform(5, SIZE - 5, 2)
    for _ in range(rng.integers(3, 6)):
        q = np.clip(p + rng.normal(0, 7, 2), 3, SIZE - 4)
        for t in np.linspace(0, 1, 20):
            c = p * (1 - t) + q * t
            img = np.maximum(img, np.exp(-((yy - c[0]) ** 2 + (xx - c[1]) ** 2) / (2 * 1.5 ** 2)))
        p = q
    return np.round(np.clip(img * 1.4, 0, 1) * 255).astype(np.uint8)


def images(seed, train):
    """(n, 28, 28) uint8: the digits of one split."""
    return np.stack([digit(seed, train, i) for i in range(N_TRAIN if train else N_TEST)])


def idx_bytes(imgs):
    n, h, w = imgs.shape
    return struct.pack('>IIII', MAGIC, n, h, w) + np.ascontiguousarray(imgs, np.uint8).tobytes()


def write(directory, train, imgs, gz):
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, NAMES[bool(train)] + ('.gz' if gz else ''))
    with (gzip.open(path, 'wb', compresslevel=1) if gz else open(path, 'wb')) as f:
        f.write(idx_bytes(imgs))
    return path


def build(root, seed=0):
    """Writes the tree under root (a --data_root) and returns root."""
    root = str(root)
    raw = os.path.join(root, 'MNIST', 'raw')
    write(raw, True, images(seed, True), gz=True)
    write(raw, False, images(seed, False), gz=False)
    return root
