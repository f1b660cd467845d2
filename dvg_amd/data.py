"""The input pipeline: synthetic stand-ins for the datasets of the reference, and `make_batch_generator`, which also serves
KTH / BAIR / UCF clips (dvg_amd/datasets.py) and Moving-MNIST over real MNIST digits (dvg_amd/mnist.py) from `--data_root`.

`SyntheticMovingMNIST` follows the trajectory logic of data/moving_mnist.py:38-91 exactly —
`num_digits` 32x32 sprites on a 64x64 canvas, start ~ randint(32), velocity ~ randint(-4,5),
the non-deterministic bounce rules (:56-84), additive compositing clipped at 1 (:90) — but the
sprites come from a seeded in-repo generator instead of MNIST.  Frames are (T,H,W,1) float32 in
[0,1]; a batch is (B,T,H,W,1), which `utils.normalize_data` turns into T x (B,1,H,W)."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

from . import datasets, mnist
from .utils import normalize_data


def _sprites(rng: np.random.Generator, n: int, size: int = 32) -> np.ndarray:
    """Digit-like blobs: a few thick random strokes, smoothed, values in [0,1]."""
    out = np.zeros((n, size, size), np.float32)
    yy, xx = np.mgrid[0:size, 0:size]
    for i in range(n):
        img = np.zeros((size, size), np.float32)
        p = rng.uniform(6, size - 6, 2)
        for _ in range(rng.integers(3, 6)):
            q = np.clip(p + rng.normal(0, 7, 2), 4, size - 5)
            for t in np.linspace(0, 1, 24):
                c = p * (1 - t) + q * t
                img = np.maximum(img, np.exp(-((yy - c[0]) ** 2 + (xx - c[1]) ** 2) / (2 * 1.6 ** 2)))
            p = q
        out[i] = np.clip(img * 1.3, 0, 1)
    return out


class SyntheticMovingMNIST:
    def __init__(self, seq_len=20, num_digits=2, image_size=64, seed=1, n_sprites=64, deterministic=False):
        self.seq_len, self.num_digits, self.image_size = seq_len, num_digits, image_size
        self.digit_size = 32
        self.deterministic = deterministic
        self.rng = np.random.default_rng(seed)
        self.data = _sprites(self.rng, n_sprites, self.digit_size)
        self.N = n_sprites

    def __len__(self):
        return 10000

    def position(self):
        """Where the trajectory stream stands (see BatchStream): the generator's state; the sprites are rebuilt from the seed."""
        return {"sampler": "SyntheticMovingMNIST", "rng": self.rng.bit_generator.state}

    def restore(self, pos):
        datasets.check_position(pos, "SyntheticMovingMNIST")
        self.rng.bit_generator.state = pos["rng"]

    def _trajectory(self):
        """One sample's RNG draws in the order of moving_mnist.py:43-85: per digit the sprite index, the start and
        the velocity, then the per-frame bounce rules.  Returns (ids (num_digits,), pos (num_digits, T, 2) = (sy, sx))."""
        rng, S, D = self.rng, self.image_size, self.digit_size
        ids = np.zeros(self.num_digits, np.int32)
        pos = np.zeros((self.num_digits, self.seq_len, 2), np.int32)
        for n in range(self.num_digits):
            ids[n] = rng.integers(self.N)
            sx, sy = int(rng.integers(S - D)), int(rng.integers(S - D))
            dx, dy = int(rng.integers(-4, 5)), int(rng.integers(-4, 5))
            for t in range(self.seq_len):
                if sy < 0:
                    sy = 0
                    if self.deterministic:
                        dy = -dy
                    else:
                        dy, dx = int(rng.integers(1, 5)), int(rng.integers(-4, 5))
                elif sy >= S - D:
                    sy = S - D - 1
                    if self.deterministic:
                        dy = -dy
                    else:
                        dy, dx = int(rng.integers(-4, 0)), int(rng.integers(-4, 5))
                if sx < 0:
                    sx = 0
                    if self.deterministic:
                        dx = -dx
                    else:
                        dx, dy = int(rng.integers(1, 5)), int(rng.integers(-4, 5))
                elif sx >= S - D:
                    sx = S - D - 1
                    if self.deterministic:
                        dx = -dx
                    else:
                        dx, dy = int(rng.integers(-4, 0)), int(rng.integers(-4, 5))
                pos[n, t] = (sy, sx)
                sy += dy
                sx += dx
        return ids, pos

    def __getitem__(self, index):
        S, D = self.image_size, self.digit_size
        ids, pos = self._trajectory()
        x = np.zeros((self.seq_len, S, S, 1), np.float32)
        for n in range(self.num_digits):
            digit = self.data[ids[n]]
            for t in range(self.seq_len):
                sy, sx = pos[n, t]
                x[t, sy:sy + D, sx:sx + D, 0] += digit
        x[x > 1] = 1.0
        return x

    def trajectories(self, batch_size: int):
        """The host half of a batch: sprite ids (B, num_digits) and positions (B, num_digits, T, 2) int32, drawn in the
        order `batch()` draws them (same generator state -> same batch)."""
        trajs = [self._trajectory() for _ in range(batch_size)]
        ids = np.stack([t[0] for t in trajs])
        pos = np.stack([t[1] for t in trajs])
        lim = self.image_size - self.digit_size
        if ids.min() < 0 or ids.max() >= self.N or pos.min() < 0 or pos.max() > lim:
            raise RuntimeError("SyntheticMovingMNIST: trajectory outside the canvas")
        return ids, pos

    def batch_device(self, batch_size: int, device) -> list:
        """The same batch as `utils.normalize_data(opt, dtype, self.batch(batch_size))` - bit for bit, given the same
        generator state - composited on the GPU (dvg_moving_mnist_compose) straight into the T x (B,1,S,S) layout:
        only the integer trajectories (a few KB) cross PCIe."""
        return self.compose_device(*self.trajectories(batch_size), device)

    def compose_device(self, ids, pos, device) -> list:
        """The device half: additive compositing + clip + normalize_data's layout in one kernel."""
        from . import ops
        if getattr(self, "_dev_sprites", None) is None or self._dev_sprites.device != torch.device(device):
            self._dev_sprites = torch.from_numpy(self.data).to(device)
        out = ops.moving_mnist_compose(self._dev_sprites, torch.from_numpy(ids).to(device),
                                       torch.from_numpy(pos).to(device), self.seq_len, self.image_size)
        return [out[t] for t in range(self.seq_len)]

    def batch(self, batch_size: int) -> torch.Tensor:
        return torch.from_numpy(np.stack([self[i] for i in range(batch_size)]))  # (B,T,H,W,1)


def synthetic_video(batch, seq_len, channels, res, seed=1) -> torch.Tensor:
    """(B,T,H,W,C) U[0,1]-textured clips with temporal coherence, for the KTH/BAIR/UCF-shaped configs."""
    rng = np.random.default_rng(seed)
    base = rng.random((batch, 1, res, res, channels), dtype=np.float32)
    # float32 draws, scaled / accumulated / clipped in place: the float64 form took longer on the host than a dcgan_64
    # training iteration at this shape takes on the GPU (train.py draws batches on a background thread)
    drift = rng.standard_normal((batch, seq_len, res, res, channels), dtype=np.float32)
    drift *= np.float32(0.05)
    np.cumsum(drift, axis=1, out=drift)
    drift += base
    return torch.from_numpy(np.clip(drift, 0, 1, out=drift))


class _Batch:
    """A drawn batch: calling it (on the thread that owns the GPU stream) puts it on the device; `position` is where the
    sampler stood right after this batch's draws, i.e. where a run that has consumed this batch resumes."""
    __slots__ = ("load", "position")

    def __init__(self, load, position):
        self.load, self.position = load, position

    def __call__(self):
        return self.load()


class _Counter:
    """The `seed + k` stream of the textured synthetic clips as a sampler: its position is k."""

    def __init__(self):
        self.k = 0

    def position(self):
        return {"sampler": "synthetic_video", "k": self.k}

    def restore(self, pos):
        datasets.check_position(pos, "synthetic_video")
        self.k = int(pos["k"])


class BatchStream:
    """What make_batch_generator returns: an endless iterator of `load()` callables over one host sampler.  `draw()` makes the
    host half of the next batch (integers only), `load(host)` the device half.  The sampler's state is taken right after every
    draw and travels with the yielded callable (`.position`), because whoever sits in front (train_graphs.BatchPrefetcher) draws
    ahead of what the training loop has consumed: the position of a RUN is that of the last batch it consumed, not the
    sampler's.  `position()` is the position of the last batch handed out (before the first: the sampler's initial state);
    `restore(position)` makes the next batch the one that followed that position in the run that saved it, bit for bit.
    `first`: called once before the first draw (the synthetic path's warning / refusal, which stay lazy)."""

    def __init__(self, sampler, draw, load, first=None, augmenter=None):
        self.sampler, self._draw, self._load, self._first, self.augmenter = sampler, draw, load, first, augmenter
        self._pos = self._position()

    def _position(self):
        """The sampler's position; with `--augment` it also carries the augmenter's, under "augment"."""
        pos = self.sampler.position()
        return pos if self.augmenter is None else dict(pos, augment=self.augmenter.position())

    def __iter__(self):
        return self

    def __next__(self):
        if self._first is not None:
            first, self._first = self._first, None
            first()
        host = self._draw()
        self._pos = self._position()
        return _Batch(lambda: self._load(host), self._pos)

    def position(self):
        return self._pos

    def restore(self, pos):
        saved = pos.get("augment") if isinstance(pos, dict) else None
        if self.augmenter is None and saved is not None:
            raise SystemExit(f"data position: saved with --augment {saved.get('spec')!r}, this run has no --augment")
        if self.augmenter is not None and saved is None:
            raise SystemExit(f"data position: saved without --augment, this run has --augment {self.augmenter.spec!r}")
        if self.augmenter is not None:
            self.augmenter.restore(saved)
            pos = {k: v for k, v in pos.items() if k != "augment"}
        self.sampler.restore(pos)
        self._pos = self._position()


def make_batch_generator(opt, seq_len, seed, device=None, train=True):
    """Yields `load()` callables: the host half of a batch has been drawn when the callable is yielded, calling it (on the
    thread that owns the GPU stream) puts the batch on the device as normalize_data's list of T x (B,C,H,W) frames.
    smmnist: the host draws the integer trajectories, the device composites them (bit-identical to the host batch).  With the
    MNIST image files of both splits under `--data_root` (dvg_amd/mnist.py: <root>/MNIST/raw, <root>/raw or <root>, raw or .gz)
    the wanted split is read, uploaded and scaled to 32x32 ONCE, before this returns (dvg_mnist_scale_u8); a batch is then the
    reference's draws (mnist.MovingMnistSampler) and one dvg_moving_mnist_compose_u8 launch.  Without them, or with
    --synthetic_data, it is the reference's trajectory generator over seeded in-repo sprites, and says so.
    kth | bair | ucf | frames (a folder of clips: datasets.frames_index): the `train` / test split under `--data_root` is indexed and decoded once into a device frame pool
    (dvg_amd/datasets.py) BEFORE this returns - a missing tree is a SystemExit here, on the caller's thread; the host half
    then draws `local_batch` clips like the reference's loaders, the callable uploads the B pool indices and gathers the
    clips on the current stream (dvg_clip_gather_u8).  With --synthetic_data those names train on random textured clips of
    their shape instead.  `opt.resize` / `opt.resize_fit` (--resize; docs/DESIGN_NOTES_frames.md): decoded frames that are not
    image_width x image_width are scaled into the pool by dvg_resample_u8, bit-equal to Pillow's Image.resize.  `opt.augment` (train.py --augment; docs/DESIGN_NOTES_augment.md) applies to the TRAIN split of these
    three only: the host also draws per-clip flip / reverse / shift / jitter parameters (datasets.ClipAugmenter) and the gather
    is dvg_clip_gather_aug_u8; `train=False` ignores it.
    The result is a BatchStream: `position()` / `restore()` report and set where the stream stands (train.py --resume)."""
    if opt.dataset in datasets.REAL_DATASETS and not getattr(opt, 'synthetic_data', False):
        return _clip_batches(opt, seq_len, seed, device or torch.device('cuda'), train)
    tried = None
    if opt.dataset == 'smmnist' and not getattr(opt, 'synthetic_data', False):
        root = getattr(opt, 'data_root', None)
        path = mnist.find_tree(root, train) if root else None
        if path is not None:
            return _mnist_batches(opt, seq_len, seed, device or torch.device('cuda'), path)
        if root and os.path.isdir(root):
            tried = [p for t in (True, False) for p in mnist.candidates(root, t)]
    return _synthetic_batches(opt, seq_len, seed, device, tried)


def _clip_batches(opt, seq_len, seed, device, train):
    index = datasets.open_index(opt.dataset, opt.data_root, train, opt.image_width)
    sampler = datasets.make_sampler(index, seq_len, seed)
    pool = datasets.shared_pool(index, opt.data_root, opt.image_width, device, getattr(opt, 'data_threads', 5),
                                datasets.resize_spec(opt))       # --resize: frames of another size are scaled into the pool
    if opt.channels != pool.shape[3] and not (opt.channels == 1 and pool.shape[3] == 3):
        raise SystemExit(f"dataset: --channels {opt.channels} from {opt.dataset} frames of {pool.shape[3]} channel(s) under "
                         f"{opt.data_root!r}")

    def firsts():
        return np.array([sampler.draw()[0] for _ in range(opt.local_batch)], np.int64)

    def load(first):
        from . import ops
        return list(ops.clip_gather(pool, first, seq_len, opt.channels).unbind(0))
    cfg = datasets.parse_augment(getattr(opt, 'augment', '') or '')
    if not train or not datasets.augment_spec(cfg):       # the test split is never augmented; no --augment: the path above, as ever
        return BatchStream(sampler, firsts, load)
    # --augment (train split): the host half of a batch is (first, geom, photo), the device half still one upload and one
    # launch.  The augmenter draws from its own generator, after the sampler's draws of the batch: the clips stay the same
    augmenter = datasets.ClipAugmenter(cfg, seed ^ datasets.AUGMENT_SEED_XOR)

    def load_aug(host):
        from . import ops
        return list(ops.clip_gather_aug(pool, host[0], host[1], host[2], seq_len, opt.channels).unbind(0))
    return BatchStream(sampler, lambda: (firsts(), *augmenter.draw(opt.local_batch)), load_aug, augmenter=augmenter)


def _mnist_batches(opt, seq_len, seed, device, path):
    from . import ops
    try:
        raw = mnist.read_idx_images(path)
    except ValueError as e:
        raise SystemExit(str(e))
    sprites = ops.mnist_scale_u8(torch.from_numpy(raw.copy()).to(device), mnist.DIGIT_SIZE)      # the pool stays uint8
    sampler = mnist.MovingMnistSampler(len(raw), seq_len, opt.num_digits, opt.image_width, seed)

    return BatchStream(sampler, lambda: sampler.draw(opt.local_batch),
                       lambda h: list(ops.moving_mnist_compose_u8(sprites, h[0], h[1], seq_len, opt.image_width).unbind(0)))


def _synthetic_batches(opt, seq_len, seed, device, mnist_tried=None):
    def first():
        if opt.dataset != 'smmnist' and not getattr(opt, 'synthetic_data', False):
            raise SystemExit(f"train.py: no loader for --dataset {opt.dataset} (kth | bair | ucf | frames read --data_root). "
                             "Pass --synthetic_data to train on synthetic clips of that dataset's shape.")
        if opt.rank == 0:
            what = ("Moving-MNIST trajectories over synthetic sprites (not MNIST digits)" if opt.dataset == 'smmnist'
                    else f"random textured clips shaped like {opt.dataset}")
            print(f"WARNING: synthetic data - {what}; --data_root is ignored", file=sys.stderr)
            if mnist_tried:
                print("         no MNIST image files of both splits under --data_root; tried: " + ", ".join(mnist_tried), file=sys.stderr)
    if opt.dataset == 'smmnist':
        ds = SyntheticMovingMNIST(seq_len=seq_len, num_digits=opt.num_digits, image_size=opt.image_width, seed=seed)
        return BatchStream(ds, lambda: ds.trajectories(opt.local_batch),
                           lambda h: ds.compose_device(h[0], h[1], device or torch.device('cuda')), first)
    counter = _Counter()

    def draw():
        seq = synthetic_video(opt.local_batch, seq_len, opt.channels, opt.image_width, seed=seed + counter.k)
        counter.k += 1
        return seq
    return BatchStream(counter, draw, lambda seq: normalize_data(opt, torch.cuda.FloatTensor, seq)[0], first)
