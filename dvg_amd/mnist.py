"""Moving-MNIST from real digits, the host half: the MNIST IDX image files under `--data_root`, the reference's draws
(data/moving_mnist.py:47-88) from a private generator, the coefficient tables of Pillow's bilinear resize, and numpy
restatements of the resize and of the compositing that the tests hold the kernels against.  Host code, no GPU at import.

The device half is dvg_amd/csrc/mnist.hip: `ops.mnist_scale_u8` scales a split's digits once (`transforms.Scale(32)`,
moving_mnist.py:24-26), `ops.moving_mnist_compose_u8` makes a batch from the uint8 pool and the integer trajectories.

Out of scope: the download (`datasets.MNIST(..., download=True)`) and torchvision's processed `.pt` cache: the four IDX files
as they are published, raw or gzipped, are what is read.  Labels are not read: the reference discards them (:49)."""
from __future__ import annotations

import gzip
import math
import os
import struct

import numpy as np

DIGIT_SIZE = 32                      # moving_mnist.py:15
IDX_IMAGES_MAGIC = 0x00000803        # unsigned byte, three dimensions
FILES = {True: 'train-images-idx3-ubyte', False: 't10k-images-idx3-ubyte'}      # by `train` (utils.py:30-43)
PRECISION_BITS = 32 - 8 - 2          # Pillow's fixed point for 8-bit channels
TAPS = 3                             # Pillow's ksize = 2 * ceil(support) + 1 for an up-scaling bilinear filter


def candidates(root, train):
    """The paths tried for a split's image file, in order: torchvision's layout <root>/MNIST/raw, its old one <root>/raw, a
    flat directory; each raw, then gzipped."""
    return [os.path.join(root, *sub, FILES[bool(train)] + ext) for sub in (('MNIST', 'raw'), ('raw',), ()) for ext in ('', '.gz')]


def find_images(root, train):
    """The first existing candidate of the split, or None."""
    for p in candidates(str(root), train):
        if os.path.isfile(p):
            return p
    return None


def find_tree(root, train):
    """The image file of the wanted split when BOTH splits' image files are under `root` (what torchvision asks for before it
    reads either; it would download otherwise), else None."""
    both = {t: find_images(root, t) for t in (True, False)}
    return both[bool(train)] if all(both.values()) else None


def read_idx_images(path):
    """(n, size, size) uint8 from an IDX3 file, raw or .gz.  A wrong magic, a non-square header or a length that does not match
    the header is a ValueError naming the file."""
    try:
        with (gzip.open if str(path).endswith('.gz') else open)(path, 'rb') as f:
            data = f.read()
    except (OSError, EOFError) as e:
        raise ValueError(f"mnist: cannot read {path!r}: {e}")
    if len(data) < 16:
        raise ValueError(f"mnist: {path!r} is {len(data)} bytes, shorter than an IDX3 header")
    magic, n, h, w = struct.unpack('>IIII', data[:16])
    if magic != IDX_IMAGES_MAGIC:
        raise ValueError(f"mnist: {path!r} has magic 0x{magic:08x}, not 0x{IDX_IMAGES_MAGIC:08x} (an IDX3 file of unsigned bytes)")
    if h != w or h == 0:
        raise ValueError(f"mnist: {path!r} holds {h}x{w} images, not square ones")
    if len(data) != 16 + n * h * w:
        raise ValueError(f"mnist: {path!r} is {len(data)} bytes, its header announces {16 + n * h * w} ({n} images of {h}x{w})")
    if n == 0:
        raise ValueError(f"mnist: {path!r} holds no image")
    return np.frombuffer(data, np.uint8, offset=16).reshape(n, h, w)


def resize_tables(in_size, out_size):
    """Pillow's bilinear coefficients for one axis (Resample.c: precompute_coeffs + normalize_coeffs_8bpc), shared by both
    passes of a square resize: xmin (out,) int32 = the first input position of every output position, coef (out, TAPS) int32 =
    the weights, normalised in double and rounded to PRECISION_BITS of fixed point; unused taps are 0."""
    if not 1 <= in_size <= out_size:
        raise ValueError(f"mnist: resize {in_size} -> {out_size}: only the up-scaling filter is restated")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale                                   # the bilinear filter's support is 1
    assert 2 * math.ceil(support) + 1 == TAPS
    xmin = np.zeros(out_size, np.int32)
    coef = np.zeros((out_size, TAPS), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)                  # int(): truncation, like the C cast
        n = min(int(center + support + 0.5), in_size) - lo
        w = [max(0.0, 1.0 - abs((x + lo - center + 0.5) * (1.0 / filterscale))) for x in range(n)]
        ww = sum(w)                                               # accumulated in tap order, as Pillow does
        for x in range(n):
            k = w[x] / ww if ww != 0.0 else w[x]
            coef[xx, x] = int(-0.5 + k * (1 << PRECISION_BITS)) if k < 0 else int(0.5 + k * (1 << PRECISION_BITS))
        xmin[xx] = lo
    return xmin, coef


def resize_u8(images, out_size=DIGIT_SIZE):
    """`Image.resize((out, out), BILINEAR)` on (n, s, s) uint8 in numpy: the horizontal pass, a uint8 intermediate, the vertical
    pass; each adds 1 << 21 to the int32 sum, shifts right by 22 and clamps to 0..255.  The CPU yardstick of
    dvg_mnist_scale_u8, not on the product path."""
    images = np.asarray(images)
    if images.dtype != np.uint8 or images.ndim != 3 or images.shape[1] != images.shape[2]:
        raise ValueError("mnist: resize_u8 takes (n, s, s) uint8")
    s = images.shape[1]
    xmin, coef = resize_tables(s, out_size)
    taps = np.minimum(xmin[:, None] + np.arange(TAPS), s - 1)     # a tap past the line has coefficient 0

    def one_pass(a):                                              # resamples the LAST axis
        acc = (a[..., taps].astype(np.int32) * coef).sum(-1, dtype=np.int32) + (1 << (PRECISION_BITS - 1))
        return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)

    mid = one_pass(images)                                        # (n, s, out)
    return np.ascontiguousarray(one_pass(mid.transpose(0, 2, 1)).transpose(0, 2, 1))


def compose_host(sprites_u8, ids, pos, image_size):
    """(B, T, S, S, 1) float32 as the reference composes a clip (moving_mnist.py:42-46,86-90): float32 `+=` of byte / 255 in
    digit order, then x[x > 1] = 1.  The CPU yardstick of dvg_moving_mnist_compose_u8."""
    sprites = sprites_u8.astype(np.float32) / np.float32(255)
    B, ND, T, _ = pos.shape
    D = sprites.shape[1]
    x = np.zeros((B, T, image_size, image_size, 1), np.float32)
    for b in range(B):
        for n in range(ND):
            for t in range(T):
                sy, sx = pos[b, n, t]
                x[b, t, sy:sy + D, sx:sx + D, 0] += sprites[ids[b, n]]
    x[x > 1] = 1.
    return x


class MovingMnistSampler:
    """MovingMNIST.__getitem__'s draws in its order (moving_mnist.py:47-88): per digit randint(N), sx, sy, dx, dy, then per
    frame the bounce rules - the y rule before the x rule, (dy, dx) drawn in the former, (dx, dy) in the latter.  The reference
    seeds the legacy GLOBAL numpy generator with the first index it is asked for (:30-33,39): `seed` plays that role, and the
    private np.random.RandomState here produces the same stream."""

    def __init__(self, n_digits_in_split, seq_len, num_digits, image_size, seed, deterministic=False):
        if image_size <= DIGIT_SIZE:
            raise SystemExit(f"mnist: a {image_size}x{image_size} canvas has no room for {DIGIT_SIZE}x{DIGIT_SIZE} digits to move")
        if n_digits_in_split < 1 or seq_len < 1 or num_digits < 1:
            raise SystemExit("mnist: the split, the clip and the number of digits must not be empty")
        self.N, self.seq_len, self.num_digits, self.image_size = n_digits_in_split, seq_len, num_digits, image_size
        self.deterministic = deterministic
        self.rng = np.random.RandomState(seed)

    def _clip(self, ids, pos):
        r, lim = self.rng.randint, self.image_size - DIGIT_SIZE
        for n in range(self.num_digits):
            ids[n] = r(self.N)
            sx, sy = r(lim), r(lim)
            dx, dy = r(-4, 5), r(-4, 5)
            for t in range(self.seq_len):
                if sy < 0:
                    sy = 0
                    if self.deterministic:
                        dy = -dy
                    else:
                        dy, dx = r(1, 5), r(-4, 5)
                elif sy >= lim:
                    sy = lim - 1
                    if self.deterministic:
                        dy = -dy
                    else:
                        dy, dx = r(-4, 0), r(-4, 5)
                if sx < 0:
                    sx = 0
                    if self.deterministic:
                        dx = -dx
                    else:
                        dx, dy = r(1, 5), r(-4, 5)
                elif sx >= lim:
                    sx = lim - 1
                    if self.deterministic:
                        dx = -dx
                    else:
                        dx, dy = r(-4, 0), r(-4, 5)
                pos[n, t] = (sy, sx)
                sy += dy
                sx += dx

    def draw(self, batch_size):
        """The host half of a batch: ids (B, ND) int32 and pos (B, ND, T, 2) int32 = (sy, sx), clip after clip."""
        ids = np.zeros((batch_size, self.num_digits), np.int32)
        pos = np.zeros((batch_size, self.num_digits, self.seq_len, 2), np.int32)
        for b in range(batch_size):
            self._clip(ids[b], pos[b])
        return ids, pos

    def position(self):
        """Where the draw stream stands (data.BatchStream; train.py --resume)."""
        return {"sampler": "MovingMnistSampler", "np": self.rng.get_state()}

    def restore(self, pos):
        if not isinstance(pos, dict) or pos.get("sampler") != "MovingMnistSampler":
            got = pos.get("sampler") if isinstance(pos, dict) else type(pos).__name__
            raise SystemExit(f"data position: saved for {got}, this run draws from MovingMnistSampler")
        self.rng.set_state(pos["np"])
