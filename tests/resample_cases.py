"""Not a test: the geometries, images and the Pillow oracle shared by tests/test_resample_host.py and tests/test_gpu_resample.py."""
import numpy as np
from PIL import Image

from dvg_amd import resample

# (Hin, Win) -> S x S
GEOMETRIES = [(120, 160, 64), (240, 320, 128), (63, 65, 64),
              (64, 64, 64),        # both passes skipped: a copy (with the full box)
              (64, 48, 64),        # the vertical pass skipped (with the full box)
              (5, 7, 8),           # up-scaling, taps clipped at both edges
              (1, 1, 4), (28, 28, 32),
              (300, 1000, 64),     # 95 horizontal lanczos taps
              (1100, 40, 64)]      # the intermediate of the whole frame exceeds a workgroup's LDS: several bands
KINDS = ("random", "checker")


def images(kind, n, H, W, C, seed=0):
    """(n, H, W, C) uint8: random bytes, or a 0 / 255 checkerboard whose phase moves with the frame and the channel (bicubic and
    lanczos overshoot on it: the clamp acts)."""
    if kind == "random":
        return np.random.default_rng([seed, H, W, C]).integers(0, 256, (n, H, W, C), dtype=np.uint8)
    i, y, x, c = np.ogrid[0:n, 0:H, 0:W, 0:C]
    return (((y + x + i + c) % 2) * 255).astype(np.uint8)


def boxes(H, W, S):
    """The full image and the `crop` box of a square target."""
    return [None, resample.fit_box(W, H, S, S, "crop")]


def pillow(imgs, S, filter, box):
    """`Image.resize((S, S), FILTER, box=box)` of every frame: the oracle."""
    C = imgs.shape[3]
    return np.stack([np.asarray(Image.fromarray(a[:, :, 0] if C == 1 else a).resize((S, S), resample.pil_filter(filter), box=box))
                     .reshape(S, S, C) for a in imgs])
