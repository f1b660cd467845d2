"""Pillow's 8-bit resampler restated, the host half: the five convolution filters of `Image.resize`, the per-axis coefficient
tables (Resample.c: precompute_coeffs + normalize_coeffs_8bpc), which passes a geometry needs (ImagingResample), the crop box
of `--resize_fit`, and a numpy restatement of the two passes that the tests hold the kernel against.  Host code, no GPU at
import.

The device half is dvg_amd/csrc/resample.hip: `ops.resample_u8` scales decoded frames of any size into the frame pool
(dvg_amd/datasets.py build_pool, `--resize`).  `mnist.resize_tables` / `dvg_mnist_scale_u8` stay what they are: the square,
up-scaling, bilinear case of the same arithmetic.

Out of scope: NEAREST (no convolution), `reducing_gap`, boxes with fractional corners, modes other than L and RGB."""
from __future__ import annotations

import math

import numpy as np

FILTERS = ('box', 'bilinear', 'hamming', 'bicubic', 'lanczos')
SUPPORT = {'box': 0.5, 'bilinear': 1.0, 'hamming': 1.0, 'bicubic': 2.0, 'lanczos': 3.0}
PRECISION_BITS = 32 - 8 - 2          # Pillow's fixed point for 8-bit channels
FITS = ('crop', 'stretch')
_H0, _H1 = float(np.float32(0.54)), float(np.float32(0.46))      # Resample.c writes them as float literals


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (_H0 + _H1 * math.cos(x))


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


KERNELS = {'box': _box, 'bilinear': _bilinear, 'hamming': _hamming, 'bicubic': _bicubic, 'lanczos': _lanczos}


def pil_filter(name):
    """Pillow's constant of a filter name."""
    from PIL import Image
    return getattr(Image.Resampling, name.upper())


def _check(in_size, lo, hi, out_size, filter):
    if filter not in FILTERS:
        raise ValueError(f"resample: unknown filter {filter!r} ({' | '.join(FILTERS)})")
    if in_size < 1 or out_size < 1 or not 0 <= lo < hi <= in_size or int(lo) != lo or int(hi) != hi:
        raise ValueError(f"resample: box [{lo}, {hi}) of an axis of {in_size} -> {out_size}: integer corners inside the image")


def tables(in_size, lo, hi, out_size, filter):
    """One axis of `resize`: the input positions [lo, hi) of an axis of in_size positions -> out_size output positions.
    xmin (out,) int32 = the first input position of every output position (absolute: the box lives in it), coef (out, ksize)
    int32 with ksize = 2 * ceil(support * max(scale, 1)) + 1 = the weights, summed in tap order, normalised in double and rounded
    to PRECISION_BITS of fixed point; unused taps are 0."""
    _check(in_size, lo, hi, out_size, filter)
    kernel = KERNELS[filter]
    scale = float(hi - lo) / out_size
    filterscale = max(scale, 1.0)
    support = SUPPORT[filter] * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xmin = np.zeros(out_size, np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = lo + (xx + 0.5) * scale
        x0 = max(int(center - support + 0.5), 0)                  # int(): truncation, like the C cast
        n = min(int(center + support + 0.5), in_size) - x0
        w = [kernel((x + x0 - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:                                               # accumulated in tap order, as Pillow does
            ww += v
        for x in range(n):
            k = w[x] / ww if ww != 0.0 else w[x]
            coef[xx, x] = int(-0.5 + k * (1 << PRECISION_BITS)) if k < 0 else int(0.5 + k * (1 << PRECISION_BITS))
        xmin[xx] = x0
    return xmin, coef


def pass_needed(in_size, lo, hi, out_size):
    """ImagingResample's need_horizontal / need_vertical: a pass is skipped when the size stays and the box is the whole axis."""
    return out_size != in_size or lo != 0 or hi != out_size


def full_box(W, H):
    return (0, 0, int(W), int(H))


def check_box(box, W, H):
    """(x0, y0, x1, y1) as integers inside a W x H image, or a ValueError; None = the whole image."""
    if box is None:
        return full_box(W, H)
    if len(box) != 4 or any(int(v) != v for v in box):
        raise ValueError(f"resample: box {box!r}: four integers (x0, y0, x1, y1)")
    x0, y0, x1, y1 = (int(v) for v in box)
    if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
        raise ValueError(f"resample: box {box!r} leaves the {W}x{H} image or is empty")
    return x0, y0, x1, y1


def fit_box(W, H, out_w, out_h, fit):
    """The source box (x0, y0, x1, y1) of `--resize_fit`: 'stretch' = the whole image; 'crop' = the largest centred box with
    integer corners and the target's aspect ratio (a square target: m = min(W, H), offsets (W - m) // 2 and (H - m) // 2)."""
    if fit not in FITS:
        raise ValueError(f"resample: unknown fit {fit!r} ({' | '.join(FITS)})")
    if min(W, H, out_w, out_h) < 1:
        raise ValueError("resample: sizes must be >= 1")
    if fit == 'stretch':
        return full_box(W, H)
    if W * out_h >= H * out_w:                                    # the image is wider than the target: full height
        bw, bh = max(1, H * out_w // out_h), H
    else:
        bw, bh = W, max(1, W * out_h // out_w)
    x0, y0 = (W - bw) // 2, (H - bh) // 2
    return x0, y0, x0 + bw, y0 + bh


def _one_pass(a, xmin, coef):
    """Resamples the LAST axis of a (..., in) uint8 array: clip8((2^21 + sum_k pixel * coef) >> 22), int32 throughout."""
    size = a.shape[-1]
    taps = np.minimum(xmin[:, None] + np.arange(coef.shape[1]), size - 1)     # a tap past the line has coefficient 0
    acc = np.full(a.shape[:-1] + (len(xmin),), 1 << (PRECISION_BITS - 1), np.int32)
    for k in range(coef.shape[1]):                                            # taps in order
        acc += a[..., taps[:, k]].astype(np.int32) * coef[:, k]
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_u8_host(images, out_hw, filter='bilinear', box=None):
    """`Image.resize((Wout, Hout), FILTER, box=box)` on (n, Hin, Win, C) uint8 in numpy, C = 1 or 3: the horizontal pass over the
    rows the vertical pass needs, a uint8 intermediate, the vertical pass; a pass the geometry does not need is skipped, as
    Pillow skips it.  The CPU yardstick of dvg_resample_u8, not on the product path."""
    images = np.asarray(images)
    if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] not in (1, 3) or 0 in images.shape:
        raise ValueError("resample: resize_u8_host takes a non-empty (n, H, W, C) uint8 array with C = 1 or 3")
    _, H, W, _ = images.shape
    out_h, out_w = (int(v) for v in out_hw)
    x0, y0, x1, y1 = check_box(box, W, H)
    a = images
    if pass_needed(W, x0, x1, out_w):
        a = _one_pass(a.transpose(0, 1, 3, 2), *tables(W, x0, x1, out_w, filter)).transpose(0, 1, 3, 2)    # (n, H, out_w, C)
    if pass_needed(H, y0, y1, out_h):
        a = _one_pass(a.transpose(0, 2, 3, 1), *tables(H, y0, y1, out_h, filter)).transpose(0, 3, 1, 2)    # (n, out_h, out_w, C)
    return np.ascontiguousarray(a)


def pil_resize(im, size, filter, fit):
    """`im.resize((size, size), FILTER, box=fit_box(...))`: what `--resize` means, and what build_pool runs on a CPU device."""
    return im.resize((size, size), pil_filter(filter), box=fit_box(im.size[0], im.size[1], size, size, fit))
