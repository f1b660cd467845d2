"""Wrappers of the weight-average entry points (ema.hip): one streaming launch that moves a flat fp32 average towards the flat
parameters and leaves the two fp64 partial sums per chunk that measure how far it lags.  dvg_amd/ema.py (WeightAverage) is the
caller."""
from __future__ import annotations

import torch

from .._lib import lib
from ._core import _dev_f32, _p, _run, _stream


def ema_update_blocks(n: int) -> int:
    """Pairs of partial sums dvg_ema_update writes for `n` floats: a function of n alone."""
    return int(lib().dvg_ema_update_blocks(int(n)))


def ema_update(ema: torch.Tensor, param: torch.Tensor, decay: float, updates: torch.Tensor, partials: torch.Tensor) -> int:
    """ema = fmaf(w, param - ema, ema) over two flat fp32 tensors of one size (numel % 4 == 0, 16-byte aligned), with
    w = 1 - min(decay, (1 + k) / (10 + k)) for k = updates[0], one device int32 the kernel only reads; partials[2b], [2b + 1] =
    the fp64 sums of (param - ema')^2 and param^2 over chunk b.  Returns the number of pairs written."""
    _dev_f32(ema, "ema_update.ema")
    _dev_f32(param, "ema_update.param")
    if not ema.is_contiguous() or not param.is_contiguous() or param.numel() != ema.numel() or param.device != ema.device:
        raise RuntimeError("ema_update: two contiguous fp32 ranges of one size on one device expected")
    if (updates.dtype != torch.int32 or updates.numel() != 1 or updates.device != ema.device or partials.dtype != torch.float64
            or not partials.is_contiguous() or partials.device != ema.device):
        raise RuntimeError("ema_update: a one-element int32 counter and a contiguous fp64 partials buffer on ema's device expected")
    n = ema.numel()
    nb = ema_update_blocks(n)
    if 2 * nb > partials.numel():
        raise RuntimeError(f"ema_update: {2 * nb} partial sums do not fit {partials.numel()}")
    _run("ema_update", 2.0 * n, 12.0 * n, lib().dvg_ema_update, _p(ema), _p(param), n, float(decay), _p(updates), _p(partials),
         _stream())
    return nb
