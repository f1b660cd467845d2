"""Wrapper of the learning-rate schedule's entry point (lr_schedule.hip): one single-thread launch that writes the multiplier of
this iteration and advances the device-side count of iterations (the Adam step that reads the multiplier: ops.adam_step with
`lr_scale`).  dvg_amd/lr_schedule.py (LrSchedule) is the caller."""
from __future__ import annotations

import torch

from .._lib import check, lib
from ._core import _p, _stream

LR_KINDS = ("constant", "linear", "cosine", "step")     # `kind` of dvg_lr_schedule_tick = the index


def lr_schedule_tick(kind: str, warmup: int, total: int, step_every: int, min_ratio: float, gamma: float, iters: torch.Tensor,
                     scale: torch.Tensor) -> None:
    """scale[0] = (float)s(k) for k = iters[0], then iters[0] = min(k + 1, INT_MAX): one device int32 and one device fp32, both
    read and written by the launch alone.  Every other value is a constant of the run, passed by value."""
    if kind not in LR_KINDS:
        raise RuntimeError(f"lr_schedule_tick: kind must be one of {LR_KINDS}, got {kind!r}")
    if (not iters.is_cuda or iters.dtype != torch.int32 or iters.numel() != 1 or scale.dtype != torch.float32
            or scale.numel() != 1 or scale.device != iters.device):
        raise RuntimeError("lr_schedule_tick: a one-element int32 counter and a one-element fp32 scale on one GPU expected")
    check(lib().dvg_lr_schedule_tick(LR_KINDS.index(kind), int(warmup), int(total), int(step_every), float(min_ratio),
                                     float(gamma), _p(iters), _p(scale), _stream()), "lr_schedule_tick")
