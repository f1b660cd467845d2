"""Wrappers of the gradient-guard entry points (grad_guard.hip): the fp64 sum of squares of a flat gradient range in fixed
chunks and the one-workgroup decision kernel (the Adam step that applies its verdict: ops.adam_step).  dvg_amd/optim.py
(GradGuard, guarded_step) is the caller."""
from __future__ import annotations

import torch

from .._lib import check, lib
from ._core import _dev_f32, _p, _run, _stream


def grad_sumsq_blocks(n: int) -> int:
    """Partial sums dvg_grad_sumsq writes for `n` floats: a function of n alone."""
    return int(lib().dvg_grad_sumsq_blocks(int(n)))


def grad_sumsq(g: torch.Tensor, partials: torch.Tensor, slot: int = 0) -> int:
    """partials[slot : slot + blocks] = the fp64 sums of squares of the chunks of the flat fp32 tensor `g` (numel % 4 == 0,
    16-byte aligned); returns the number of slots written."""
    _dev_f32(g, "grad_sumsq.g")
    if not g.is_contiguous() or partials.dtype != torch.float64 or not partials.is_contiguous() or partials.device != g.device:
        raise RuntimeError("grad_sumsq: a contiguous gradient range and a contiguous fp64 partials buffer on its device expected")
    n = g.numel()
    nb = grad_sumsq_blocks(n)
    if slot < 0 or slot + nb > partials.numel():
        raise RuntimeError(f"grad_sumsq: {nb} partial sums from slot {slot} do not fit {partials.numel()}")
    _run("grad_sumsq", 2.0 * n, 4.0 * n, lib().dvg_grad_sumsq, _p(g), n, partials.data_ptr() + 8 * slot, _stream())
    return nb


def grad_guard_finish(partials: torch.Tensor, nblocks: int, max_norm: float, skip_nonfinite: bool, stat: torch.Tensor,
                      counters: torch.Tensor) -> None:
    """stat (4 floats: norm, clip factor, skip, max finite norm) and counters (3 ints: sites, clipped, skipped) from
    partials[0:nblocks] (dvg_grad_guard_finish)."""
    if (partials.dtype != torch.float64 or stat.dtype != torch.float32 or counters.dtype != torch.int32 or stat.numel() != 4
            or counters.numel() != 3 or not 0 < nblocks <= partials.numel() or not partials.is_cuda
            or stat.device != partials.device or counters.device != partials.device):
        raise RuntimeError("grad_guard_finish: fp64 partials, 4 fp32 stat values and 3 int32 counters on one GPU expected")
    check(lib().dvg_grad_guard_finish(_p(partials), int(nblocks), float(max_norm), int(bool(skip_nonfinite)), _p(stat),
                                      _p(counters), _stream()), "grad_guard_finish")
