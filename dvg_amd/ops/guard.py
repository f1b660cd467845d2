"""Wrappers of the gradient-guard entry points (grad_guard.hip): the fp64 sum of squares of a flat gradient range in fixed
chunks, the one-workgroup decision kernel, and the Adam step that applies its verdict.  dvg_amd/optim.py (GradGuard,
guarded_step) is the caller."""
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


def adam_step_guarded(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, step_dev, stat, skips_dev) -> None:
    """dvg_adam_step_guarded over the flat buffers p, g, m, v: the gradient times stat[1], nothing when stat[2] != 0 (then
    skips_dev, one device int, is advanced); `step_dev`: the device-side step count, None = `step`."""
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _dev_f32(t, "adam_step_guarded." + name)
        if not t.is_contiguous() or t.numel() != p.numel() or t.device != p.device:
            raise RuntimeError(f"adam_step_guarded: {name} must be contiguous, on p's device and of p's size")
    ints = [skips_dev] if step_dev is None else [skips_dev, step_dev]
    if (stat.dtype != torch.float32 or stat.numel() != 4 or stat.device != p.device or not stat.is_contiguous()
            or any(t.dtype != torch.int32 or t.numel() != 1 or t.device != p.device for t in ints)):
        raise RuntimeError("adam_step_guarded: 4 fp32 stat values and one-element int32 counters on p's device expected")
    check(lib().dvg_adam_step_guarded(_p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
                                      float(weight_decay), int(step), _p(step_dev), _p(stat), _p(skips_dev), _stream()),
          "adam_step_guarded")
