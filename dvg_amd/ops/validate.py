"""The reduction of a validation pass (train.py --val_every; dvg_amd/validate.py): dvg_val_accumulate, csrc/validate.hip."""
from __future__ import annotations

import torch

from ._core import _dev_f32, _p, _run, _stream, lib


def val_accumulators(steps: int, device):
    """(acc, cnt) for `steps` predicted steps, zeroed: acc (2, 3, steps, 2) fp64 = track, metric ssim / psnr / mse, step, {sum,
    sum of squares}; cnt (2, 3, steps) int64."""
    return (torch.zeros((2, 3, steps, 2), dtype=torch.float64, device=device),
            torch.zeros((2, 3, steps), dtype=torch.int64, device=device))


def val_accumulate(ssim: torch.Tensor, psnr: torch.Tensor, mse: torch.Tensor, acc: torch.Tensor, cnt: torch.Tensor,
                   best: torch.Tensor = None) -> None:
    """acc, cnt += the (B, S, T) metric arrays of one batch (include/dvg_hip.h: track 0 = per row the sample with the largest
    SSIM sum, track 1 = the mean over the samples; finite entries only); best (B,) int32, optional, <- that sample.  One launch
    on the current stream, nothing read back."""
    for name, t in (("ssim", ssim), ("psnr", psnr), ("mse", mse)):
        _dev_f32(t, f"val_accumulate.{name}")
        if t.dim() != 3 or t.shape != ssim.shape or t.device != ssim.device or not t.is_contiguous():
            raise RuntimeError(f"val_accumulate: {name} {tuple(t.shape)} must be a contiguous (B, S, T) tensor like ssim "
                               f"{tuple(ssim.shape)}, on its device")
    b, s, t = ssim.shape
    if (acc.dtype != torch.float64 or tuple(acc.shape) != (2, 3, t, 2) or not acc.is_contiguous() or acc.device != ssim.device or
            cnt.dtype != torch.int64 or tuple(cnt.shape) != (2, 3, t) or not cnt.is_contiguous() or cnt.device != ssim.device):
        raise RuntimeError(f"val_accumulate: acc must be a contiguous fp64 (2, 3, {t}, 2) and cnt a contiguous int64 (2, 3, {t}) "
                           "tensor on ssim's device (ops.val_accumulators)")
    if best is not None and (best.dtype != torch.int32 or tuple(best.shape) != (b,) or not best.is_contiguous() or
                             best.device != ssim.device):
        raise RuntimeError(f"val_accumulate: best must be a contiguous int32 ({b},) tensor on ssim's device")
    _run("val_accumulate", 0.0, 12.0 * ssim.numel(), lib().dvg_val_accumulate, _p(ssim), _p(psnr), _p(mse), b, s, t, _p(acc),
         _p(cnt), _p(best), _stream())
