"""Frames of any size into the frame pool (resample.hip): Pillow's 8-bit `Image.resize`, bit for bit, on the device."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import resample
from .._lib import lib
from ._core import _p, _run, _stream

# (device, Hin, Win, Hout, Wout, filter, box) -> the tables of a geometry on the device, plus the host copy of ymin.  Constants
# of the geometry, not derived from a parameter, and never made or used under a graph capture (the pool is built before any):
# this cache stays outside _derived's registry on purpose.  A run sees a handful of geometries (one per frame size in the tree).
_TABLES = {}
TABLES_MAX = 256


def _geometry(device, hin, win, hout, wout, filter, box):
    key = (str(device), hin, win, hout, wout, filter, box)
    hit = _TABLES.get(key)
    if hit is not None:
        return hit
    x0, y0, x1, y1 = box
    xt = resample.tables(win, x0, x1, wout, filter) if resample.pass_needed(win, x0, x1, wout) else None
    yt = resample.tables(hin, y0, y1, hout, filter) if resample.pass_needed(hin, y0, y1, hout) else None
    dev = [None if t is None else tuple(torch.from_numpy(a).to(device) for a in t) for t in (xt, yt)]
    if len(_TABLES) >= TABLES_MAX:
        _TABLES.clear()
    hit = _TABLES[key] = (dev[0], dev[1], None if yt is None else np.ascontiguousarray(yt[0]))
    return hit


def resample_band(hin, win, hout, wout, c, filter='bilinear', box=None):
    """(band, span) dvg_resample_u8 runs a geometry with: output rows per workgroup and the most input rows a band needs;
    band 0 = not even a one-row band fits the LDS budget (dvg_resample_u8 refuses it)."""
    x0, y0, x1, y1 = resample.check_box(box, win, hin)
    yk, ymin = 0, None
    if resample.pass_needed(hin, y0, y1, hout):
        ymin, coef = resample.tables(hin, y0, y1, hout, filter)
        yk = coef.shape[1]
    span = ctypes.c_int(0)
    band = lib().dvg_resample_u8_band(None if ymin is None else ymin.ctypes.data, hin, win, hout, wout, c, yk, ctypes.addressof(span))
    return band, span.value


def resample_u8(src, out_hw, filter='bilinear', box=None, out=None):
    """(n,Hout,Wout,C) uint8 = Pillow's `resize((Wout, Hout), FILTER, box=box)` of every frame of src (n,Hin,Win,C) uint8, C = 1 or
    3, bit for bit (dvg_resample_u8).  filter: one of resample.FILTERS; box (x0, y0, x1, y1) in integers, None = the whole frame.
    A pass the geometry does not need is skipped exactly as ImagingResample skips it (both: a copy).  The coefficient tables come
    from dvg_amd/resample.py and stay on the device per geometry.  `out`: where to write - a contiguous (n,Hout,Wout,C) uint8
    tensor on src's device, e.g. a slice pool[a:b] of the frame pool."""
    if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dtype != torch.uint8 or src.dim() != 4 or not src.is_contiguous() \
            or src.numel() == 0:
        raise RuntimeError("resample_u8: src must be a contiguous non-empty (n,H,W,C) uint8 GPU tensor - no CPU fallback")
    n, hin, win, c = src.shape
    if c not in (1, 3):
        raise RuntimeError(f"resample_u8: {c} channels: 1 or 3 interleaved")
    hout, wout = (int(v) for v in out_hw)
    if filter not in resample.FILTERS or hout < 1 or wout < 1:
        raise RuntimeError(f"resample_u8: filter {filter!r} -> {hout}x{wout}: one of {' | '.join(resample.FILTERS)}, sizes >= 1")
    try:
        box = resample.check_box(box, win, hin)
    except ValueError as e:
        raise RuntimeError(f"resample_u8: {e}")
    if out is None:
        out = torch.empty((n, hout, wout, c), device=src.device, dtype=torch.uint8)
    elif not isinstance(out, torch.Tensor) or out.device != src.device or out.dtype != torch.uint8 or \
            tuple(out.shape) != (n, hout, wout, c) or not out.is_contiguous():
        raise RuntimeError(f"resample_u8: out must be a contiguous ({n},{hout},{wout},{c}) uint8 tensor on src's device")
    xt, yt, ymin_host = _geometry(src.device, hin, win, hout, wout, filter, box)
    _run("resample_u8", 0.0, float(src.numel() + out.numel()), lib().dvg_resample_u8, _p(src), _p(out), n, hin, win, hout, wout, c,
         None if xt is None else _p(xt[0]), None if xt is None else _p(xt[1]), 0 if xt is None else xt[1].shape[1],
         None if yt is None else _p(yt[0]), None if yt is None else _p(yt[1]), 0 if yt is None else yt[1].shape[1],
         None if ymin_host is None else ymin_host.ctypes.data, _stream())
    return out
