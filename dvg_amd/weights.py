"""Every repacked form of a layer weight that a kernel reads, built once per parameter version.

The eval / no-grad blocks (fused.py) and the training Functions (autograd.py, autograd_recurrent.py) ask for the same forms
through these accessors, so a form exists once however many paths use it: train_model alone calls the encoder 2*S and the
decoder 3*S times between two optimiser steps (train.py:213-232), and the fine-tuning closures run the same encoder again
without autograd.  Every accessor is keyed on the weight Parameter itself (`_derived.derived`, valid while the parameter
keeps its data pointer and version).  A channel slice [lo, hi) that covers the whole axis is the unsliced form.
"""
from __future__ import annotations

import torch

from . import ops
from ._derived import derived


def _span(weight, lo, hi, dim):
    """(lo, hi, dim) of a channel slice, or three Nones when it is the whole weight."""
    return (None, None, None) if lo is None or (lo == 0 and hi == weight.shape[dim]) else (lo, hi, dim)


def _sliced(weight, lo, hi, dim):
    w = weight.detach()
    if lo is not None:
        w = w[lo:hi] if dim == 0 else w[:, lo:hi]
    return w.contiguous()


def packed(weight, transposed=False, lo=None, hi=None, dim=0):
    """[taps][Cout][Cin] repack (ops.pack_igemm_weight) of a Conv2d weight, or - `transposed` - of a ConvTranspose2d weight
    or a Conv2d's data-gradient kernel; optionally of the channels [lo, hi) along `dim` (the x half and the skip half of a
    concat conv: dim 1 of a Conv2d weight, dim 0 of a ConvTranspose2d weight)."""
    lo, hi, dim = _span(weight, lo, hi, dim)
    return derived(weight, ("wp", transposed, lo, hi, dim), (weight,),
                   lambda: ops.pack_igemm_weight(_sliced(weight, lo, hi, dim), transposed))


def wx(weight, lo=None, hi=None):
    """The F(2,3)-row repack (ops.pack_wx_weight) of a Conv2d 3x3 weight that the WX kernels read, optionally of the input
    channels [lo, hi)."""
    lo, hi, dim = _span(weight, lo, hi, 1)
    return derived(weight, ("wx", lo, hi), (weight,), lambda: ops.pack_wx_weight(_sliced(weight, lo, hi, dim)))


def split_packed(weight, c1: int, transposed=False):
    """The packed x half and skip half of a concat conv's weight: the channels [0, c1) and [c1, C) of dim 1 of a Conv2d
    weight, or - `transposed` - of dim 0 of a ConvTranspose2d weight."""
    dim = 0 if transposed else 1
    return packed(weight, transposed, 0, c1, dim), packed(weight, transposed, c1, weight.shape[dim], dim)


def winograd(weight, m, lo=None, hi=None, dgrad=False):
    """Winograd-domain weights U = G g G^T (ops.winograd_weight) of a Conv2d weight for F(m x m, 3x3), optionally of the
    input channels [lo, hi): forward form, or - dgrad - of the flipped / transposed kernel whose 3x3 correlation with d(out)
    is the data gradient."""
    lo, hi, _ = _span(weight, lo, hi, 1)

    def build():
        w = weight.detach()
        if lo is not None:
            w = w[:, lo:hi]
        if dgrad:
            w = w.transpose(0, 1).flip(2, 3)
        return ops.winograd_weight(w.contiguous(), m)

    return derived(weight, ("wino", m, lo, hi, dgrad), (weight,), build)


def winograd_live(weight, lo=None, hi=None):
    """The 25 slabs of winograd(weight, 4, lo, hi) at ops.LIVE_POSITIONS: the U of an F(4x4) layer that reads its input through
    nearest-x2 upsampling and runs on the live positions alone (ops.conv3x3_winograd(live=True)).  A gather of the packed 36-slab
    tensor - the position is its outermost axis - once per weight version."""
    lo, hi, _ = _span(weight, lo, hi, 1)

    def build():
        u = winograd(weight, 4, lo, hi)
        return u.index_select(0, torch.tensor(ops.LIVE_POSITIONS, device=u.device))

    return derived(weight, ("wino_live", lo, hi), (weight,), build)


def k4_weight(weight, c1: int) -> torch.Tensor:
    """nearest-x2 upsampling followed by a 3x3 conv (pad 1) IS a stride-2 transposed conv with the 4x4 kernel
    K4 = W (*) ones(2x2): of the 9 taps of an output pixel only 4 distinct low-resolution inputs contribute.  Returns K4
    of the x half W[:, :c1] of a Conv2d weight in ConvTranspose2d layout (C1, Cout, 4, 4).  Tap t (0..2) of the 3x3
    kernel lands on k = 2 - t and k = 3 - t of the 4-tap kernel, per axis."""
    w = weight.detach()[:, :c1]                           # (Cout, C1, 3, 3)
    k4 = torch.zeros((w.shape[0], c1, 4, 4), device=w.device, dtype=torch.float32)
    for ty in range(3):
        for tx in range(3):
            k4[:, :, 2 - ty:4 - ty, 2 - tx:4 - tx] += w[:, :, ty:ty + 1, tx:tx + 1]
    return k4.permute(1, 0, 2, 3).contiguous()


def k4_packed(weight, c1: int, adjoint=False):
    """The packed K4 (k4_weight) of the x half of a concat conv: the x half of every decoder block's first conv
    (vgg_64.py:98-105) then runs on the CONVT4S2 igemm mode with 4/9 of the MACs.  adjoint: the same K4 packed for the data
    gradient (a plain 4x4 stride-2 conv with the same weight).  K4 itself is kept, so that the pair costs one K4."""
    def build():
        k4 = derived(weight, ("k4", c1), (weight,), lambda: k4_weight(weight, c1))
        return ops.pack_igemm_weight(k4, transposed=not adjoint)

    return derived(weight, ("k4p", c1, adjoint), (weight,), build)


def transposed(weight):
    """Contiguous transpose of a 2-D parameter: the data gradients of Linear / LSTMCell are NT GEMMs against W^T, and BPTT
    asks for the same transpose once per time step."""
    return derived(weight, "T", (weight,), lambda: ops.transpose2d(weight.detach()))


def gemm_operand(weight, kind: str):
    """Weights of the two dense ends as [N][K] GEMM operands in NHWC flatten order.

    kind == "head": Conv2d(512,dim,4,1,0) on a 4x4 map (vgg_64.py:44):
        W[n][ (h*4+w)*512 + c ] = w[n][c][h][w]
    kind == "stem": ConvTranspose2d(dim,512,4,1,0) on a 1x1 map (vgg_64.py:65):
        W[ (h*4+w)*512 + c ][k] = w[k][c][h][w]
    kind == "stem_t": the same transposed to [KP][N], rows zero-padded to KP in {96, 128} (dvg_stem_gemm), or None
        when dim > 128 / N % 32 != 0.
    kind == "head_T" / "stem_T": the plain 2-D transpose of "head" / "stem" (the data gradient's NT operand).
    """
    def build():
        if kind.endswith("_T"):
            return ops.transpose2d(gemm_operand(weight, kind[:-2]))
        w = weight.detach()
        if kind == "head":
            n, c, kh, kw = w.shape
            return w.permute(0, 2, 3, 1).reshape(n, kh * kw * c).contiguous()
        k, c, kh, kw = w.shape
        if kind == "stem":
            return w.permute(2, 3, 1, 0).reshape(kh * kw * c, k).contiguous()
        gw = None
        if k <= 128 and (kh * kw * c) % 32 == 0:
            gw = torch.zeros((96 if k <= 96 else 128, kh * kw * c), device=w.device, dtype=torch.float32)
            gw[:k] = w.permute(0, 2, 3, 1).reshape(k, kh * kw * c)
        return gw

    if kind not in ("head", "stem", "stem_t", "head_T", "stem_T"):
        raise RuntimeError(kind)
    return derived(weight, ("gw", kind), (weight,), build)


def first_pair_taps(weight):
    """[tap][channel] form of the 1 -> 64 channel 3x3 weight that opens the fused first pair (ops.conv3x3_first_pair)."""
    return derived(weight, "w_t9x64", (weight,), lambda: weight.detach().reshape(64, 9).t().contiguous())
