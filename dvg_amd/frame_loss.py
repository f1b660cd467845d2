"""`train.py --frame_loss KIND --gdl_weight G --ssim_weight W_s`: the three frame terms of train_model's loss (train.py:227-239 of the reference:
plain nn.MSELoss) with an L1 or Charbonnier pixel penalty and / or the gradient-difference loss of Mathieu et al. (2016).  For one
decoder call at one step, P, T of shape (B, C, H, W), d = P - T, n = B C H W:

    pix = sum rho(d)        rho = d^2 (mse) | |d| (l1) | sqrt(d^2 + eps^2) (charbonnier; no "- eps")
    gdl = sum_{x >= 1} | |P[y, x] - P[y, x-1]| - |T[y, x] - T[y, x-1]| | + sum_{y >= 1} | |P[y, x] - P[y-1, x]| - |T[y, x] - T[y-1, x]| |
    dssim = sum over the B C images and their (H-10) x (W-10) = m / (B C) window positions of 1 - SSIM(T, P)
    term = (pix + G gdl) / n + W_s dssim / m, summed over the steps

with the reference's weights 0.001 / 1000 / 0.001 on the three calls, sign(0) = 0 everywhere (a tied edge has gradient exactly 0).
SSIM is the Finn SSIM `--val_every` selects model_best.pth by (11x11 Gaussian window, sigma 1.5, K1 0.01, K2 0.03, L 1): 1 - dssim / m
is its mean over the channels.  The fused path is one pass of dvg_frame_losses_ext (csrc/frame_loss.hip, ops.frame_losses_ext) and,
for W_s > 0, one of dvg_frame_ssim_loss (csrc/ssim_loss.hip, ops.frame_ssim_loss) that adds its gradient to the first one's;
`torch_terms` and `torch_ssim_sum` are the same definitions as torch ops, for the unfused and the step-by-step paths.
docs/DESIGN_NOTES_frame_loss.md.

Without a flag nothing here runs: `make` returns None and the Trainer takes the code path it always took - same launches, same bits.
The options are NOT part of the --resume fingerprint: resuming an MSE run with `--frame_loss l1 --gdl_weight 1` to sharpen it is a
use, not an accident; `--ssim_weight` likewise."""
from __future__ import annotations

import argparse
import math

import torch

from . import ops

KINDS = ops.FRAME_LOSS_KINDS                  # ("mse", "l1", "charbonnier"): dvg_frame_losses_ext's `kind` = the index


def _eps(text: str) -> float:
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not a number") from None
    if not 0.0 < v < math.inf:                 # NaN fails too
        raise argparse.ArgumentTypeError("must be a finite number > 0")
    return v


def _weight(text: str) -> float:
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not a number") from None
    if not 0.0 <= v < math.inf:
        raise argparse.ArgumentTypeError("must be a finite number >= 0")
    return v


def add_arguments(parser) -> None:
    g = parser.add_argument     # docs/DESIGN_NOTES_frame_loss.md
    g('--frame_loss', default='mse', choices=KINDS,
      help='the pixel penalty of the three frame terms: mse (the reference), l1, or charbonnier sqrt(d^2 + eps^2); not part of '
           'the --resume fingerprint: an MSE run may be resumed with another frame loss to sharpen it')
    g('--charbonnier_eps', default=1e-3, type=_eps, metavar='E', help='--frame_loss charbonnier: eps > 0 (default 1e-3)')
    g('--gdl_weight', default=0.0, type=_weight, metavar='G',
      help='add G times the gradient-difference loss (Mathieu et al. 2016, alpha = 1) to every frame term, G >= 0 (default 0: '
           'none); like --frame_loss it may change on --resume')
    g('--ssim_weight', default=0.0, type=_weight, metavar='W_s',
      help='add W_s times the mean of 1 - SSIM (the Finn SSIM --val_every selects by; frames of 11 x 11 pixels or more) to every '
           'frame term, W_s >= 0 (default 0: none); like --frame_loss it may change on --resume')


class FrameLossSpec:
    """What the options ask for: `kind` (a name of KINDS), `eps` (charbonnier's), `gdl` (G), `ssim` (W_s)."""

    def __init__(self, kind: str, eps: float = 1e-3, gdl: float = 0.0, ssim: float = 0.0):
        kind, eps, gdl, ssim = str(kind), float(eps), float(gdl), float(ssim)
        if kind not in KINDS:
            raise ValueError(f"frame loss: kind must be one of {', '.join(KINDS)}")
        if not 0.0 < eps < math.inf:
            raise ValueError("frame loss: eps must be a finite number > 0")
        if not 0.0 <= gdl < math.inf:
            raise ValueError("frame loss: the gdl weight must be a finite number >= 0")
        if not 0.0 <= ssim < math.inf:
            raise ValueError("frame loss: the ssim weight must be a finite number >= 0")
        self.kind, self.eps, self.gdl, self.ssim = kind, eps, gdl, ssim

    @property
    def kind_id(self) -> int:
        return KINDS.index(self.kind)

    def label(self) -> str:
        text = self.kind if self.gdl == 0.0 else '%s + %g gdl' % (self.kind, self.gdl)
        return text if self.ssim == 0.0 else '%s + %g ssim' % (text, self.ssim)

    def __repr__(self):
        return f"FrameLossSpec({self.kind!r}, eps={self.eps!r}, gdl={self.gdl!r}" + (f", ssim={self.ssim!r})" if self.ssim else ")")


def make(opt):
    """The spec train.py's options ask for; None for mse with G = 0 and W_s = 0 (an options object from before the flags has no
    such attribute): the Trainer then runs the code it always ran.  Host only."""
    kind = getattr(opt, "frame_loss", "mse")
    gdl = float(getattr(opt, "gdl_weight", 0.0) or 0.0)
    ssim = float(getattr(opt, "ssim_weight", 0.0) or 0.0)
    if kind == "mse" and gdl == 0.0 and ssim == 0.0:
        return None
    try:
        return FrameLossSpec(kind, getattr(opt, "charbonnier_eps", 1e-3), gdl, ssim)
    except ValueError as e:
        raise SystemExit(f"train.py: {e}") from None


def torch_terms(x_pred, x_target, spec):
    """(pix, gdl) of the definition above as 0-dim tensors: plain torch, differentiable, any device and dtype.  The operands are
    (..., H, W) and broadcast against each other; every leading index is a plane.  gdl is an exact 0 for G = 0."""
    d = x_pred - x_target
    if spec.kind == "mse":
        pix = (d * d).sum()
    elif spec.kind == "l1":
        pix = d.abs().sum()
    else:
        pix = (d * d + spec.eps * spec.eps).sqrt().sum()
    if spec.gdl == 0.0:
        return pix, torch.zeros((), dtype=d.dtype, device=d.device)
    gdl = torch.zeros((), dtype=d.dtype, device=d.device)
    for dim in (-1, -2):                       # neighbours along x, then along y; a size of 1 has no edge
        n = d.shape[dim]
        dp = x_pred.narrow(dim, 1, n - 1) - x_pred.narrow(dim, 0, n - 1)
        dt = x_target.narrow(dim, 1, n - 1) - x_target.narrow(dim, 0, n - 1)
        gdl = gdl + (dp.abs() - dt.abs()).abs().sum()
    return pix, gdl


SSIM_WIN, SSIM_SIGMA, SSIM_C1, SSIM_C2 = 11, 1.5, 0.01 ** 2, 0.03 ** 2     # utils.finn_ssim's window and constants, L = 1


def ssim_positions(shape) -> int:
    """m: the window positions of a (..., H, W) operand, (H - 10) (W - 10) per plane."""
    h, w = shape[-2], shape[-1]
    if h < SSIM_WIN or w < SSIM_WIN:
        raise ValueError(f"--ssim_weight: {h}x{w} frames are smaller than the 11x11 window")
    return math.prod(shape[:-2]) * (h - SSIM_WIN + 1) * (w - SSIM_WIN + 1)


def _ssim_filter(a, g):
    """The separable window over the valid positions of (..., H, W): 11 shifted slices times taps along x, then along y - no
    convolution library, so any dtype on any device."""
    wo, ho = a.shape[-1] - SSIM_WIN + 1, a.shape[-2] - SSIM_WIN + 1
    rows = sum(g[k] * a[..., k:k + wo] for k in range(SSIM_WIN))
    return sum(g[k] * rows[..., k:k + ho, :] for k in range(SSIM_WIN))


def torch_ssim_sum(x_pred, x_target):
    """sum (1 - SSIM) over every plane and window position of (..., H, W) operands (which broadcast against each other) as a 0-dim
    tensor: plain torch, differentiable, any device and dtype.  tests/finn_ref.ssim_map's arithmetic in the operands' dtype."""
    i = torch.arange(SSIM_WIN, dtype=torch.float64) - SSIM_WIN // 2
    g = torch.exp(-i * i / (2.0 * SSIM_SIGMA ** 2))
    g = (g / g.sum()).tolist()
    x, y = torch.broadcast_tensors(x_target, x_pred)
    mx, my = _ssim_filter(x, g), _ssim_filter(y, g)
    vx, vy, vxy = _ssim_filter(x * x, g) - mx * mx, _ssim_filter(y * y, g) - my * my, _ssim_filter(x * y, g) - mx * my
    s = ((2 * mx * my + SSIM_C1) * (2 * vxy + SSIM_C2)) / ((mx * mx + my * my + SSIM_C1) * (vx + vy + SSIM_C2))
    return (1 - s).sum()


def term(pix, gdl, spec, n: float, dssim=None, m: float = 1.0):
    """(pix + G gdl) / n + W_s dssim / m: one frame term, from sums over the steps; n = elements, m = window positions per decoder
    call."""
    t = (pix + spec.gdl * gdl) / n if spec.gdl != 0.0 else pix / n
    return t + spec.ssim * dssim / m if spec.ssim != 0.0 else t


WEIGHTS = (0.001, 1000.0, 0.001)              # train.py:239 on the calls x_pred, x_target_pred, x_pred_gp (mse, ae_mse, mse_gp)


class FrameTerms:
    """What the Trainer holds under the flags: the three frame terms by either path, and the epoch line's sums on the device -
    `acc` = [pix, gdl, iterations, pixels] of the x_pred call, advanced once per train_model by three tiny device adds (eagerly and
    under capture alike: the buffer is allocated here and never changes its address) and read once per epoch.  Each rank sums its own
    shard of the batch and no collective is added: with several ranks the printed line is rank 0's.  With W_s > 0 `acc_ssim` =
    [dssim, window positions] of the x_pred call stands beside it, advanced by two more tiny adds."""

    def __init__(self, spec: FrameLossSpec, device):
        self.spec = spec
        self.acc = torch.zeros(4, dtype=torch.float64, device=device)
        self.acc_ssim = torch.zeros(2, dtype=torch.float64, device=device) if spec.ssim != 0.0 else None
        self._ssim_row = {}
        self._tail = {}

    def fused(self, x_all, targets, S: int, B: int):
        """x_all (3 S B, C, H, W) detached - per step the calls x_pred, x_target_pred, x_pred_gp -, targets (S B, C, H, W):
        (the three terms' sums times their elements per call n - what ops.frame_losses returns for MSE - and d loss / d x_all) in
        one pass of dvg_frame_losses_ext; train.py's loss weights [0.001 / n, 1000 / n, 0.001 / n] apply to both alike.  With
        W_s > 0 a pass of dvg_frame_ssim_loss follows: it adds its gradient to d x_all and W_s (n / m) dssim to the sums."""
        n = targets[0].numel() * B
        calls, tgt = x_all.view(S, 3, B, *targets.shape[1:]), targets.view(S, B, *targets.shape[1:])
        sums, d_x = ops.frame_losses_ext(calls, tgt, self.spec, tuple(w / n for w in WEIGHTS))
        self.add(sums[0, 0], sums[1, 0], S * n)
        out = sums[0] + self.spec.gdl * sums[1] if self.spec.gdl != 0.0 else sums[0]
        if self.spec.ssim != 0.0:
            m = ssim_positions(tgt.shape[1:])
            dssim, _ = ops.frame_ssim_loss(calls, tgt, tuple(self.spec.ssim * w / m for w in WEIGHTS), dpred=d_x)
            self.add_ssim(dssim[0], S * m)
            out = out + (self.spec.ssim * n / m) * dssim
        return out, d_x

    def _term(self, x_pred, x_target, n_call, count):
        pix, gdl = torch_terms(x_pred, x_target, self.spec)
        if count:
            self.add(pix, gdl, x_target.numel())
        if self.spec.ssim == 0.0:
            return term(pix, gdl, self.spec, float(n_call))
        dssim = torch_ssim_sum(x_pred, x_target)
        if count:
            self.add_ssim(dssim, ssim_positions(x_target.shape))
        h, w = x_target.shape[-2:]
        return term(pix, gdl, self.spec, float(n_call), dssim, float(ssim_positions((n_call // (h * w), h, w))))

    def torch_calls(self, calls, targets):
        """calls (S, 3, B, C, H, W), targets (S, B, C, H, W): the terms (mse, ae_mse, mse_gp) summed over the steps, as torch ops."""
        return tuple(self._term(calls[:, k], targets, targets[0].numel(), k == 0) for k in range(3))

    def torch_step(self, running, calls, target):
        """One step of the step-by-step path: `running` (mse, ae_mse, mse_gp) plus this step's terms of `calls` (x_pred,
        x_target_pred, x_pred_gp) against `target`, as torch ops."""
        return tuple(r + self._term(x, target, target.numel(), k == 0) for k, (r, x) in enumerate(zip(running, calls)))

    @torch.no_grad()
    def add(self, pix, gdl, elements: int) -> None:
        """pix, gdl: 0-dim device tensors, sums of the x_pred call; elements: how many pixels they cover.  Three one- or two-element
        adds into `acc` (fp32 sums promoted by the add itself), no temporaries."""
        tail = self._tail.get(elements)
        if tail is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FrameTerms.add: first call for this shape during a capture (run one eager iteration first)")
            tail = self._tail[elements] = torch.tensor([1.0, float(elements)], dtype=torch.float64, device=self.acc.device)
        self.acc[0].add_(pix.detach())
        self.acc[1].add_(gdl.detach())
        self.acc[2:].add_(tail)

    @torch.no_grad()
    def add_ssim(self, dssim, positions: int) -> None:
        """dssim: a 0-dim device tensor, sum (1 - SSIM) of the x_pred call over `positions` window positions.  One one-element and
        one two-element add into `acc_ssim`, capture-safe like `add`."""
        row = self._ssim_row.get(positions)
        if row is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FrameTerms.add_ssim: first call for this shape during a capture (run one eager iteration first)")
            row = self._ssim_row[positions] = torch.tensor([0.0, float(positions)], dtype=torch.float64, device=self.acc.device)
        self.acc_ssim[0].add_(dssim.detach())
        self.acc_ssim.add_(row)

    def read_and_reset(self) -> dict:
        """{"iterations", "pixel", "gdl"}: train_model calls and the means per pixel since the last read; with W_s > 0 also "ssim",
        the mean SSIM of the x_pred call.  Reads the device.  (The step-by-step path adds once per step: its count is the steps.)"""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FrameTerms.read_and_reset: cannot read the device during a hipGraph capture")
        pix, gdl, iters, elems = self.acc.tolist()
        self.acc.zero_()
        den = max(elems, 1.0)
        d = {"iterations": int(iters), "pixel": pix / den, "gdl": gdl / den}
        if self.acc_ssim is not None:
            dssim, positions = self.acc_ssim.tolist()
            self.acc_ssim.zero_()
            d["ssim"] = 1.0 - dssim / max(positions, 1.0)
        return d

    def epoch_line(self) -> str:
        """train.py's line after the schedule's (reads the device, resets the sums)."""
        d = self.read_and_reset()
        line = '     frame loss: %s   pixel %.6g  gdl %.6g' % (self.spec.label(), d["pixel"], d["gdl"])
        return line + '  ssim %.6g' % d["ssim"] if "ssim" in d else line
