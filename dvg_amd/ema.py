"""`train.py --ema_decay D`: an exponential moving average of ALL weights, kept on the device beside the flat parameter arena and
moved once per training iteration by ONE streaming launch (dvg_ema_update, csrc/ema.hip) that is captured with the rest of the
iteration - the parameters are stepped through raw pointers inside a replayed hipGraph, where a Python-side average would never
see a step.  Semantics, the warm-up schedule and what is not averaged: docs/DESIGN_NOTES_ema.md.

Without the flag nothing here runs: `make_average` returns None - no buffer, no launch, no file, no state key."""
from __future__ import annotations

import math

import torch

from . import ops
from .train_state import detached_copy, owned_state_dict

FILE = "model_ema.pth"


def effective_decay(decay: float, k: int) -> float:
    """The decay of the update that follows `k` applied ones: min(decay, (1 + k) / (10 + k)), as the kernel forms it in fp64."""
    return min(float(decay), (1.0 + k) / (10.0 + k))


class WeightAverage:
    """Owns `e` (fp32, a clone of arena.p: make it after the parameter broadcast, so every rank starts from rank 0's values),
    `updates` (one device int32: updates applied so far) and `partials` (fp64, two sums per chunk of the last update).  All of it
    is allocated here, so the first update may already be captured in a hipGraph."""

    def __init__(self, decay: float, arena):
        decay = float(decay)
        if not 0.0 <= decay < 1.0:               # NaN fails too
            raise ValueError("WeightAverage: decay must be in [0, 1)")
        self.decay, self.arena = decay, arena
        self.e = arena.p.detach().clone()
        self.updates = torch.zeros(1, dtype=torch.int32, device=arena.p.device)
        self.partials = torch.zeros(2 * ops.ema_update_blocks(arena.p.numel()), dtype=torch.float64, device=arena.p.device)

    @torch.no_grad()
    def update(self) -> None:
        """One update over the whole arena, then the count of updates advanced by a one-element add (the kernel reads the count
        and never writes it) - on the current stream, in order, eagerly and under capture alike."""
        ops.ema_update(self.e, self.arena.p, self.decay, self.updates, self.partials)
        self.updates.add_(1)

    def read_lag(self) -> dict:
        """{"updates", "decay_eff", "lag"}: the updates applied, the decay the last of them used, and lag = |p - e| / |p| of that
        update, from its partial sums.  Reads the device (once per epoch, never inside an iteration)."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("WeightAverage.read_lag: cannot read the device during a hipGraph capture")
        s = torch.cat([self.partials.view(-1, 2).sum(0), self.updates.double()]).tolist()
        k = int(s[2])
        lag = math.sqrt(s[0]) / math.sqrt(s[1]) if s[1] > 0 else (0.0 if s[0] == 0 else math.inf)
        return {"updates": k, "decay_eff": effective_decay(self.decay, max(k - 1, 0)), "lag": lag}

    def epoch_line(self) -> str:
        """train.py's line after the gradient guard's (reads the device; every rank reads the same bits, rank 0 prints)."""
        d = self.read_lag()
        return '     ema: decay %.6g (effective %.6g)  updates %d  lag |p-ema|/|p| %.3e' % (self.decay, d["decay_eff"],
                                                                                           d["updates"], d["lag"])

    # ---- detached copies that carry the average (the live arena is never written) ---------------------------------------------
    def _averaged(self, p: torch.Tensor) -> torch.Tensor:
        """The average of the parameter `p`, a view of the live arena: `e` at its offset, as a tensor that owns its storage."""
        off, rem = divmod(p.data_ptr() - self.arena.p.data_ptr(), 4)
        if rem or off < 0 or off + p.numel() > self.e.numel() or not p.is_contiguous():
            raise RuntimeError("WeightAverage: a parameter that is no view of the arena has no average")
        return self.e[off:off + p.numel()].view(p.shape).clone()

    @torch.no_grad()
    def module_copy(self, module):
        """train_state.detached_copy(module) with every parameter taken from the average; buffers (BatchNorm statistics) are
        the live ones.  Every tensor owns its storage."""
        twin = detached_copy(module)
        for live, mine in zip(module.parameters(), twin.parameters()):
            mine.copy_(self._averaged(live))
        return twin

    @torch.no_grad()
    def state_dict_copy(self, module):
        """module.state_dict() with owned tensors: parameters from the average, buffers live."""
        sd = owned_state_dict(module.state_dict())
        for name, live in module.named_parameters():
            sd[name] = self._averaged(live)
        return sd

    def save(self, tr, path) -> None:
        """`model.pth`'s seven-key container with the averaged parameters (trainer.Trainer.save writes the live ones)."""
        torch.save({'encoder': self.module_copy(tr.encoder), 'decoder': self.module_copy(tr.decoder),
                    'frame_predictor': self.module_copy(tr.frame_predictor),
                    'likelihood': self.state_dict_copy(tr.likelihood), 'gp_layer': self.state_dict_copy(tr.gp_layer),
                    'gp_layer_optimizer': tr.optimizer.state_dict(), 'opt': tr.opt}, path)

    # ---- train_state ----------------------------------------------------------------------------------------------------------
    def state(self) -> dict:
        """{"e": an owned copy, "ema": {"decay", "updates"}} for train_state.capture (reads the count from the device)."""
        return {"e": self.e.detach().clone(), "ema": {"decay": self.decay, "updates": int(self.updates.item())}}

    @torch.no_grad()
    def load_state(self, e, meta) -> None:
        """Through the existing buffers (a captured graph holds their addresses); e = None: restart from the parameters now in
        the arena with no update applied.  The decay of THIS run applies from here on."""
        if e is None:
            self.e.copy_(self.arena.p)
            self.updates.zero_()
            return
        if e.numel() != self.e.numel():
            raise ValueError(f"WeightAverage: the saved average has {e.numel()} floats, this run's {self.e.numel()}")
        self.e.copy_(e)
        self.updates.fill_(int(meta["updates"]))


# ---- train.py's calls ------------------------------------------------------------------------------------------------------------
def add_arguments(parser) -> None:
    parser.add_argument('--ema_decay', default=None, type=float, metavar='D',   # docs/DESIGN_NOTES_ema.md
                        help='keep an exponential moving average of all weights, updated once per iteration on the device with '
                             'decay min(D, (1 + k) / (10 + k)) after k updates; written to model_ema.pth beside model.pth '
                             '(generate_frames.py --ema reads it); D in [0, 1), default: no average')


def ema_options(opt):
    """The decay train.py's --ema_decay asks for, None without the flag (an options object from before it has no such attribute).
    Host only."""
    d = getattr(opt, "ema_decay", None)
    if d is None:
        return None
    d = float(d)
    if not 0.0 <= d < 1.0:
        raise SystemExit("train.py: --ema_decay must be in [0, 1)")
    return d


def make_average(opt, arena):
    """The WeightAverage the options ask for; None - no buffer, no launch - without the flag."""
    d = ema_options(opt)
    return None if d is None else WeightAverage(d, arena)


def print_checksums(tr, rank) -> None:
    """train.py --print_param_checksum (multi-rank tests: every rank must agree): the sum and the absolute sum of all parameters,
    and of the weight average when there is one."""
    ps = [p.detach().double() for m in tr.modules for p in m.parameters()]
    print('rank %d param checksum %.17g %.17g' % (rank, sum(float(p.sum()) for p in ps), sum(float(p.abs().sum()) for p in ps)),
          flush=True)
    if tr.ema is not None:
        e = tr.ema.e.double()
        print('rank %d ema checksum %.17g %.17g updates %d' % (rank, float(e.sum()), float(e.abs().sum()), int(tr.ema.updates)),
              flush=True)


def checkpoint_path(model_dir: str, dataset: str) -> str:
    """generate_frames.py --ema: `<model_dir>/<dataset>_ema.pth`, else `<model_dir>/model_ema.pth`."""
    import os
    first, second = '%s/%s_ema.pth' % (model_dir, dataset), '%s/%s' % (model_dir, FILE)
    for path in (first, second):
        if os.path.exists(path):
            return path
    raise SystemExit(f"generate_frames.py --ema: neither {first} nor {second} exists (train.py --ema_decay writes the latter)")
