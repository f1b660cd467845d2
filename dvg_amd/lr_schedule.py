"""`train.py --lr_schedule KIND`: a learning-rate multiplier that moves EVERY ITERATION, kept on the device.  An iteration is a
replayed hipGraph whose Adam launches have their arguments baked in, and a re-capture per change of `param_groups[...]['lr']`
(train_graphs.GraphedIteration) rebuilds a pool of many GB: fine for the GP optimiser's two MultiStepLR milestones, not for a
warm-up or a decay.  So ONE single-thread launch at the top of the iteration (dvg_lr_schedule_tick, csrc/lr_schedule.hip) writes
the multiplier of this iteration into one device float, and every Adam launch of the iteration reads it
(dvg_adam_step_scheduled): the rate of a launch is `param_groups[...]['lr']` - the base rate, `--lr`, for the GP group times its
MultiStepLR factor - times the multiplier.  Semantics, and what is not done: docs/DESIGN_NOTES_lr_schedule.md.

Without the flag nothing here runs: `make_schedule` returns None - no buffer, no launch, no state key, no log line - and the
optimisers keep the literal 0.002 of the reference and their unscheduled kernels."""
from __future__ import annotations

import math

import torch

from . import ops

KINDS = ops.LR_KINDS
SPEC_FIELDS = ("kind", "warmup", "total", "min_ratio", "step_every", "gamma", "lr")
REFERENCE_LR = 0.002       # the reference's train.py:95-104; what every optimiser gets without a schedule
INT_MAX = 2 ** 31 - 1


def multiplier(spec: dict, k: int) -> float:
    """s(k), the multiplier of the iteration that follows `k` completed ones, in fp64 with the kernel's operations in the kernel's
    order (the tests' restatement is tests/lr_schedule_ref.py)."""
    W, N, R = spec["warmup"], spec["total"], spec["min_ratio"]
    if k < W:
        return (k + 1.0) / W
    u = min(1.0, float(k - W) / float(max(1, N - W)))
    if spec["kind"] == "linear":
        return R + (1.0 - R) * (1.0 - u)
    if spec["kind"] == "cosine":
        return R + (1.0 - R) * (0.5 * (1.0 + math.cos(math.pi * u)))
    if spec["kind"] == "step":
        return max(R, math.pow(spec["gamma"], float((k - W) // spec["step_every"])))
    return 1.0


class SpecError(ValueError):
    """A field of a spec that dvg_lr_schedule_tick would refuse (or a base rate that is no rate): `.field` names it."""

    def __init__(self, field: str, what: str):
        super().__init__(f"{field} {what}")
        self.field = field


def check_spec(spec: dict) -> dict:
    """The spec with plain values, or a SpecError."""
    s = {"kind": spec["kind"], "warmup": int(spec["warmup"]), "total": int(spec["total"]), "min_ratio": float(spec["min_ratio"]),
         "step_every": int(spec["step_every"]), "gamma": float(spec["gamma"]), "lr": float(spec["lr"])}
    if s["kind"] not in KINDS:
        raise SpecError("kind", f"must be one of {', '.join(KINDS)}")
    if not 0.0 <= s["lr"] < math.inf:                    # NaN fails too
        raise SpecError("lr", "must be a finite rate >= 0")
    if s["warmup"] < 0:
        raise SpecError("warmup", "must be >= 0")
    if not s["warmup"] < s["total"] <= INT_MAX:
        raise SpecError("total", "must be above the warm-up (and below 2^31)")
    if not 0.0 <= s["min_ratio"] <= 1.0:
        raise SpecError("min_ratio", "must be in [0, 1]")
    if s["kind"] == "step" and s["step_every"] < 1:
        raise SpecError("step_every", "must be >= 1")
    if s["kind"] == "step" and not 0.0 < s["gamma"] <= 1.0:
        raise SpecError("gamma", "must be in (0, 1]")
    return s


class LrSchedule:
    """Owns `iters` (one device int32: iterations completed) and `scale` (one device fp32: the multiplier the Adam launches read,
    s(0) until the first tick).  Both are allocated here, so the first tick may already be captured in a hipGraph, and neither
    ever changes its address: a captured graph holds them.  `spec`: SPEC_FIELDS as plain values; the fields `step_every` and
    `gamma` are 1 and 1.0 unless the kind is `step`."""

    def __init__(self, spec: dict, device):
        self.spec = check_spec(spec)
        self.iters = torch.zeros(1, dtype=torch.int32, device=device)
        self.scale = torch.full((1,), multiplier(self.spec, 0), dtype=torch.float32, device=device)
        self.optimizers = []

    def attach(self, optimizers) -> None:
        """Every step of `optimizers` (FusedAdam) from now on runs at its group's rate times `scale`."""
        self.optimizers = list(optimizers)
        for o in self.optimizers:
            o.lr_scale = self.scale

    def tick(self) -> None:
        """The first launch of an iteration: scale = s(iters), iters += 1 - on the current stream, eagerly and under capture
        alike.  Every step site of the iteration then reads the one value."""
        s = self.spec
        ops.lr_schedule_tick(s["kind"], s["warmup"], s["total"], s["step_every"], s["min_ratio"], s["gamma"], self.iters, self.scale)

    def read(self) -> dict:
        """{"iters", "scale"}: iterations completed and the multiplier the last of them ran at (s(0) before the first).  Reads
        the device: once per epoch, never inside an iteration."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("LrSchedule.read: cannot read the device during a hipGraph capture")
        k, s = torch.cat([self.iters.double(), self.scale.double()]).tolist()
        return {"iters": int(k), "scale": s}

    def epoch_line(self) -> str:
        """train.py's line after the weight average's (reads the device): kind, k / N, the multiplier, and the rates the last
        iteration's steps ran at - base rate x multiplier per optimiser group, the GP groups' MultiStepLR factor included."""
        d = self.read()
        rates = sorted({float(g["lr"]) * d["scale"] for o in self.optimizers for g in o.param_groups}, reverse=True)
        return '     lr schedule: %s  iteration %d / %d  multiplier %.6g  rates %s' % (
            self.spec["kind"], d["iters"], self.spec["total"], d["scale"], ' '.join('%.4g' % r for r in rates))

    # ---- train_state ----------------------------------------------------------------------------------------------------------
    def state(self) -> dict:
        """{"spec", "iters"} for train_state.capture (reads the count from the device)."""
        return {"spec": dict(self.spec), "iters": int(self.iters.item())}

    @torch.no_grad()
    def load_state(self, iters: int) -> None:
        """Through the existing buffers: `iters` iterations are done; the scale is what the next one will run at, until its tick
        writes the same."""
        k = min(max(int(iters), 0), INT_MAX)
        self.iters.fill_(k)
        self.scale.fill_(multiplier(self.spec, k))


def spec_mismatch(saved: dict, now: dict):
    """The first field of a saved spec that differs from this run's, as (field, saved value, this run's), or None."""
    for f in SPEC_FIELDS:
        if saved.get(f) != now[f]:
            return f, saved.get(f), now[f]
    return None


def restore(schedule, sd: dict, path: str, global_step: int, rank: int = 0, restored_lr=None) -> None:
    """train_state.restore's part: `sd` is the whole state (plain values under "lr_schedule", or no such key); `restored_lr`: the
    base rate the optimisers have just taken from the state."""
    saved = sd.get("lr_schedule")
    if schedule is None:
        if saved is not None and rank == 0:
            print(f"{path}: the learning-rate schedule in the file is ignored: this run has no --lr_schedule", flush=True)
        return
    bad = spec_mismatch(saved["spec"], schedule.spec) if saved is not None else None
    if saved is None and restored_lr is not None and float(restored_lr) != schedule.spec["lr"]:
        bad = ("lr", float(restored_lr), schedule.spec["lr"])       # the optimisers' rate IS state: --lr cannot change it here
    if bad is not None:
        raise SystemExit(f"train.py --resume: {path}: lr_schedule.{bad[0]} is {bad[1]!r} in the file and {bad[2]!r} in this run")
    if saved is None:
        schedule.load_state(global_step)
        if rank == 0:
            print(f"{path}: no learning-rate schedule in the file: --lr_schedule counts from global step {int(global_step)}",
                  flush=True)
        return
    schedule.load_state(saved["iters"])


# ---- train.py's calls ------------------------------------------------------------------------------------------------------------
def add_arguments(parser) -> None:
    g = parser.add_argument     # docs/DESIGN_NOTES_lr_schedule.md
    g('--lr_schedule', default=None, choices=KINDS, metavar='KIND',
      help='move the learning rate of all four optimisers every iteration, on the device (also inside a hipGraph): --lr times a '
           'multiplier that rises linearly over --lr_warmup iterations and then stays (constant), falls linearly or along a half '
           'cosine to --lr_min_ratio at iteration --lr_total (linear, cosine), or is multiplied by --lr_gamma every --lr_step_every '
           'iterations (step); the GP optimiser\'s epoch milestones multiply with it; default: no schedule, every rate 0.002')
    g('--lr_warmup', default=None, type=int, metavar='W', help='--lr_schedule: warm-up iterations (default 0)')
    g('--lr_total', default=None, type=int, metavar='N', help='--lr_schedule: the iteration the decay ends at (default niter * epoch_size)')
    g('--lr_min_ratio', default=None, type=float, metavar='R', help='--lr_schedule: the floor of the multiplier, in [0, 1] (default 0)')
    g('--lr_step_every', default=None, type=int, metavar='K', help='--lr_schedule step: iterations per step (default epoch_size)')
    g('--lr_gamma', default=None, type=float, metavar='G', help='--lr_schedule step: the factor of a step, in (0, 1] (default 0.5)')


_OPTION_OF = {"warmup": "--lr_warmup", "total": "--lr_total", "min_ratio": "--lr_min_ratio", "step_every": "--lr_step_every",
              "gamma": "--lr_gamma", "lr": "--lr", "kind": "--lr_schedule"}


def schedule_options(opt):
    """The spec train.py's --lr_schedule and its companions ask for, None without the flag (an options object from before it has
    no such attribute).  Every invalid value, and a companion without the flag it belongs to, ends with a SystemExit that names the
    option.  Host only."""
    def get(name):
        return getattr(opt, name, None)
    kind = get("lr_schedule")
    if kind is None:
        for name in ("lr_warmup", "lr_total", "lr_min_ratio", "lr_step_every", "lr_gamma"):
            if get(name) is not None:
                raise SystemExit(f"train.py: --{name} needs --lr_schedule")
        return None
    if kind != "step":
        for name in ("lr_step_every", "lr_gamma"):
            if get(name) is not None:
                raise SystemExit(f"train.py: --{name} needs --lr_schedule step")
    step = kind == "step"
    spec = {"kind": kind, "warmup": 0 if get("lr_warmup") is None else get("lr_warmup"),
            "total": int(opt.niter) * int(opt.epoch_size) if get("lr_total") is None else get("lr_total"),
            "min_ratio": 0.0 if get("lr_min_ratio") is None else get("lr_min_ratio"),
            "step_every": 1 if not step else int(opt.epoch_size) if get("lr_step_every") is None else get("lr_step_every"),
            "gamma": 1.0 if not step else 0.5 if get("lr_gamma") is None else get("lr_gamma"), "lr": opt.lr}
    try:
        return check_spec(spec)
    except SpecError as e:
        raise SystemExit(f"train.py: {_OPTION_OF[e.field]}: {e}") from None


def base_rate(opt) -> float:
    """The `lr` train.py builds its four optimisers with: --lr under a schedule or with an --optimizer other than adam, else the
    reference's literal 0.002 (--lr stays unused, so no existing command line changes its result)."""
    plain = getattr(opt, "lr_schedule", None) is None and getattr(opt, "optimizer", "adam") == "adam"
    return REFERENCE_LR if plain else float(opt.lr)


def make_schedule(opt, device, optimizers=()):
    """The LrSchedule the options ask for, attached to `optimizers`; None - no buffer, no launch - without the flag."""
    spec = schedule_options(opt)
    if spec is None:
        return None
    schedule = LrSchedule(spec, device)
    schedule.attach(optimizers)
    return schedule
