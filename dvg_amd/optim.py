"""Fused multi-tensor Adam for the four optimisers of train.py:95-106.

`FusedAdam(params, lr=...)` is a `torch.optim.Optimizer` with torch.optim.Adam's arithmetic (non-amsgrad) and
state layout (`step`, `exp_avg`, `exp_avg_sq` per parameter, so `state_dict()` is interchangeable with
torch.optim.Adam's and `MultiStepLR` drives `param_groups[...]['lr']` as in train.py:105-106), but every
parameter group lives in ONE flat fp32 buffer: parameters are re-pointed at views of it, the moments are views of
two more, the GRADIENTS are views of a fourth (`p.grad` is set to its view, so backward accumulates straight into
the flat buffer) and a step is ONE `dvg_adam_step` launch per group.

`FlatArena`: several optimisers can carve their groups out of one shared arena (trainer.Trainer does: GP, likelihood,
LSTM, decoder, encoder in that order), so that the data-parallel gradient all-reduce (dvg_amd/parallel.py) runs on
contiguous ranges of ONE buffer - no gather into a communication buffer, no scatter back, no copy into the
optimiser's buffer.

`FusedOptimizer` is what is not Adam's in that; `FusedAdamW`, `FusedSGD` and `FusedRMSprop` (train.py --optimizer) are the other
rules of dvg_optim_step, each with the state layout of torch.optim's class of its name, and a group of any of the four may carry a
`decay_mask` (train.py --weight_decay; docs/DESIGN_NOTES_optimizers.md).
"""
from __future__ import annotations

from typing import List, Optional

import torch

from . import ops
from ._lib import check, lib


class FlatArena:
    """Four flat fp32 buffers (param, grad, exp_avg, exp_avg_sq) of `numel` floats; `alloc` hands out ranges."""

    def __init__(self, numel: int, device):
        self.p = torch.zeros(numel, device=device)
        self.g = torch.zeros(numel, device=device)
        self.m = torch.zeros(numel, device=device)
        self.v = torch.zeros(numel, device=device)
        self.used = 0

    @staticmethod
    def padded(n: int) -> int:
        return (n + 3) // 4 * 4          # every view 16-byte aligned

    @classmethod
    def size_for(cls, params) -> int:
        return sum(cls.padded(p.numel()) for p in params if p.requires_grad)

    def alloc(self, n: int) -> int:
        if self.used + n > self.p.numel():
            raise RuntimeError("FlatArena: out of space")
        off, self.used = self.used, self.used + n
        return off


def flat_offsets(params):
    """(offsets, n): where each parameter starts in its group's flat range and the range's length; every view padded to 4 floats."""
    offs, n = [], 0
    for p in params:
        offs.append(n)
        n += FlatArena.padded(p.numel())
    return offs, n


class FusedOptimizer(torch.optim.Optimizer):
    """What the fused optimisers share: the flat storage and its arena ranges, the gradient views, the hipGraph bookkeeping, the
    skip counters, the host half of the state, the version bumps and `lr_scale`.  A rule names its two state buffers (M_NAME,
    V_NAME: the keys of torch's class; V_NAME None = the second buffer is unused), says which keys of a parameter's state its
    torch class has (_export) and launches its step (_launch).  Every parameter's state keeps a `step` count here whatever the
    torch layout says: the capture protocol and train_state.global_step read it."""
    RULE = None
    M_NAME, V_NAME = "exp_avg", "exp_avg_sq"

    def __init__(self, params, defaults, arena: Optional[FlatArena] = None):
        super().__init__(params, defaults)
        self.arena = arena
        self._flat = {}   # group index -> dict(p, g, m, v, params, offsets, gviews, tdev, lo, hi)
        self._captured_groups = []   # groups stepped while a hipGraph was being captured (see after_graph_replay)
        self._graph_stale = False    # an eager step() or a restored state since that capture (see begin_capture)
        # one device fp32 (an lr_schedule.LrSchedule's multiplier) every launch of step() multiplies its group's rate with, read on
        # the device (dvg_adam_step_scheduled); None: the rate is param_groups[...]['lr'] and the launches are the unscheduled ones
        self.lr_scale: Optional[torch.Tensor] = None
        if all(p.is_cuda for g in self.param_groups for p in g["params"]):
            for gi, group in enumerate(self.param_groups):   # flat storage right away: p.grad are views from the start
                self._build(gi, group)

    # ---- flat storage -------------------------------------------------------------------------------
    def _build(self, gi: int, group) -> dict:
        params: List[torch.nn.Parameter] = [p for p in group["params"] if p.requires_grad]
        if not params:
            return {}
        dev = params[0].device
        for p in params:
            if p.dtype != torch.float32 or p.device != dev:
                raise RuntimeError(f"{type(self).__name__}: parameters of a group must be fp32 on one device")
        offs, n = flat_offsets(params)
        if self.arena is not None:
            lo = self.arena.alloc(n)
            a = self.arena
            flat_p, flat_g, flat_m, flat_v = (t[lo:lo + n] for t in (a.p, a.g, a.m, a.v))
        else:
            lo = 0
            flat_p = torch.zeros(n, device=dev)
            flat_m, flat_v, flat_g = torch.zeros_like(flat_p), torch.zeros_like(flat_p), torch.zeros_like(flat_p)
        steps = {}
        with torch.no_grad():
            for p, o in zip(params, offs):
                view = flat_p[o:o + p.numel()].view(p.shape)
                view.copy_(p)
                st = self.state.get(p, {})
                if st:                              # state restored by load_state_dict
                    self._import(st, flat_m[o:o + p.numel()], flat_v[o:o + p.numel()])
                    steps[p] = float(st.get("step", 0.0))
                p.data = view                       # the module keeps the same Parameter object
        f = dict(p=flat_p, g=flat_g, m=flat_m, v=flat_v, params=params, offsets=offs, lo=lo, hi=lo + n,
                 tdev=torch.zeros(1, dtype=torch.int32, device=dev),     # device-side step count of the group
                 gviews=[flat_g[o:o + p.numel()].view(p.shape) for p, o in zip(params, offs)])
        for p, o, gv in zip(params, offs, f["gviews"]):
            self.state[p] = self._state_views(steps.get(p, 0.0), flat_m, flat_v, p, o)
            if p.grad is not None:
                gv.copy_(p.grad)
            p.grad = gv                             # backward accumulates into the flat gradient buffer
        self._flat[gi] = f
        return f

    def _state_views(self, step, flat_m, flat_v, p, o) -> dict:
        st = {"step": torch.tensor(float(step)), self.M_NAME: flat_m[o:o + p.numel()].view(p.shape)}
        if self.V_NAME is not None:
            st[self.V_NAME] = flat_v[o:o + p.numel()].view(p.shape)
        return st

    def _import(self, st, m, v) -> None:
        """A parameter's state in the torch layout (load_state_dict) into its flat ranges; a buffer the state lacks - torch's SGD
        and RMSprop without momentum keep none - is zero."""
        for name, dst in ((self.M_NAME, m), (self.V_NAME, v)):
            if name is None:
                continue
            if torch.is_tensor(st.get(name)):
                dst.copy_(st[name].reshape(-1))
            else:
                dst.zero_()

    def _export(self, group, st: dict) -> dict:
        """A parameter's state as the torch class of this rule lays it out (state_dict)."""
        return st

    def flat_range(self, gi: int = 0):
        """(lo, hi) of group `gi` in the arena (or in its own flat buffer)."""
        f = self._flat[gi]
        return f["lo"], f["hi"]

    def flat_grad(self, gi: int = 0) -> torch.Tensor:
        return self._flat[gi]["g"]

    def state_dict(self):
        """torch.optim layout, but every per-parameter tensor is a COPY that owns its storage: `exp_avg` / `exp_avg_sq` are
        views of the flat moment buffers (of the shared arena under trainer.Trainer), and torch.save writes the whole storage
        behind a view - the GP optimiser's entry of a checkpoint (train.py:385) would carry the Adam moments of every
        module (+2 x all parameter bytes)."""
        self.sync_step_counts()
        sd = super().state_dict()
        group_of = {k: g for g in sd["param_groups"] for k in g["params"]}
        sd["state"] = {k: {n: (t.detach().clone() if torch.is_tensor(t) else t) for n, t in self._export(group_of[k], st).items()}
                       for k, st in sd["state"].items()}
        sd["state"] = {k: st for k, st in sd["state"].items() if st}     # torch keeps no entry for a parameter without state
        sd["param_groups"] = [{k: v for k, v in g.items() if k != "decay_mask"} for g in sd["param_groups"]]
        return sd

    def load_state_dict(self, state_dict):
        masks = [g.get("decay_mask") for g in self.param_groups]        # not state: a torch class's state dict has none
        counts = {p: float(st["step"]) for p, st in self.state.items() if "step" in st}
        super().load_state_dict(state_dict)
        for g, mask in zip(self.param_groups, masks):
            if mask is not None:
                g["decay_mask"] = mask
        for p, st in self.state.items():         # a layout without `step` (torch.optim.SGD): the counts held until now stay
            if st:
                st.setdefault("step", counts.get(p, 0.0))
        # torch aliases (does not copy) the tensors of `state_dict`: copy them into our flat buffers right away
        if self.arena is not None and self._flat:
            for gi, f in self._flat.items():     # arena ranges are already ours: refresh moments / steps in place
                for p, o in zip(f["params"], f["offsets"]):
                    st = self.state[p]
                    self._import(st, f["m"][o:o + p.numel()], f["v"][o:o + p.numel()])
                    self.state[p] = self._state_views(float(st.get("step", counts.get(p, 0.0))), f["m"], f["v"], p, o)
                if "skips" in f:
                    f["skips"].zero_()           # the loaded counts are counts of applied steps (as load_host_state)
            return
        self._flat.clear()
        for gi, group in enumerate(self.param_groups):
            self._build(gi, group)

    # ---- the host half of the state (train_state: the tensors are saved as whole arena buffers) ----------------------
    def host_state(self) -> dict:
        """Per group the hyper-parameters and the per-parameter step counts, as plain numbers."""
        self.sync_step_counts()
        return {"param_groups": [{k: v for k, v in g.items() if k not in ("params", "decay_mask")} for g in self.param_groups],
                "steps": [[int(self.state[p]["step"]) for p in g["params"] if p.requires_grad] for g in self.param_groups]}

    def load_host_state(self, hs: dict) -> None:
        """The inverse of host_state(); parameters, gradients and moments are not touched (the caller wrote the arena).  A
        captured graph's device step counts no longer describe this state: the graph is marked stale (check_graph_fresh raises
        until begin_capture seeds `tdev` from the restored counts)."""
        if len(hs["param_groups"]) != len(self.param_groups):
            raise ValueError(f"{type(self).__name__}: another number of parameter groups")
        for g, saved, steps in zip(self.param_groups, hs["param_groups"], hs["steps"]):
            params = [p for p in g["params"] if p.requires_grad]
            if len(steps) != len(params):
                raise ValueError(f"{type(self).__name__}: another number of parameters in a group")
            for k, v in saved.items():
                g[k] = tuple(v) if k == "betas" else v
            for p, t in zip(params, steps):
                self.state[p]["step"] = torch.tensor(float(t))
        for f in self._flat.values():
            if f:
                f.pop("ticked", None)
                if "skips" in f:
                    f["skips"].zero_()           # the restored counts are counts of applied steps
                self._restore_grad_views(f)
        if self._captured_groups:
            self._graph_stale = True

    @torch.no_grad()
    def zero_grad(self, set_to_none: bool = False):
        """One fill per group; `p.grad` stays (or becomes again) the view of the flat gradient buffer.  Unlike
        torch.optim the default is set_to_none=False: a None gradient makes autograd allocate a fresh tensor per parameter
        and step() copy it back into the flat buffer (still correct - and it keeps torch.optim.Adam's "a parameter without
        a gradient is skipped" semantics, which is why set_to_none=True is honoured when asked for)."""
        for gi, group in enumerate(self.param_groups):
            f = self._flat.get(gi)
            if not f or set_to_none:
                for p in group["params"]:
                    p.grad = None
                continue
            f["g"].zero_()
            for p, gv in zip(f["params"], f["gviews"]):
                if p.grad is not gv:
                    p.grad = gv

    def _restore_grad_views(self, f) -> None:
        for p, gv in zip(f["params"], f["gviews"]):
            if p.grad is not gv:
                p.grad = gv

    # ---- hipGraph support -------------------------------------------------------------------------------
    def begin_capture(self) -> None:
        """Call right before capturing a graph that contains step(): the device step counts are synchronised with the
        host ones (the captured kernels then increment and read them on the device).
        INVARIANT: the device counts `tdev` are valid only from here through the replays of the graph captured
        next.  An EAGER step() in between advances the host count only (it passes the count as an argument), so a replay
        after it would apply stale bias corrections: step() marks the captured graph stale and after_graph_replay() raises.
        Re-capture (begin_capture again) to continue with graphs after eager steps."""
        self.sync_step_counts()      # guarded steps that were skipped: the host counts become the counts of applied steps
        self._captured_groups = []
        self._graph_stale = False
        for gi, f in self._flat.items():
            if f:
                f.pop("ticked", None)
                f["tdev"].fill_(int(self.state[f["params"][0]]["step"]))

    def end_capture(self) -> None:
        """Call after the capture: every group whose device step count a captured zero_grads() launch advanced (`ticked`)
        must also have been stepped inside the same capture - otherwise each replay would advance the count without a step
        and later bias corrections would be wrong without any error."""
        for gi, f in self._flat.items():
            if f and f.pop("ticked", False):
                raise RuntimeError(f"{type(self).__name__}: group {gi} had its device step count advanced by a captured zero_grads() "
                                   "but was not stepped in the same capture")

    def check_graph_fresh(self) -> None:
        """Call BEFORE replaying a captured graph: raises when an eager step() ran since the capture (nothing has executed yet)."""
        if self._graph_stale and self._captured_groups:
            raise RuntimeError(f"{type(self).__name__}: an eager step() ran since the graph was captured: its device-side step counts are "
                               "stale (a replay would apply wrong Adam bias corrections).  Re-capture after eager steps.")

    def after_graph_replay(self) -> None:
        """The replayed kernels stepped the parameters through raw pointers: advance the host-side step counts (state_dict,
        torch.optim compatibility) and the version counters the packed-weight caches key on.  Raises when an eager step()
        ran since the capture (see begin_capture: the replay just applied stale bias corrections)."""
        if self._graph_stale and self._captured_groups:
            raise RuntimeError(f"{type(self).__name__}: a captured graph was replayed after an eager step(): its device-side step counts "
                               "are stale (wrong Adam bias corrections were applied).  Re-capture after eager steps.")
        for gi in self._captured_groups:
            for p in self._flat[gi]["params"]:
                torch.autograd.graph.increment_version(p)
                self.state[p]["step"] += 1

    # ---- step ---------------------------------------------------------------------------------------
    def _skips(self, f) -> torch.Tensor:
        """The group's device-side count of guarded steps that were skipped since the last sync_step_counts(); made on the
        first guarded step (an optimiser that is never guarded owns no such tensor)."""
        if "skips" not in f:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{type(self).__name__}: the first guarded step of a group cannot be inside a hipGraph capture "
                                   "(GradGuard.attach the optimisers, or run one eager guarded step, first)")
            f["skips"] = torch.zeros(1, dtype=torch.int32, device=f["p"].device)
        return f["skips"]

    def sync_step_counts(self) -> None:
        """A guarded step that was skipped (dvg_adam_step_guarded: non-finite gradients under GradGuard.skip_nonfinite) touched
        nothing, but its step had already been counted: by the zero_grads() tick on the device, by step() / after_graph_replay()
        on the host.  The kernel corrects for that with the group's `skips` counter; here the counter is read (ONE
        synchronisation for all groups, never inside an iteration), subtracted from the host counts - and from the device
        count a captured graph holds - and zeroed, so that state_dict() / host_state() save the number of steps applied.
        Does nothing, and does not synchronise, for an optimiser that was never stepped with a guard."""
        fl = [(gi, f) for gi, f in self._flat.items() if f and "skips" in f]
        if not fl:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{type(self).__name__}.sync_step_counts: cannot read the skip counters during a hipGraph capture")
        ks = torch.cat([f["skips"] for _, f in fl]).tolist()
        for (gi, f), k in zip(fl, ks):
            if not k:
                continue
            for p in f["params"]:
                self.state[p]["step"] -= k
            if gi in self._captured_groups:
                f["tdev"].sub_(k)
            f["skips"].zero_()

    def _adopt_stray_grads(self, f) -> None:
        """Gradients normally ARE the views of the flat buffer; one that was re-created (module.zero_grad() sets None) is
        copied in and `p.grad` re-pointed."""
        stray = [(gv, p.grad) for p, gv in zip(f["params"], f["gviews"])
                 if p.grad is not gv and p.grad.data_ptr() != gv.data_ptr()]
        if stray:
            torch._foreach_copy_([s[0] for s in stray], [s[1] for s in stray])
            for p, gv in zip(f["params"], f["gviews"]):
                p.grad = gv

    def _groups_with_grads(self):
        """(gi, group, flat record, [parameter has a gradient]) for every group that has gradients; a group whose parameters
        changed since its flat record was made is rebuilt first."""
        for gi, group in enumerate(self.param_groups):
            f = self._flat.get(gi)
            if f is None or [id(p) for p in f.get("params", [])] != [id(p) for p in group["params"] if p.requires_grad]:
                if self.arena is not None and f is not None:
                    raise RuntimeError(f"{type(self).__name__}: the parameters of an arena-backed group cannot change")
                f = self._build(gi, group)
            if not f:
                continue
            have = [p.grad is not None for p in f["params"]]
            if any(have):
                yield gi, group, f, have

    @torch.no_grad()
    def guard_spans(self):
        """What a guarded step of this optimiser is about to apply: (arena or None, lo, hi, flat gradient) per group that has
        gradients, with every gradient in its flat buffer.  A partially used group raises: the guard's norm is taken over whole
        flat ranges, and the per-parameter launches of step() have no guarded form."""
        spans = []
        for gi, group, f, have in self._groups_with_grads():
            if not all(have) or len({int(self.state[p]["step"]) for p in f["params"]}) != 1:
                raise RuntimeError(f"{type(self).__name__}: group {gi} is partially used (parameters without a gradient, or with different "
                                   "step counts): it cannot be stepped with a gradient guard")
            self._adopt_stray_grads(f)
            self._skips(f)
            spans.append((self.arena, f["lo"], f["hi"], f["g"]))
        return spans

    @torch.no_grad()
    def step(self, closure=None, guard=None):
        """`guard`: a GradGuard whose `stat` the launches of this call obey (guarded_step has just filled it)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group, f, have in self._groups_with_grads():
            steps = {int(self.state[p]["step"]) for p in f["params"]}
            capturing = torch.cuda.is_current_stream_capturing()
            if all(have) and len(steps) == 1:
                # the whole group in one launch; the step count lives on the device so that a captured hipGraph
                # (train.GraphedIteration) applies fresh bias corrections at every replay.
                self._adopt_stray_grads(f)
                t = steps.pop() + 1
                if capturing:
                    # the count lives on the device (begin_capture synchronised it): advanced by the zero_grads() launch of
                    # this capture when there was one since the group's last step, else by a one-element add
                    if not f.pop("ticked", False):
                        f["tdev"].add_(1)
                    tdev = f["tdev"]
                else:
                    tdev = None                      # eager: the host count goes in as an argument, no device-side bookkeeping
                    f.pop("ticked", None)
                    if gi in self._captured_groups:  # a captured graph holds this group's device count: now behind the host's
                        self._graph_stale = True
                stat, skips = (None, None) if guard is None else (guard.stat, self._skips(f))
                self._launch(group, f["p"], f["g"], f["m"], f["v"], group.get("decay_mask"), t, tdev, stat, skips)
                touched = f["params"]
                if capturing:
                    self._captured_groups.append(gi)
            else:
                # torch.optim semantics for a partially used group: parameters without a gradient are skipped
                # (no moment decay, no step count) - one launch per parameter that has one
                if capturing:
                    raise RuntimeError(f"{type(self).__name__}: a partially used parameter group cannot be captured in a hipGraph")
                if guard is not None:
                    raise RuntimeError(f"{type(self).__name__}: group {gi} is partially used: it cannot be stepped with a gradient guard")
                touched = [p for p in f["params"] if p.grad is not None]
                mask = group.get("decay_mask")
                for p, gv, o in zip(f["params"], f["gviews"], f["offsets"]):
                    if p.grad is None:
                        continue
                    st = self.state[p]
                    if p.grad is not gv and p.grad.data_ptr() != gv.data_ptr():
                        gv.copy_(p.grad)
                    self._launch(group, p, gv, st[self.M_NAME], st[self.V_NAME] if self.V_NAME is not None else None,
                                 None if mask is None else mask[o // 4:(o + p.numel() + 3) // 4], int(st["step"]) + 1, None, None, None)
            for p in touched:
                # the kernel wrote through raw pointers; also while capturing, so that code captured AFTER this step
                # re-packs its weights instead of reusing the packs from before the step
                torch.autograd.graph.increment_version(p)
                if not capturing:                # a capture executes nothing: after_graph_replay() counts the replays
                    self.state[p]["step"] += 1
        return loss

    def _launch(self, group, p, g, m, v, mask, t, tdev, stat, skips) -> None:
        """One launch of the rule over p, g, m, v (a flat group or one parameter's views) with the group's hyper-parameters."""
        raise NotImplementedError

    def set_decay_mask(self, gi: int, mask: Optional[torch.Tensor]) -> None:
        """`mask`: one uint8 per 16-byte piece of group `gi`'s flat range, on its device; 0 = the piece does not decay.  None
        takes the mask away: every piece decays by the group's weight_decay."""
        f = self._flat[gi]
        if mask is not None and (mask.dtype != torch.uint8 or mask.numel() != (f["hi"] - f["lo"]) // 4 or mask.device != f["p"].device):
            raise ValueError(f"{type(self).__name__}: decay_mask of group {gi} must be {(f['hi'] - f['lo']) // 4} uint8 on {f['p'].device}")
        if mask is None:
            self.param_groups[gi].pop("decay_mask", None)
        else:
            self.param_groups[gi]["decay_mask"] = mask.contiguous()

    def hyper_mismatch(self, hs: dict):
        """The first hyper-parameter of a saved host_state() that is not this optimiser's, as (field, saved, this run's), or None.
        The rates are not compared: schedulers move them, and the restored ones hold."""
        for gi, (g, saved) in enumerate(zip(self.param_groups, hs["param_groups"])):
            for k in HYPER_FIELDS:
                if k in g or k in saved:
                    a, b = saved.get(k), g.get(k)
                    a, b = (list(a) if isinstance(a, (list, tuple)) else a), (list(b) if isinstance(b, (list, tuple)) else b)
                    if a != b:
                        return (k if len(self.param_groups) == 1 else f"{k}[{gi}]"), saved.get(k), g.get(k)
        return None


HYPER_FIELDS = ("betas", "eps", "weight_decay", "momentum", "nesterov", "alpha")


def _check_hyper(cls, **kw) -> None:
    for k, v in kw.items():
        vs = v if isinstance(v, (tuple, list)) else (v,)
        if any(x != x or x < 0 for x in vs) or (k in ("betas", "alpha") and any(x >= 1 for x in vs)):
            raise ValueError(f"{cls.__name__}: invalid hyper-parameter {k}={v!r}")


class FusedAdam(FusedOptimizer):
    """torch.optim.Adam.  Constructed without a decay mask it issues the launches it always did (dvg_adam_step, _guarded,
    _scheduled); a group that carries `decay_mask` goes through rule 0 of dvg_optim_step, the same arithmetic."""
    RULE = ops.ADAM

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, arena: Optional[FlatArena] = None):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError(f"{type(self).__name__}: invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), arena)

    def _launch(self, group, p, g, m, v, mask, t, tdev, stat, skips) -> None:
        b1, b2 = group["betas"]
        hyper = (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]))
        if mask is None and self.RULE == ops.ADAM:
            ops.adam_step(p, g, m, v, *hyper, t, tdev, stat, skips, self.lr_scale)
        else:
            ops.optim_step(self.RULE, p, g, m, v, *hyper, 0, mask, t, tdev, stat, skips, self.lr_scale)


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW: the decay leaves the gradient alone, p *= 1 - lr weight_decay before Adam's update (rule 1)."""
    RULE = ops.ADAMW

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, arena: Optional[FlatArena] = None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, arena=arena)


class FusedSGD(FusedOptimizer):
    """torch.optim.SGD with momentum, nesterov and L2 weight decay, no dampening (rule 2).  The momentum buffer is the flat `m`
    buffer, zero from the start - which is torch's first step without a special case; the `v` buffer is not touched."""
    RULE = ops.SGD
    M_NAME, V_NAME = "momentum_buffer", None

    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0, nesterov=False, arena: Optional[FlatArena] = None):
        _check_hyper(type(self), lr=lr, momentum=momentum, weight_decay=weight_decay)
        if nesterov and momentum <= 0:
            raise ValueError(f"{type(self).__name__}: nesterov needs a positive momentum")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=bool(nesterov)), arena)

    def _export(self, group, st):       # torch.optim.SGD keeps no step count, and no state at all without momentum
        return {"momentum_buffer": st["momentum_buffer"]} if group["momentum"] != 0 else {}

    def _launch(self, group, p, g, m, v, mask, t, tdev, stat, skips) -> None:
        ops.optim_step(self.RULE, p, g, m, None, float(group["lr"]), float(group["momentum"]), 0.0, 0.0, float(group["weight_decay"]),
                       ops.NESTEROV if group["nesterov"] else 0, mask, t, tdev, stat, skips, self.lr_scale)


class FusedRMSprop(FusedOptimizer):
    """torch.optim.RMSprop, not centered (rule 3): `v` is square_avg, `m` the momentum buffer (used when momentum > 0)."""
    RULE = ops.RMSPROP
    M_NAME, V_NAME = "momentum_buffer", "square_avg"

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, arena: Optional[FlatArena] = None):
        _check_hyper(type(self), lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum)
        super().__init__(params, dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=False, weight_decay=weight_decay), arena)

    def _export(self, group, st):       # torch.optim.RMSprop has a momentum buffer only with momentum
        return {k: v for k, v in st.items() if k != "momentum_buffer" or group["momentum"] > 0}

    def _launch(self, group, p, g, m, v, mask, t, tdev, stat, skips) -> None:
        ops.optim_step(self.RULE, p, g, m, v, float(group["lr"]), float(group["alpha"]), float(group["momentum"]), float(group["eps"]),
                       float(group["weight_decay"]), 0, mask, t, tdev, stat, skips, self.lr_scale)


RULES = {"adam": FusedAdam, "adamw": FusedAdamW, "sgd": FusedSGD, "rmsprop": FusedRMSprop}


@torch.no_grad()
def zero_grads(optimizers) -> None:
    """`zero_grad()` of several FusedAdam optimisers whose groups live in ONE arena (train.py:201-203: encoder, decoder and
    frame predictor at the top of train_model): adjacent ranges of the gradient arena are zeroed by one launch
    (dvg_zero_tick), and during a hipGraph capture the same launch advances the device-side step counts of those groups
    (step() then skips its one-element increment).  Optimisers without flat arena storage fall back to their own zero_grad."""
    spans = []
    for o in optimizers:
        fl = getattr(o, "_flat", None)
        if not isinstance(o, FusedOptimizer) or o.arena is None or not fl or any(not f for f in fl.values()):
            o.zero_grad()
            continue
        for f in fl.values():
            spans.append((o.arena, f["lo"], f["hi"], f, o))
    capturing = torch.cuda.is_current_stream_capturing()
    spans.sort(key=lambda s_: (id(s_[0]), s_[1]))
    i = 0
    while i < len(spans):
        arena, lo, hi = spans[i][0], spans[i][1], spans[i][2]
        group = [spans[i]]
        while (i + 1 < len(spans) and spans[i + 1][0] is arena and spans[i + 1][1] == hi and len(group) < 4):
            i += 1
            hi = spans[i][2]
            group.append(spans[i])
        ticks = [ops._p(s_[3]["tdev"]) if capturing else None for s_ in group] + [None] * (4 - len(group))
        check(lib().dvg_zero_tick(ops._p(arena.g[lo:hi]), hi - lo, *ticks, ops._stream()), "dvg_zero_tick")
        for s_ in group:
            if capturing:
                s_[3]["ticked"] = True
            s_[4]._restore_grad_views(s_[3])
        i += 1


class GradGuard:
    """Gradient-norm clipping and the skip of a non-finite step, decided on the device (train.py --clip_grad_norm /
    --skip_nonfinite; docs/DESIGN_NOTES_gradguard.md).  Owns the three device buffers the guard's kernels share:

      partials  fp64 partial sums of squares (dvg_grad_sumsq), sized on first use
      stat      4 floats: norm of the last step site, its clip factor, its skip flag, the largest finite norm since the last read
      counters  3 ints: step sites, clipped, skipped since the last read

    max_norm <= 0: no clipping (the factor is 1).  skip_nonfinite: a site whose norm is not finite - some gradient is Inf or NaN -
    changes no parameter, no moment and no effective step count."""

    def __init__(self, max_norm: float, skip_nonfinite: bool, device):
        if max_norm != max_norm or max_norm < 0:
            raise ValueError("GradGuard: max_norm must be >= 0 (0 = no clipping)")
        self.max_norm, self.skip_nonfinite, self.device = float(max_norm), bool(skip_nonfinite), torch.device(device)
        self.stat = torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float32, device=self.device)
        self.counters = torch.zeros(3, dtype=torch.int32, device=self.device)
        self.partials = None

    def reserve(self, nblocks: int) -> torch.Tensor:
        if self.partials is None or self.partials.numel() < nblocks:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("GradGuard: the partial-sum buffer cannot grow during a hipGraph capture (GradGuard.attach "
                                   "the optimisers, or run one eager guarded step, first)")
            self.partials = torch.zeros(nblocks, dtype=torch.float64, device=self.device)
        return self.partials

    def attach(self, optimizers) -> None:
        """Everything a guarded step of `optimizers` allocates, now: the partial sums for all their groups and the groups' skip
        counters.  Needed only when the FIRST guarded step is captured in a hipGraph."""
        n = 0
        for o in optimizers:
            for f in o._flat.values():
                if f:
                    o._skips(f)
                    n += ops.grad_sumsq_blocks(f["g"].numel())
        if n:
            self.reserve(n)

    def read_and_reset(self) -> dict:
        """The numbers since the last call - {"max", "last", "sites", "clipped", "skipped"} - read from the device (this
        synchronises: once per epoch, never inside an iteration); the counters and the maximum start again from zero."""
        st, ct = self.stat.tolist(), self.counters.tolist()
        self.counters.zero_()
        self.stat[3:].zero_()
        return {"max": st[3], "last": st[0], "sites": ct[0], "clipped": ct[1], "skipped": ct[2]}

    def epoch_line(self) -> str:
        """train.py's line after `train frames/s` (reads and resets)."""
        d = self.read_and_reset()
        return ('     grad norm: max %.4g last %.4g  clipped %d  skipped %d  of %d steps'
                % (d["max"], d["last"], d["clipped"], d["skipped"], d["sites"]))


def add_arguments(parser) -> None:
    parser.add_argument('--clip_grad_norm', default=0.0, type=float, metavar='C',   # docs/DESIGN_NOTES_gradguard.md
                        help='limit the L2 norm of ALL gradients that step together after one backward pass to C, by the factor '
                             'min(1, C / (norm + 1e-6)) of torch\'s clip_grad_norm_; decided on the device, also in a hipGraph (0 = off)')
    parser.add_argument('--skip_nonfinite', action='store_true',
                        help='skip such a step when a gradient is Inf or NaN: no parameter, Adam moment or step count changes')
    g = parser.add_argument         # docs/DESIGN_NOTES_optimizers.md
    g('--optimizer', default='adam', metavar='RULE',
      help='the update rule of all four optimisers: adam (default) | adamw | sgd | rmsprop, the arithmetic of torch.optim\'s class of '
           'that name in one fused launch per group (dvg_optim_step); with a rule other than adam --lr is their base rate.  Part '
           'of the --resume fingerprint when it is not adam')
    g('--weight_decay', default=0.0, type=float, metavar='W',
      help='weight decay of the conv, transposed-conv, linear and recurrent weight matrices of the encoder, decoder and frame '
           'predictor (tensors with dim() >= 2); never of biases, BatchNorm parameters, the GP layer or the likelihood.  adamw: '
           'decoupled (p *= 1 - lr W); else the L2 term W p in the gradient (default 0)')
    g('--momentum', default=None, type=float, metavar='M', help='--optimizer sgd | rmsprop: momentum (default: 0.9 for sgd, 0 for rmsprop)')
    g('--nesterov', action='store_true', help='--optimizer sgd: Nesterov momentum (needs a positive --momentum)')
    g('--rmsprop_alpha', default=None, type=float, metavar='A', help='--optimizer rmsprop: the smoothing constant, in [0, 1) (default 0.99)')


def guard_options(opt):
    """(max_norm, skip_nonfinite) when train.py's --clip_grad_norm / --skip_nonfinite ask for a gradient guard, None when
    neither does (an options object from before the flags has neither attribute).  Host only."""
    c = float(getattr(opt, "clip_grad_norm", 0.0) or 0.0)
    skip = bool(getattr(opt, "skip_nonfinite", False))
    if c != c or c < 0:
        raise SystemExit("train.py: --clip_grad_norm must be >= 0")
    return (c, skip) if (c > 0 or skip) else None


def optimizer_options(opt):
    """What train.py's --optimizer / --weight_decay and their companions ask for: None when they ask for nothing new - adam
    without weight decay, the four FusedAdam of always - else {"rule", "weight_decay", "momentum", "nesterov", "alpha"} (a field a
    rule does not have is None).  Every invalid value, and a companion of another rule, ends with a one-line SystemExit naming the
    option (an options object from before the flags has none of the attributes).  Host only."""
    def get(name, default=None):
        return getattr(opt, name, default)

    def number(name, hi=None):
        x = get(name)
        if x is not None and (x != x or x < 0 or x == float("inf") or (hi is not None and x >= hi)):
            raise SystemExit(f"train.py: --{name} must be >= 0" + (f" and below {hi}" if hi is not None else ""))
        return x
    rule = get("optimizer", "adam")
    if rule not in RULES:
        raise SystemExit(f"train.py: --optimizer must be one of {' | '.join(RULES)}, not {rule!r}")
    wd = number("weight_decay") or 0.0
    momentum, alpha, nesterov = number("momentum"), number("rmsprop_alpha", 1), bool(get("nesterov", False))
    if momentum is not None and rule not in ("sgd", "rmsprop"):
        raise SystemExit("train.py: --momentum needs --optimizer sgd or rmsprop")
    if alpha is not None and rule != "rmsprop":
        raise SystemExit("train.py: --rmsprop_alpha needs --optimizer rmsprop")
    if nesterov and rule != "sgd":
        raise SystemExit("train.py: --nesterov needs --optimizer sgd")
    if rule in ("sgd", "rmsprop"):
        momentum = (0.9 if rule == "sgd" else 0.0) if momentum is None else float(momentum)
    if nesterov and not momentum > 0:
        raise SystemExit("train.py: --nesterov needs a positive --momentum")
    if rule == "rmsprop":
        alpha = 0.99 if alpha is None else float(alpha)
    if rule == "adam" and wd == 0:
        return None
    return {"rule": rule, "weight_decay": float(wd), "momentum": momentum, "nesterov": nesterov if rule == "sgd" else None,
            "alpha": alpha}


DECAYING_MODULES = ("encoder", "decoder", "frame_predictor")


def decays(module: str, p) -> bool:
    """--weight_decay applies to `p` of Trainer.<module>: the weight matrices (dim() >= 2) of the encoder, decoder and frame
    predictor - conv, transposed conv, linear, recurrent - and nothing of the GP layer or the likelihood."""
    return module in DECAYING_MODULES and p.dim() >= 2


def decay_mask(params, decaying) -> torch.Tensor:
    """The decay mask of a group made of `params` (those that require a gradient, in order), on the CPU: one uint8 per 16-byte
    piece of the group's flat range, 1 over every piece of a parameter `decaying(p)` is true for.  Views are padded to 4 floats
    (flat_offsets), so a piece belongs to one parameter."""
    params = [p for p in params if p.requires_grad]
    offs, n = flat_offsets(params)
    mask = torch.zeros(n // 4, dtype=torch.uint8)
    for p, o in zip(params, offs):
        if decaying(p):
            mask[o // 4:(o + FlatArena.padded(p.numel())) // 4] = 1
    return mask


def make_optimizer(spec, module: str, groups, lr: float, arena):
    """The optimiser of Trainer.<module> (`groups`: its parameters, or its parameter groups) under `spec` (optimizer_options): None
    = FusedAdam as the Trainer always built it.  Else the rule's class, with the weight decay and - built once, from the arena
    offsets - the decay mask of the modules that decay; the others get weight decay 0 and no mask."""
    if spec is None:
        return FusedAdam(groups, lr=lr, arena=arena)
    wd = spec["weight_decay"] if module in DECAYING_MODULES else 0.0
    kw = {"adam": {}, "adamw": {}, "sgd": dict(momentum=spec["momentum"], nesterov=spec["nesterov"]),
          "rmsprop": dict(alpha=spec["alpha"], momentum=spec["momentum"])}[spec["rule"]]
    o = RULES[spec["rule"]](groups, lr=lr, weight_decay=wd, arena=arena, **kw)
    if wd > 0:
        for gi, f in o._flat.items():
            if f:
                o.set_decay_mask(gi, decay_mask(f["params"], lambda p: decays(module, p)).to(f["p"].device))
    return o


class OptimizerReport:
    """train.py's line per epoch when --optimizer / --weight_decay ask for something: the rule, its hyper-parameters and how many
    of the arena's floats decay.  Counted once, from the masks; reads no device memory afterwards."""

    def __init__(self, spec, optimizers, arena_floats: int):
        self.spec = spec
        self.total = int(arena_floats)
        self.decaying = 4 * sum(int(g["decay_mask"].sum()) for o in optimizers for g in o.param_groups if g.get("decay_mask") is not None)

    def epoch_line(self) -> str:
        s = self.spec
        hyper = {"adam": "", "adamw": "", "sgd": " momentum %g%s" % (s["momentum"] or 0, " nesterov" if s["nesterov"] else ""),
                 "rmsprop": " alpha %g momentum %g" % (s["alpha"] or 0, s["momentum"] or 0)}[s["rule"]]
        return '     optimizer: %s%s  weight decay %g on %d of %d floats' % (s["rule"], hyper, s["weight_decay"], self.decaying, self.total)


def make_guard(opt, device, optimizers):
    """The GradGuard the options ask for, with everything a guarded step of `optimizers` allocates made now (the first
    guarded step may then be captured in a hipGraph); None - no object, no launch - without the flags."""
    go = guard_options(opt)
    if go is None:
        return None
    guard = GradGuard(go[0], go[1], device)
    guard.attach(optimizers)
    return guard


@torch.no_grad()
def guarded_step(optimizers, guard: Optional[GradGuard]) -> None:
    """`o.step()` for every FusedAdam in `optimizers` under ONE verdict of `guard` about ALL the gradients they are about to
    apply: the sum of squares of every flat range (adjacent ranges of a shared arena as one), the decision kernel, then the
    guarded Adam launches - on the current stream, in order, eagerly or inside a hipGraph capture.  With several ranks call it
    after the all-reduce of these ranges has finished: every rank then reduces the same bits in the same order.
    guard = None: the plain steps, nothing else."""
    if guard is None:
        for o in optimizers:
            o.step()
        return
    spans = []
    for o in optimizers:
        if not isinstance(o, FusedOptimizer):
            raise RuntimeError("guarded_step: fused optimisers (FusedAdam, FusedAdamW, FusedSGD, FusedRMSprop) expected")
        spans += o.guard_spans()
    if not spans:
        return
    shared = sorted((s_ for s_ in spans if s_[0] is not None), key=lambda s_: (id(s_[0]), s_[1]))
    ranges = []                                            # flat gradient tensors, adjacent arena ranges merged
    for arena, lo, hi, _ in shared:
        if ranges and ranges[-1][0] is arena and ranges[-1][2] == lo:
            ranges[-1][2] = hi
        else:
            ranges.append([arena, lo, hi])
    flats = [a.g[lo:hi] for a, lo, hi in ranges] + [s_[3] for s_ in spans if s_[0] is None]
    partials = guard.reserve(sum(ops.grad_sumsq_blocks(g.numel()) for g in flats))
    slot = 0
    for g in flats:
        slot += ops.grad_sumsq(g, partials, slot)
    ops.grad_guard_finish(partials, slot, guard.max_norm, guard.skip_nonfinite, guard.stat, guard.counters)
    for o in optimizers:
        o.step(guard=guard)
