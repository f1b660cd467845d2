"""The file side of `train.py --resume`: where a training state lives, how it is written so that a kill cannot damage the last
good one, how it is read so that every failure is one line, and the fingerprint that refuses a state from another configuration.
What the state IS - which tensors and counters of a Trainer (dvg_amd/trainer.py) - is `capture` / `restore` below, which
`Trainer.state_dict` / `Trainer.load_state_dict` call (docs/DESIGN_NOTES_resume.md lists every entry and why it is state).

One process: `<output_path>/train_state.pth` holds everything.  Several ranks: rank 0 writes the shared part (parameters, Adam
moments and step counts, scheduler, epoch) to `train_state.pth`, every rank what differs between replicas (BatchNorm buffers,
random streams, data positions) to `train_state.rank<r>.pth` beside it.

Host only: no kernel is launched from here (with a gradient guard, capture() first has the optimisers fold their skip counters
into the step counts: FusedAdam.sync_step_counts, one read of a few device ints)."""
from __future__ import annotations

import os
import random

import numpy as np
import torch

FORMAT = 1
NAME = "train_state.pth"
# the options a state is tied to: the shapes of the arena and of the batches, and what decides which closures run
OPTION_FIELDS = ("model", "image_width", "channels", "g_dim", "rnn_size", "predictor_rnn_layers", "batch_size", "n_past",
                 "n_future", "n_eval", "dataset", "num_digits", "last_frame_skip", "ft")
RANK_KEY = "rank_state"


def refuse(path, what):
    raise SystemExit(f"train.py --resume: {path}: {what}")


def resolve(path: str) -> str:
    """`--resume PATH`: a train_state.pth, or the directory that holds one."""
    return os.path.join(path, NAME) if os.path.isdir(path) else path


def rank_path(path: str, rank: int) -> str:
    root, ext = os.path.splitext(path)
    return f"{root}.rank{rank}{ext}"


# fields a fingerprint carries only when they differ from the value given here: a state without the field was written by a run
# with that value (every state from before --predictor is an `lstm` state, every one from before --optimizer was honoured an
# `adam` state, every one from before --gp_kernel an `rbf` state), and such a run writes the fingerprint it always did
ABSENT_MEANS = {"predictor": "lstm", "optimizer": "adam", "gp_kernel": "rbf"}


def option_fingerprint(opt) -> dict:
    fp = {k: getattr(opt, k) for k in OPTION_FIELDS}
    fp["world"] = int(opt.world)
    for k, default in ABSENT_MEANS.items():
        if getattr(opt, k, default) != default:
            fp[k] = getattr(opt, k)
    return fp


def check_fingerprint(saved: dict, now: dict, path: str) -> None:
    """Ends the program naming the first field that disagrees.  `now` may be a part of the fingerprint (train.py checks the
    options before it builds anything, the arena layout once the Trainer exists)."""
    if "model" in now:            # an options fingerprint: the fields of ABSENT_MEANS are compared whichever side lacks them
        for k, default in ABSENT_MEANS.items():
            a, b = saved.get(k, default), now.get(k, default)
            if a != b:
                refuse(path, f"{k} is {a!r} in the file and {b!r} in this run")
    for k, v in now.items():
        if k in ABSENT_MEANS:
            continue
        if k not in saved:
            refuse(path, f"the fingerprint has no field {k!r}")
        a, b = saved[k], v
        if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
            a, b = _plain(a), _plain(b)
        if a != b:
            refuse(path, f"{k} is {saved[k]!r} in the file and {v!r} in this run")


def _plain(x):
    return [_plain(v) for v in x] if isinstance(x, (list, tuple)) else x


def atomic_save(obj, path: str) -> None:
    """torch.save to a temporary name in the same directory, then os.replace: at every instant `path` is either the previous
    complete file or the new complete file."""
    tmp = f"{path}.tmp.{os.getpid()}"
    try:
        torch.save(obj, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def write(state: dict, directory: str, rank: int, world: int) -> str:
    """Write what this rank owns of `state` (Trainer.state_dict) under `directory`; returns the path of the shared file."""
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, NAME)
    if world == 1:
        atomic_save(state, path)
        return path
    state = dict(state)
    mine = state.pop(RANK_KEY)
    atomic_save({"format": FORMAT, "epoch": state["epoch"], "world": world, RANK_KEY: mine}, rank_path(path, rank))
    if rank == 0:
        atomic_save(state, path)
    return path


def _load(path: str) -> dict:
    if not os.path.isfile(path):
        refuse(path, "no such file")
    try:
        sd = torch.load(path, map_location="cpu", weights_only=False)
    except Exception as e:   # noqa: BLE001 - a truncated zip, a pickle cut short, something that is no torch file at all
        refuse(path, f"cannot be read, truncated or not a training state ({type(e).__name__})")
    if not isinstance(sd, dict) or sd.get("format") != FORMAT:
        refuse(path, f"format is {sd.get('format') if isinstance(sd, dict) else type(sd).__name__!r} in the file and "
                     f"{FORMAT!r} in this run")
    return sd


def read(path: str, rank: int = 0, world: int = 1) -> dict:
    """The state for this rank: the shared file, and with several ranks this rank's own file merged into it.  Every failure -
    a missing file, a truncated one, a missing field, files of different epochs - is a one-line SystemExit."""
    sd = _load(path)
    for k in ("fingerprint", "epoch", "arena", "optimizers", "scheduler"):
        if k not in sd:
            refuse(path, f"no field {k!r}")
    saved_world = sd["fingerprint"].get("world")
    if saved_world != world:
        refuse(path, f"world is {saved_world!r} in the file and {world!r} in this run")
    if world > 1:
        rp = rank_path(path, rank)
        mine = _load(rp)
        if mine.get("epoch") != sd["epoch"] or mine.get("world") != world:
            refuse(rp, f"epoch is {mine.get('epoch')!r} in the file and {sd['epoch']!r} in {os.path.basename(path)}")
        sd[RANK_KEY] = mine.get(RANK_KEY)
    if not isinstance(sd.get(RANK_KEY), dict):
        refuse(path, f"no field {RANK_KEY!r}")
    for k in ("buffers", "rng", "data"):
        if k not in sd[RANK_KEY]:
            refuse(path, f"no field {RANK_KEY}.{k!r}")
    return sd


def random_streams(device) -> dict:
    """Every global random stream a training run draws from: torch's CPU generator, the current device's, Python's and numpy's."""
    return {"torch_cpu": torch.get_rng_state().clone(), "torch_cuda": torch.cuda.get_rng_state(device).clone(),
            "python": random.getstate(), "numpy": np.random.get_state()}


def set_random_streams(rng: dict, device) -> None:
    torch.set_rng_state(rng["torch_cpu"].cpu())
    torch.cuda.set_rng_state(rng["torch_cuda"].cpu(), device)
    random.setstate(rng["python"])
    np.random.set_state(rng["numpy"])


def detached_copy(module):
    """A deep copy of `module` whose parameters and buffers are fresh tensors with their OWN storage and no gradient
    (copy.deepcopy alone clones the whole storage behind every arena view, and would copy `.grad` as well).  Trainer.save's
    helper (checkpoint below), beside the other code that writes training state."""
    import copy
    memo = {}
    for p in module.parameters():
        memo[id(p)] = torch.nn.Parameter(p.detach().clone(), requires_grad=p.requires_grad)
    for b in module.buffers():
        memo[id(b)] = b.detach().clone()
    hidden = getattr(module, "hidden", None)
    if hidden is not None:         # the recurrent state of the last sequence, may carry an autograd graph: (h, c) pairs for
        # an lstm, single tensors for a gru / rnn
        memo[id(hidden)] = [s.detach().clone() if torch.is_tensor(s) else tuple(t.detach().clone() for t in s)
                            for s in hidden]
    return copy.deepcopy(module, memo)


def owned_state_dict(sd):
    """`sd` (a module's state_dict) with every tensor cloned into its own storage; keeps the module version info torch's
    state_dict carries (and load_state_dict reads)."""
    out = type(sd)((k, v.detach().clone() if torch.is_tensor(v) else v) for k, v in sd.items())
    if hasattr(sd, "_metadata"):
        out._metadata = sd._metadata
    return out


def checkpoint(tr) -> dict:
    """train.py:380-388: whole-module pickles + GP / likelihood / GP-optimiser state dicts (Trainer.save writes it)."""
    return {'encoder': detached_copy(tr.encoder), 'decoder': detached_copy(tr.decoder),
            'frame_predictor': detached_copy(tr.frame_predictor), 'likelihood': owned_state_dict(tr.likelihood.state_dict()),
            'gp_layer': owned_state_dict(tr.gp_layer.state_dict()), 'gp_layer_optimizer': tr.optimizer.state_dict(), 'opt': tr.opt}


# ---- what the state of a trainer.Trainer is ---------------------------------------------------------------------------------
def named_optimizers(tr):
    return (("gp", tr.optimizer), ("frame_predictor", tr.frame_predictor_optimizer), ("decoder", tr.decoder_optimizer),
            ("encoder", tr.encoder_optimizer))


def named_buffers(tr):
    for i, m in enumerate(tr.modules):
        for k, b in m.named_buffers():
            yield f"{i}.{k}", b


def fingerprint(tr) -> dict:
    """The options and the arena layout: (optimiser, group, lo, hi) of every FusedAdam group."""
    fp = option_fingerprint(tr.opt)
    fp["layout"] = [[name, gi, *o.flat_range(gi)] for name, o in named_optimizers(tr) for gi in sorted(o._flat)]
    return fp


def global_step(tr) -> int:
    """Iterations trained so far: the Adam step count of the encoder, which only train_model steps."""
    o = tr.encoder_optimizer
    return int(o.state[o.param_groups[0]["params"][0]]["step"])


def capture(tr, epoch=0, train_gen=None, test_gen=None, shared=True) -> dict:
    """Everything the next iteration reads that is not rebuilt from the options: with it, a run continues as if it had not
    stopped.  epoch: the number of the NEXT epoch; train_gen / test_gen: the batch generators whose positions to record;
    shared=False leaves out what rank 0 writes for all ranks.  Every tensor owns its storage (a view of the arena would make
    torch.save write the whole arena behind it)."""
    writer = tr._plot_writer
    mine = {"rank": tr.rank,
            "buffers": {k: b.detach().clone() for k, b in named_buffers(tr)},
            "rng": random_streams(tr.dev),
            "plot_writer": writer.rng.get_state() if writer is not None else None,
            "data": {"train": train_gen.position() if train_gen is not None else None,
                     "test": test_gen.position() if test_gen is not None else None}}
    sd = {"format": FORMAT, "epoch": int(epoch), RANK_KEY: mine}
    for _, o in named_optimizers(tr):    # steps a gradient guard skipped are not steps: the counts of steps really applied
        o.sync_step_counts()             # (every rank: the host counts stay the same on all of them)
    if shared:
        lo, hi = tr.rng_gp
        a = tr.arena
        sd.update(fingerprint=fingerprint(tr), global_step=global_step(tr),
                  arena={"p": a.p.detach().clone(), "m": a.m.detach().clone(), "v": a.v.detach().clone(),
                         # train_model does not zero the GP optimiser's gradients (Trainer.reference_gp_grad_leak): what the
                         # last GP closure left in this range is consumed by the next optimizer.step()
                         "g_gp": a.g[lo:hi].detach().clone(), "g_gp_range": (lo, hi)},
                  optimizers={name: o.host_state() for name, o in named_optimizers(tr)},
                  scheduler=tr.scheduler.state_dict())
        if tr.ema is not None:   # --ema_decay: the average and its count of updates (dvg_amd/ema.py); no key without the flag
            st = tr.ema.state()
            sd["arena"]["e"], sd["ema"] = st["e"], st["ema"]
        if tr.lr_schedule is not None:   # --lr_schedule: the spec and the count of iterations (dvg_amd/lr_schedule.py); no key without the flag
            sd["lr_schedule"] = tr.lr_schedule.state()
        if tr.validation is not None:    # --val_every: the history and the best scores (dvg_amd/validate.py); no key without the flag
            sd["validation"] = tr.validation.state()
    return sd


@torch.no_grad()
def restore(tr, sd, train_gen=None, test_gen=None, path="<state>") -> int:
    """Write a capture() into `tr` THROUGH the existing arena views: no parameter, gradient or moment changes its address.
    Returns the number of the next epoch.  A mismatch of the fingerprint ends the program (SystemExit naming the field)."""
    check_fingerprint(sd["fingerprint"], fingerprint(tr), path)
    for name, o in named_optimizers(tr):    # the hyper-parameters are state, as the rates are: a command line cannot change them
        bad = o.hyper_mismatch(sd["optimizers"][name])
        if bad is None and name != "gp" and getattr(tr.opt, "optimizer", "adam") != "adam":
            # under another rule --lr is the base rate; only the GP optimiser's is moved by its milestones
            a, b = sd["optimizers"][name]["param_groups"][0]["lr"], o.param_groups[0]["lr"]
            bad = ("lr", a, b) if float(a) != float(b) else None
        if bad is not None:
            refuse(path, f"optimizers.{name}.{bad[0]} is {bad[1]!r} in the file and {bad[2]!r} in this run")
    a, saved = tr.arena, sd["arena"]
    for name in ("p", "m", "v"):
        if saved[name].numel() != getattr(a, name).numel():
            refuse(path, f"arena.{name} has {saved[name].numel()} floats in the file and {getattr(a, name).numel()} in this run")
        getattr(a, name).copy_(saved[name])
    lo, hi = saved["g_gp_range"]
    a.g[lo:hi].copy_(saved["g_gp"])
    if tr.ema is not None:       # the decay of THIS run applies; a state without an average restarts it from the restored weights
        tr.ema.load_state(saved.get("e"), sd.get("ema"))
        if "e" not in saved and tr.rank == 0:
            print(f"{path}: no weight average in the file: --ema_decay restarts it from the restored weights", flush=True)
    elif "e" in saved and tr.rank == 0:
        print(f"{path}: the weight average in the file is ignored: this run has no --ema_decay", flush=True)
    if tr.validation is not None:   # a state without validations starts an empty history
        tr.validation.load_state(sd.get("validation"))
    elif "validation" in sd and tr.rank == 0 and not getattr(tr.opt, "val_every", 0):
        print(f"{path}: the validation history in the file is ignored: this run has no --val_every", flush=True)
    for name, o in named_optimizers(tr):
        o.load_host_state(sd["optimizers"][name])      # step counts (begin_capture seeds the device counts from them), lr
    tr.scheduler.load_state_dict(sd["scheduler"])
    from . import lr_schedule    # --lr_schedule: the count of iterations, a state from before the flag counts from its global step
    lr_schedule.restore(tr.lr_schedule, sd, path, sd.get("global_step", global_step(tr)), tr.rank,
                        tr.encoder_optimizer.param_groups[0]["lr"])
    mine = sd[RANK_KEY]
    buffers = dict(named_buffers(tr))
    if set(buffers) != set(mine["buffers"]):
        refuse(path, "buffers: another set of module buffers than this run's")
    for k, b in buffers.items():
        b.copy_(mine["buffers"][k])
    # the kernels read parameters through raw pointers and cache packed / folded forms by version (dvg_amd/_derived.py): what
    # was packed from the weights this Trainer held until now must not be served again
    for m in tr.modules:
        for t in list(m.parameters()) + list(m.buffers()):
            torch.autograd.graph.increment_version(t)
    tr._ft_cache = None
    tr.frame_predictor.hidden = None
    # the host-side memo of the `variational_params_initialized` buffer just restored (read here, not during a capture)
    tr.gp_layer._init_checked = bool(int(tr.gp_layer.variational_strategy.variational_params_initialized.item()))
    # a captured iteration holds device step counts and packs of the old state: GraphedIteration re-captures when this moves
    tr.state_loads += 1
    set_random_streams(mine["rng"], tr.dev)
    if mine.get("plot_writer") is not None:
        from . import viz
        tr._plot_writer = tr._plot_writer or viz.PlotWriter(getattr(tr.opt, "seed", 1))
        tr._plot_writer.rng.set_state(mine["plot_writer"])
    for gen, pos in ((train_gen, mine["data"]["train"]), (test_gen, mine["data"]["test"])):
        if gen is not None and pos is not None:
            gen.restore(pos)
    return int(sd["epoch"])


# ---- train.py's two calls --------------------------------------------------------------------------------------------------
def open_resume(opt):
    """`--resume PATH` -> (path, state) read for this rank and checked against the options, or None without the flag.  Runs
    before anything is built: a wrong file costs a second, not a start-up."""
    if not getattr(opt, "resume", ""):
        return None
    path = resolve(opt.resume)
    state = read(path, opt.rank, opt.world)
    check_fingerprint(state["fingerprint"], option_fingerprint(opt), path)
    return path, state


def resume(tr, opened, train_gen, test_gen) -> int:
    """Load what open_resume returned into the Trainer and the generators; returns the first epoch to run (0 without a state)
    and prints the resume line on rank 0."""
    if opened is None:
        return 0
    path, state = opened
    epoch = tr.load_state_dict(state, train_gen, test_gen, path=path)
    if tr.rank == 0:
        print('resumed from %s: epoch %d, global step %d' % (path, epoch, global_step(tr)), flush=True)
    return epoch
