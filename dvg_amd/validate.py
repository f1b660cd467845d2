"""`train.py --val_every N`: every N epochs rank 0 scores a FIXED set of held-out clips with the eval-mode rollouts of
generate_frames.py's make_gifs (dvg_amd/rollout.py: the posterior rollout and `--val_nsample` sample rollouts) and the Finn
metrics (ops.eval_frames_finn), reduces them on the device (dvg_val_accumulate, csrc/validate.hip: one launch per rollout set,
one readback per validation), prints the numbers, keeps them in the training state and in `val_log.jsonl`, and keeps a copy of
the best checkpoint (`model_best.pth`; with --ema_decay also `model_ema_best.pth`).  Semantics, the selection rule, what is put
back after a pass and the multi-rank choice: docs/DESIGN_NOTES_validation.md.

Training does not notice: the clips come from a stream of their own, the GP base samples from a private generator, every module
mode, recurrent state and cache entry the pass touched is put back.  Without the flag nothing here runs: `make` returns None -
no object, no launch, no file, no state key."""
from __future__ import annotations

import argparse
import json
import math
import os

import torch

from . import _derived, ops, rollout

FILE_BEST, FILE_EMA_BEST, LOG = "model_best.pth", "model_ema_best.pth", "val_log.jsonl"
SEED_OFFSET = 104729            # the validation stream's seed = opt.seed + this, on every rank
TRACKS = ("posterior", "best", "mean")
METRICS = ("ssim", "psnr", "mse")


# ---- options -------------------------------------------------------------------------------------------------------------------------
def _int_at_least(low, flag):
    def parse(text):
        v = int(text)
        if v < low:
            raise SystemExit(f"train.py: {flag} must be >= {low}")
        return v
    return parse


def add_arguments(parser) -> None:
    """The three flags; a value out of range ends the program while the command line is parsed, before anything is built."""
    parser.add_argument('--val_every', default=0, type=_int_at_least(0, '--val_every'), metavar='N',   # docs/DESIGN_NOTES_validation.md
                        help='every N epochs score --val_batches held-out batches (always the same clips) with the eval-mode '
                             'rollouts and the Finn SSIM / PSNR / MSE, print and log the numbers (val_log.jsonl) and keep the best '
                             'checkpoint as model_best.pth (generate_frames.py --best reads it); 0 = off')
    parser.add_argument('--val_batches', default=8, type=_int_at_least(1, '--val_batches'), metavar='K',
                        help='--val_every: batches of the test split per validation')
    parser.add_argument('--val_nsample', default=4, type=_int_at_least(0, '--val_nsample'), metavar='S',
                        help='--val_every: sample rollouts per clip beside the posterior rollout (0 = the posterior rollout only)')
    # (no attribute without the flag: the options of such a run - printed, pickled into its checkpoints - are what they always were)
    parser.add_argument('--val_gp', action='store_true', default=argparse.SUPPRESS,      # docs/DESIGN_NOTES_gp_score.md
                        help='--val_every: also score the GP trigger\'s predictive on the same clips - negative log predictive '
                             'density, standardised residuals, 68 %% / 95 %% coverage, PIT histogram, variance ~ squared-error '
                             'correlation of the one-step latent forecasts, on ground-truth frames and along the posterior rollout '
                             '(dvg_gp_score); one more "val gp:" line and a "gp" entry per record')


def options(opt):
    """{"every", "batches", "nsample"} - and "gp": True with --val_gp - when the options ask for validation, else None (an options
    object from before the flags has no such attribute).  Host only."""
    every = int(getattr(opt, "val_every", 0) or 0)
    if every < 0:
        raise SystemExit("train.py: --val_every must be >= 0")
    if every == 0:
        if getattr(opt, "val_gp", False):
            raise SystemExit("train.py: --val_gp scores the clips of a validation: it needs --val_every N")
        return None
    batches, nsample = int(getattr(opt, "val_batches", 8)), int(getattr(opt, "val_nsample", 4))
    if batches < 1 or nsample < 0:
        raise SystemExit("train.py: --val_batches must be >= 1 and --val_nsample >= 0")
    if opt.n_eval <= opt.n_past:
        raise SystemExit(f"train.py: --val_every scores the predicted steps n_past ... n_eval - 1: --n_eval {opt.n_eval} leaves none "
                         f"after --n_past {opt.n_past}")
    return dict({"every": every, "batches": batches, "nsample": nsample}, **({"gp": True} if getattr(opt, "val_gp", False) else {}))


# ---- from the accumulators to numbers (Python fp64) --------------------------------------------------------------------------------------
def summarise(acc, cnt) -> dict:
    """acc [3][T][2] (metric, step, {sum, sum of squares}) and cnt [3][T] of ONE track, as nested lists -> per metric
    {"mean": the mean over the steps that have one, "curve": sum / cnt per step, "std": sqrt(max(0, sumsq / cnt - mean^2)),
    "count"}; a step (or a track) without a single finite entry has None."""
    out = {}
    for m, name in enumerate(METRICS):
        curve, std, count = [], [], []
        for (s, q), n in zip(acc[m], cnt[m]):
            n = int(n)
            count.append(n)
            if n == 0:
                curve.append(None)
                std.append(None)
                continue
            mean = float(s) / n
            curve.append(mean)
            std.append(math.sqrt(max(0.0, float(q) / n - mean * mean)))
        have = [v for v in curve if v is not None]
        out[name] = {"mean": sum(have) / len(have) if have else None, "curve": curve, "std": std, "count": count}
    return out


def selection_score(tracks: dict, nsample: int):
    """The one number checkpoints are compared by: the mean over the predicted steps of the `best` track's SSIM, or - without
    samples - of the `posterior` track's.  None when nothing finite was scored."""
    return tracks["best" if nsample >= 1 else "posterior"]["ssim"]["mean"]


def improves(score, best_so_far) -> bool:
    """Strictly greater replaces; a tie - and a score that is None or NaN - keeps what there is."""
    if score is None or score != score:
        return False
    return best_so_far is None or score > best_so_far


def _plain(v):
    """JSON has no NaN / Infinity: whatever is not a finite number is written as null."""
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, float) and not math.isfinite(v):
        return None
    return v


def log_text(history) -> str:
    """val_log.jsonl: one JSON object per validation, in order."""
    return "".join(json.dumps(_plain(rec), sort_keys=True) + "\n" for rec in history)


def write_log(history, directory: str) -> str:
    """The whole file from the history, through a temporary name: at every instant it is a complete log."""
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, LOG)
    tmp = f"{path}.tmp.{os.getpid()}"
    try:
        with open(tmp, "w") as f:
            f.write(log_text(history))
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def read_log(path: str) -> list:
    with open(path) as f:
        return [json.loads(ln) for ln in f if ln.strip()]


def _num(v) -> float:
    return float("nan") if v is None else float(v)


def line(tag: str, res: dict, best_epoch) -> str:
    """`     val: ssim .. psnr .. mse .. | best of S: ssim .. psnr .. | mean: ssim .. psnr ..  (N clips x T steps)  best so far: epoch E`;
    a number nothing finite went into prints as nan, and without samples the two sample groups are left out."""
    t = res["tracks"]
    text = '     %s: ssim %.4f psnr %.2f mse %.5f' % (tag, _num(t["posterior"]["ssim"]["mean"]), _num(t["posterior"]["psnr"]["mean"]),
                                                     _num(t["posterior"]["mse"]["mean"]))
    if res["nsample"] >= 1:
        text += ' | best of %d: ssim %.4f psnr %.2f | mean: ssim %.4f psnr %.2f' % (
            res["nsample"], _num(t["best"]["ssim"]["mean"]), _num(t["best"]["psnr"]["mean"]), _num(t["mean"]["ssim"]["mean"]),
            _num(t["mean"]["psnr"]["mean"]))
    return text + '  (%d clips x %d steps)  best so far: epoch %d' % (res["clips"], res["steps"], -1 if best_epoch is None else best_epoch)


# ---- the pass ------------------------------------------------------------------------------------------------------------------------
class Validator:
    """Owns the held-out stream (made like train.py's test stream, with a seed of its own that does not depend on the rank) and
    its initial position, a private device generator for the GP base samples, and the accumulators.  `run(modules)` scores the
    same `batches` batches with the same base samples every time."""

    def __init__(self, opt, device):
        from .data import make_batch_generator
        o = options(opt)
        if o is None:
            raise ValueError("Validator: the options have no --val_every")
        self.opt, self.dev = opt, torch.device(device)
        self.batches, self.nsample = o["batches"], o["nsample"]
        self.steps = opt.n_eval - opt.n_past
        self.seed = int(opt.seed) + SEED_OFFSET
        self.stream = make_batch_generator(opt, opt.n_eval, self.seed, device, train=False)
        self.start = self.stream.position()
        self.gen = torch.Generator(device=self.dev)
        # [0]: the posterior rollout (one "sample"), [1]: the sample rollouts; read back as one fp64 tensor
        self.acc = torch.zeros((2, 2, 3, self.steps, 2), dtype=torch.float64, device=self.dev)
        self.cnt = torch.zeros((2, 2, 3, self.steps), dtype=torch.int64, device=self.dev)
        self.best = None        # (B,) int32: the best sample per row of the last batch scored
        self.gp = None          # --val_gp: the GP scorer (dvg_amd/gp_score.py); without the flag no object, no launch, no key
        if o.get("gp"):
            from . import gp_score
            self.gp = gp_score.GPScorer(opt.g_dim, gp_score.track_steps(opt.n_past, opt.n_eval), self.dev)

    def draws(self):
        """The K batches of a validation and their base samples, from the start of both streams: yields (x, eps) with x the
        n_eval frames (B,C,H,W) and eps[s][i] the (D,B) base sample of sample s at GP step i.  Nothing is drawn from torch's
        global generators."""
        opt = self.opt
        self.stream.restore(self.start)
        self.gen.manual_seed(self.seed)
        gp_steps = rollout.trigger_steps(opt.n_past, opt.n_eval)
        for _ in range(self.batches):
            x = next(self.stream)()
            b = x[0].shape[0]
            yield x, [{i: torch.randn(opt.g_dim, b, generator=self.gen, device=self.dev) for i in gp_steps}
                      for _ in range(self.nsample)]

    @torch.no_grad()
    def run(self, modules, trainer=None) -> dict:
        """One validation of (encoder, decoder, frame_predictor, gp_layer, likelihood).  trainer: the trainer.Trainer that owns
        them, if one does (its fine-tuning cache is put back as well)."""
        live = _Live(modules, trainer)
        try:
            for m in modules:
                m.eval()
            self._score(*modules)
            flat = torch.cat([self.acc.flatten(), self.cnt.flatten().double()]).cpu()      # the one readback
            gp = self.gp.read() if self.gp is not None else None                           # (--val_gp: and its own)
        finally:
            live.put_back()
        n = self.acc.numel()
        acc = flat[:n].view(self.acc.shape).tolist()
        cnt = flat[n:].view(self.cnt.shape).long().tolist()
        tracks = {"posterior": summarise(acc[0][0], cnt[0][0]), "best": summarise(acc[1][0], cnt[1][0]),
                  "mean": summarise(acc[1][1], cnt[1][1])}
        res = {"clips": self.batches * int(self.opt.local_batch), "steps": self.steps, "nsample": self.nsample, "tracks": tracks,
               "score": selection_score(tracks, self.nsample)}
        if gp is not None:
            res["gp"] = gp
        return res

    def _score(self, enc, dec, fp, gp, lik):
        opt, T, S = self.opt, self.steps, self.nsample
        lo, hi, lfs = opt.n_past, opt.n_eval, bool(opt.last_frame_skip)
        self.acc.zero_()
        self.cnt.zero_()
        if self.gp is not None:
            self.gp.zero()
        for x, eps in self.draws():
            B = x[0].shape[0]
            fp.batch_size = B
            gt = torch.stack(list(x[lo:hi]))
            state = rollout.condition(enc, fp, x, lo, lfs, decoder=dec)
            post = rollout.posterior_from(state, enc, dec, fp, gp, lik, lo, hi, lfs)
            m = ops.eval_frames_finn(gt, torch.stack(post[lo:hi]))                         # three (T, B)
            ops.val_accumulate(*(v.t().contiguous().view(B, 1, T) for v in m), self.acc[0], self.cnt[0])
            if self.gp is not None:      # the one-step latent forecasts on the clips and along the posterior rollout just made
                self.gp.score(enc, gp, lik, x, post, lo, hi)
            if S == 0:
                continue
            ssim, psnr, mse = (torch.empty((B, S, T), device=self.dev) for _ in range(3))
            for s in range(S):
                frames = rollout.sample_from(state, enc, dec, fp, gp, lik, lo, hi, lfs, eps_by_step=eps[s])
                m = ops.eval_frames_finn(gt, torch.stack(frames[lo:hi]))
                ssim[:, s], psnr[:, s], mse[:, s] = (v.t() for v in m)
            if self.best is None or self.best.numel() != B:
                self.best = torch.zeros(B, dtype=torch.int32, device=self.dev)
            ops.val_accumulate(ssim, psnr, mse, self.acc[1], self.cnt[1], self.best)


class _Live:
    """What a pass changes on live objects, taken before it and put back after it: the training flag of every submodule, the
    frame predictor's recurrent state and batch size, the trainer's fine-tuning cache, and the cache entries the eval-mode calls
    made - skip-keyed ones (hoisted skip halves, frozen-skip declarations, skip projections) and parameter-derived ones (eval-mode
    BatchNorm folds, inference weight forms)."""

    def __init__(self, modules, trainer):
        self.flags = [(sm, sm.training) for m in modules for sm in m.modules()]
        self.fp, self.trainer = modules[2], trainer
        self.hidden, self.batch_size = getattr(self.fp, "hidden", None), getattr(self.fp, "batch_size", None)
        self.ft_cache = trainer._ft_cache if trainer is not None else None
        self.skips, self.derived = _derived.skip_mark(), _derived.derived_mark()

    def put_back(self):
        for sm, flag in self.flags:
            sm.training = flag
        self.fp.hidden, self.fp.batch_size = self.hidden, self.batch_size
        if self.trainer is not None:
            self.trainer._ft_cache = self.ft_cache
        _derived.skip_drop_since(self.skips)
        _derived.derived_restore(self.derived)


# ---- train.py's side: when to validate, what to print and keep ---------------------------------------------------------------------------
class Validation:
    """The Validator plus what a run remembers of its validations: the history (one record per validation: what val_log.jsonl
    holds) and the best score and epoch, of the live weights and - with --ema_decay - of the averaged ones."""

    def __init__(self, opt, device):
        self.every = options(opt)["every"]
        self.validator = Validator(opt, device)
        self.load_state(None)

    # ---- train_state ---------------------------------------------------------------------------------------------------------------
    def state(self) -> dict:
        return {"history": [dict(r) for r in self.history], "best": dict(self.best_live), "ema_best": dict(self.best_ema)}

    def load_state(self, st) -> None:
        """st = None (a state written without validation): an empty history."""
        st = st or {}
        self.history = [dict(r) for r in st.get("history", [])]
        self.best_live = dict(st.get("best") or {"score": None, "epoch": None})
        self.best_ema = dict(st.get("ema_best") or {"score": None, "epoch": None})

    # ---- one validation ------------------------------------------------------------------------------------------------------------
    def validate(self, tr, epoch: int) -> dict:
        from . import train_state
        opt = tr.opt
        save = not getattr(opt, "no_save", False)
        rec = {"epoch": int(epoch), "global_step": train_state.global_step(tr)}
        res = self.validator.run(tr.modules, tr)
        rec.update(res)
        if improves(res["score"], self.best_live["score"]):
            self.best_live = {"score": res["score"], "epoch": int(epoch)}
            if save:
                os.makedirs(opt.output_path, exist_ok=True)
                tr.save(os.path.join(opt.output_path, FILE_BEST))
        print(line("val", res, self.best_live["epoch"]), flush=True)
        if "gp" in res:
            from . import gp_score
            print(gp_score.line("val gp", res["gp"]), flush=True)
        if tr.ema is not None:
            # the same clips and base samples on what model_ema.pth holds: every parameter from the average, every buffer live
            twins = [tr.ema.module_copy(m) for m in tr.modules]
            ema = self.validator.run(twins)
            del twins
            rec["ema"] = ema
            if improves(ema["score"], self.best_ema["score"]):
                self.best_ema = {"score": ema["score"], "epoch": int(epoch)}
                if save:
                    os.makedirs(opt.output_path, exist_ok=True)
                    tr.ema.save(tr, os.path.join(opt.output_path, FILE_EMA_BEST))
            print(line("val(ema)", ema, self.best_ema["epoch"]), flush=True)
            if "gp" in ema:
                from . import gp_score
                print(gp_score.line("val(ema) gp", ema["gp"]), flush=True)
        self.history.append(rec)
        if save:
            write_log(self.history, opt.output_path)
        return rec


def make(opt, device):
    """The Validation the options ask for, on rank 0 - which holds the BatchNorm buffers model.pth is written with; None
    without the flag and on every other rank (they meet rank 0 at the next collective)."""
    if options(opt) is None or int(getattr(opt, "rank", 0)) != 0:
        return None
    return Validation(opt, device)


def after_epoch(tr, epoch: int) -> None:
    """train.py's call, once per epoch after its log lines and checkpoint: validates when the epoch is one of every N."""
    v = tr.validation
    if v is not None and epoch % v.every == 0:
        v.validate(tr, epoch)


def best_checkpoint_path(model_dir: str, ema: bool) -> str:
    """generate_frames.py --best: `<model_dir>/model_best.pth`, with --ema `<model_dir>/model_ema_best.pth`."""
    path = '%s/%s' % (model_dir, FILE_EMA_BEST if ema else FILE_BEST)
    if not os.path.exists(path):
        raise SystemExit(f"generate_frames.py --best: {path} does not exist (train.py --val_every"
                         f"{' --ema_decay' if ema else ''} writes it)")
    return path
