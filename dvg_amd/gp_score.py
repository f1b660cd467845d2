"""`train.py --val_gp` / `generate_frames.py --gp_report`: is the GP trigger's predictive variance worth anything on clips the
model has not seen?  The one-step latent forecasts of held-out clips are scored as a probabilistic regressor is: negative log
predictive density, standardised residuals, 68 % / 95 % coverage, a PIT histogram and the correlation between the predicted
variance and the realised squared error.  The sums and counts are reduced on the device (dvg_gp_score, csrc/gp_score.hip: one
launch per batch and track, one readback per validation); this module holds the host logic - from the accumulators to numbers
(`summarise`, `report`, `line`) - and the scorer that feeds the kernel (`GPScorer`).  Equations, both tracks, what each number
means when the GP is calibrated: docs/DESIGN_NOTES_gp_score.md."""
from __future__ import annotations

import json
import math
import os
from fractions import Fraction

import torch

TRACKS = ("forced", "rollout")
FILE = "gp_report.json"
# dvg_gp_score's slots (include/dvg_hip.h)
NLPD, E, E2, V, Z, Z2, Y, Y2, V2, E4, VE2, ABS_E, LN_V, SQRT_V = range(14)
TAKEN, SKIPPED, IN68, IN95, PIT0 = 0, 1, 2, 3, 4
WORST = 5


# ---- from the accumulators to numbers (Python fp64) --------------------------------------------------------------------------------------
def _finite(v):
    return v if v is not None and math.isfinite(v) else None


def _ratio(a, b):
    return _finite(a / b) if b else None


def _central(sxy, sx, sy, n) -> float:
    """sxy / n - (sx / n)(sy / n) from three sums, the difference formed EXACTLY (rationals) and rounded once: formed in fp64 it
    would add a rounding of the size of the product, mean^2 / variance times larger than that of the result."""
    return float(Fraction(sxy) / n - Fraction(sx) * Fraction(sy) / (n * n))


def summarise(acc, cnt) -> dict:
    """acc [rows][14] sums and cnt [rows][14] counts (nested lists, dvg_gp_score's slots) -> the scores of the rows POOLED:
    sums are added with math.fsum, counts as integers.  A quantity with nothing finite behind it is None."""
    s = [math.fsum(float(row[k]) for row in acc) for k in range(14)]
    c = [sum(int(row[k]) for row in cnt) for k in range(14)]
    n = c[TAKEN]
    out = {"taken": n, "skipped": c[SKIPPED]}
    names = ("nlpd", "rmse", "mae", "mean_var", "z_mean", "z_std", "cover68", "cover95", "pit", "pit_err", "var_err_corr", "smse")
    if n == 0 or not all(math.isfinite(v) for v in s):
        out.update({k: None for k in names})
        return out
    mean = [v / n for v in s]
    out["nlpd"] = mean[NLPD]
    out["rmse"] = math.sqrt(max(0.0, mean[E2]))
    out["mae"] = mean[ABS_E]
    out["mean_var"] = mean[V]
    out["z_mean"] = mean[Z]
    out["z_std"] = math.sqrt(max(0.0, _central(s[Z2], s[Z], s[Z], n)))
    out["cover68"], out["cover95"] = c[IN68] / n, c[IN95] / n
    out["pit"] = [c[PIT0 + k] / n for k in range(10)]
    out["pit_err"] = 0.5 * math.fsum(abs(p - 0.1) for p in out["pit"])
    # Pearson of v and e^2 from their pooled moments; a variance that is zero up to the rounding of its two terms has none
    var_v, var_e2, cov = _central(s[V2], s[V], s[V], n), _central(s[E4], s[E2], s[E2], n), _central(s[VE2], s[V], s[E2], n)
    ok = var_v > 1e-12 * mean[V2] and var_e2 > 1e-12 * mean[E4]
    out["var_err_corr"] = _finite(cov / math.sqrt(var_v * var_e2)) if ok else None
    # the squared error against that of predicting the targets' mean; targets without variance have none
    spread = n * _central(s[Y2], s[Y], s[Y], n)
    out["smse"] = _ratio(s[E2], spread) if spread > 1e-12 * s[Y2] else None
    return out


def report(acc, cnt, steps: int, dims: int) -> dict:
    """The rows are (step, dim), step-major: {"pooled": all rows, "per_step": one summary per step (its dims pooled), "per_dim": one
    per latent dim (its steps pooled), "worst_dims": the five dims with the largest nlpd, worst first}."""
    if len(acc) != steps * dims or len(cnt) != steps * dims:
        raise ValueError(f"gp_score.report: {len(acc)} rows are not {steps} steps x {dims} dims")
    rows = lambda idx: ([acc[r] for r in idx], [cnt[r] for r in idx])    # noqa: E731
    per_step = [summarise(*rows(range(s * dims, (s + 1) * dims))) for s in range(steps)]
    per_dim = [summarise(*rows(range(d, steps * dims, dims))) for d in range(dims)]
    scored = [d for d in range(dims) if per_dim[d]["nlpd"] is not None]
    worst = sorted(scored, key=lambda d: (-per_dim[d]["nlpd"], d))[:WORST]
    return {"pooled": summarise(acc, cnt), "per_step": per_step, "per_dim": per_dim, "worst_dims": worst}


def _num(v) -> float:
    return float("nan") if v is None else float(v)


def line(tag: str, gp: dict) -> str:
    """`     val gp: nlpd .. rmse .. mean var .. z std .. cover 68/95 .. / .. pit err .. var~err corr ..  | rollout: nlpd .. z std ..
    cover 95 ..` from {"forced": report, "rollout": report}; a number nothing finite went into prints as nan."""
    f, r = gp["forced"]["pooled"], gp["rollout"]["pooled"]
    return ('     %s: nlpd %.4f rmse %.5f mean var %.5f z std %.3f cover 68/95 %.3f / %.3f pit err %.3f var~err corr %.3f'
            '  | rollout: nlpd %.4f z std %.3f cover 95 %.3f' % (
                tag, _num(f["nlpd"]), _num(f["rmse"]), _num(f["mean_var"]), _num(f["z_std"]), _num(f["cover68"]),
                _num(f["cover95"]), _num(f["pit_err"]), _num(f["var_err_corr"]), _num(r["nlpd"]), _num(r["z_std"]),
                _num(r["cover95"])))


def curves(tag: str, rep: dict) -> str:
    """The per-step nlpd and cover95 of one track, one line each (generate_frames.py --gp_report)."""
    return '     %s nlpd by step: %s\n     %s cover 95 by step: %s' % (
        tag, ' '.join('%.3f' % _num(s["nlpd"]) for s in rep["per_step"]),
        tag, ' '.join('%.3f' % _num(s["cover95"]) for s in rep["per_step"]))


def write_report(gp: dict, directory: str) -> str:
    """<directory>/gp_report.json through a temporary name: at every instant a complete file (as validate.write_log)."""
    from .validate import _plain
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, FILE)
    tmp = f"{path}.tmp.{os.getpid()}"
    try:
        with open(tmp, "w") as f:
            f.write(json.dumps(_plain(gp), sort_keys=True) + "\n")
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


# ---- the scorer ----------------------------------------------------------------------------------------------------------------------
def track_steps(n_past: int, n_eval: int) -> dict:
    """Steps per track: forced scores the targets i = 1 ... n_eval - 1, rollout i = n_past ... n_eval - 1."""
    return {"forced": n_eval - 1, "rollout": n_eval - n_past}


class GPScorer:
    """The accumulators of both tracks - rows (step, dim) - and the calls that feed them.

    forced   the GP input is enc(x[i - 1])[0], the target enc(x[i])[0], i = 1 ... n_eval - 1: both on ground-truth frames.
    rollout  the GP input is enc(xhat[i - 1])[0], xhat the frames of the posterior rollout (xhat = x while i - 1 < n_past), the
             target enc(x[i])[0], i = n_past ... n_eval - 1: what rollout.sample_from and GPtrigger_gen ask the GP.

    The caller puts every module in eval mode; everything here runs under no_grad.  The predictive is the likelihood's: the latent
    moments of gp_layer(h) and the likelihood's noise variances, added in fp64 inside dvg_gp_score.  Per batch and track: one
    encoder call, one GP call per step, ONE dvg_gp_score launch; nothing is read back before `read()`."""

    def __init__(self, dims: int, steps, device):
        from . import ops
        self.dims, self.steps, self.dev = int(dims), {t: int(steps[t]) for t in TRACKS}, torch.device(device)
        if self.dims < 1 or min(self.steps.values()) < 1:
            raise ValueError(f"GPScorer: {dims} dims and {steps} steps leave nothing to score")
        self.acc, self.cnt = {}, {}
        for t in TRACKS:
            self.acc[t], self.cnt[t] = ops.gp_score_accumulators(self.steps[t] * self.dims, self.dev)

    def zero(self) -> None:
        for t in TRACKS:
            self.acc[t].zero_()
            self.cnt[t].zero_()

    def _track(self, track, gp_layer, noise, h_in, h_target):
        """h_in, h_target (S, B, D): the GP inputs and the targets of the S steps of one batch."""
        from . import ops, rollout
        S, B, D = h_in.shape
        preds = [gp_layer(rollout.gp_input(gp_layer, h_in[s])) for s in range(S)]
        mean = torch.cat([p.mean for p in preds])                      # (S D, B), rows (step, dim)
        var = torch.cat([p.variance for p in preds])
        target = h_target.permute(1, 0, 2).reshape(B, S * D).t()       # (S D, B) with strides (1, S D): the kernel takes it as it is
        ops.gp_score(mean, var, target, self.acc[track], self.cnt[track], noise=noise, noise_period=D)

    @torch.no_grad()
    def score(self, encoder, gp_layer, likelihood, x, xhat, n_past: int, n_eval: int) -> None:
        """One batch: x the ground-truth frames, xhat the posterior rollout's (xhat[i] is x[i] for i < n_past)."""
        from . import rollout
        B, D = x[0].shape[0], self.dims
        if track_steps(n_past, n_eval) != self.steps:
            raise ValueError(f"GPScorer.score: n_past {n_past}, n_eval {n_eval} are not the steps {self.steps} it was made for")
        gt = rollout.frames_as_batch(list(x[:n_eval]))
        h = rollout._encode(encoder, gt, gt.shape[0])[0].view(n_eval, B, D)
        noise = likelihood.noise.contiguous()
        self._track("forced", gp_layer, noise, h[:n_eval - 1], h[1:])
        fed = rollout.frames_as_batch(list(xhat[n_past - 1:n_eval - 1]))
        h_fed = rollout._encode(encoder, fed, fed.shape[0])[0].view(n_eval - n_past, B, D)
        self._track("rollout", gp_layer, noise, h_fed, h[n_past:])

    def read(self) -> dict:
        """{"forced": report, "rollout": report}: the one readback."""
        flat = torch.cat([self.acc[t].flatten() for t in TRACKS] + [self.cnt[t].flatten().double() for t in TRACKS]).cpu()
        out, at = {}, 0
        parts = {}
        for kind in ("acc", "cnt"):
            for t in TRACKS:
                n = self.acc[t].numel()
                parts[kind, t] = flat[at:at + n].view(self.acc[t].shape)
                at += n
        for t in TRACKS:
            out[t] = report(parts["acc", t].tolist(), parts["cnt", t].long().tolist(), self.steps[t], self.dims)
        return out
