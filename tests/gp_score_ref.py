"""A numpy fp64 restatement of dvg_gp_score's per-entry rules (include/dvg_hip.h, dvg_amd/csrc/gp_score.hip) for
tests/test_gp_score_host.py and tests/test_gpu_gp_score.py: the sums are math.fsum of the terms (correctly rounded: the reference
has no summation error of its own), the counts are decided by the same two IEEE products as in the kernel.  Also the seeded input
sets of the GPU kernel tests, the margin that makes their counts a fair comparison, and the bar on the sums."""
import math

import numpy as np

ACC, CNT = 14, 14
LN_2PI = math.log(2.0 * math.pi)
CHI2_95 = 3.8414588206941236
# the signed squares of the standard normal's quantiles at 0.1 ... 0.9
EDGES = (-1.6423744151498172, -0.708326300800794, -0.2749958977284559, -0.06418475466730157, 0.0,
         0.06418475466730157, 0.2749958977284559, 0.708326300800794, 1.6423744151498172)
# (R, B, noise period): one entry; below / at / above a wave; a second pass of a thread (B > 256); a period that is not R; the
# shape of a validation batch's rows (90 latent dims) with B a multiple of the workgroup's waves
SHAPES = [(1, 1, 0), (1, 63, 0), (2, 64, 0), (3, 65, 0), (5, 257, 0), (15, 33, 5), (90, 128, 0)]
MARGIN = 1e-9
REL_BAR = 1e-13


def _entries(mean, var, noise, period, target):
    """Per entry in fp64: (taken mask, v, y, e) with v = var + noise[r % P]."""
    m, s, y = (np.asarray(a, np.float32).astype(np.float64) for a in (mean, var, target))
    R, B = m.shape
    if noise is None:
        nz = np.zeros((R, 1))
    else:
        P = period or R
        assert R % P == 0 and len(noise) == P
        nz = np.asarray(noise, np.float32).astype(np.float64)[np.arange(R) % P][:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        v = s + nz
        taken = np.isfinite(m) & np.isfinite(s) & np.isfinite(y) & (v > 0.0)
        e = y - m
    return taken, v, y, e


def terms(v, y, e):
    """The 14 terms of one row's taken entries, in the kernel's slot order: (14, n)."""
    e2 = e * e
    q = e2 / v
    lv, sv = np.log(v), np.sqrt(v)
    return np.stack([0.5 * ((LN_2PI + lv) + q), e, e2, v, e / sv, q, y, y * y, v * v, e2 * e2, v * e2, np.abs(e), lv, sv])


def accumulate(mean, var, noise, period, target, acc=None, cnt=None):
    """(acc, cnt, absum): acc (R, 14) fp64 and cnt (R, 14) int64 after one call, added to when given (fresh zeros when None);
    absum (R, 14): per entry of acc the sum of the |terms| this call adds - what the bar on the kernel's sums scales with."""
    taken, v, y, e = _entries(mean, var, noise, period, target)
    R = taken.shape[0]
    acc = np.zeros((R, ACC), np.float64) if acc is None else acc
    cnt = np.zeros((R, CNT), np.int64) if cnt is None else cnt
    absum = np.zeros((R, ACC), np.float64)
    for r in range(R):
        k = taken[r]
        cnt[r, 0] += int(k.sum())
        cnt[r, 1] += int((~k).sum())
        if not k.any():
            continue
        vr, yr, er = v[r, k], y[r, k], e[r, k]
        t = terms(vr, yr, er)
        for q in range(ACC):
            acc[r, q] = math.fsum([acc[r, q]] + t[q].tolist())
            absum[r, q] = math.fsum(np.abs(t[q]).tolist())
        e2, se = er * er, er * np.abs(er)
        cnt[r, 2] += int((e2 <= vr).sum())
        cnt[r, 3] += int((e2 <= CHI2_95 * vr).sum())
        decile = sum((se > c * vr).astype(np.int64) for c in EDGES)
        cnt[r, 4:] += np.bincount(decile, minlength=10)
    return acc, cnt, absum


def margins(inputs) -> float:
    """The smallest relative distance of a taken entry from an edge of a count: |e |e| - c_j v| / max(|c_j v|, tiny) over the nine
    PIT edges and |e^2 - c v| / (c v) over the two coverage edges.  An entry this close to an edge could fall on either side of
    it by the rounding of one product: the count comparisons use inputs that keep away from all of them."""
    taken, v, y, e = _entries(*inputs)
    v, e = v[taken], e[taken]
    if v.size == 0:
        return math.inf
    tiny = np.finfo(np.float64).tiny
    se, e2 = e * np.abs(e), e * e
    out = min(float((np.abs(e2 - c * v) / (c * v)).min()) for c in (1.0, CHI2_95))
    with np.errstate(over="ignore"):           # (the edge at 0: a distance over `tiny`)
        for c in EDGES:
            out = min(out, float((np.abs(se - c * v) / np.maximum(np.abs(c * v), tiny)).min()))
    return out


def bar(absum):
    """1e-13 sum|terms| per slot.  From the kernel's form: each term is a handful of ulp from exact (log, sqrt, two divisions) and the
    sum of B terms - B / 256 per thread, six butterfly levels, four waves - adds at most (B / 256 + 10) 2^-53 of sum|terms|: about
    3e-15 for the shapes here; the bar is some 30 times that."""
    return REL_BAR * absum


def inputs(R, B, period=0, noise=True, seed=0):
    """(mean, var, noise or None, period, target), fp32: mean ~ N(0, 1), var log-normal around e^-1, noise variances in [0.01, 0.2],
    target = mean + a N(0, 1.2^2 v) residual (a little over-dispersed, so that every PIT decile and both coverage counts are
    exercised).  With 32 entries or more: NaN, +inf and -inf in each of the three inputs, var = 0 (skipped without noise, taken
    with it) and negative variances (one that the noise does not bring above 0, one that it does)."""
    rng = np.random.default_rng(100000 * seed + 1000 * R + 10 * B + period + (5 if noise else 0))
    mean = rng.standard_normal((R, B)).astype(np.float32)
    var = np.exp(rng.normal(-1.0, 1.0, (R, B))).astype(np.float32)
    nz = rng.uniform(0.01, 0.2, period or R).astype(np.float32) if noise else None
    full = var.astype(np.float64) + (0.0 if nz is None else nz.astype(np.float64)[np.arange(R) % (period or R)][:, None])
    target = (mean.astype(np.float64) + 1.2 * np.sqrt(full) * rng.standard_normal((R, B))).astype(np.float32)
    if R * B >= 32:
        specials = [(a, bad) for a in (mean, var, target) for bad in (np.nan, np.inf, -np.inf)] + \
                   [(var, 0.0), (var, -0.5), (var, -0.005)]
        for k, (a, bad) in enumerate(specials):
            a.reshape(-1)[(5 + 7 * k) % (R * B)] = bad
    return mean, var, nz, period, target


def case(R, B, period=0, noise=True):
    """The input set of a kernel test, checked to keep MARGIN away from every edge (a condition on the inputs, asserted here on
    the CPU, not a tolerance of the kernel)."""
    x = inputs(R, B, period, noise)
    got = margins(x)
    assert got >= MARGIN, f"input set {(R, B, period, noise)}: margin {got:.3e} < {MARGIN}: choose another seed"
    return x
