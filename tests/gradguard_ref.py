"""fp64 numpy restatement of the gradient guard (grad_guard.hip, dvg_amd/optim.py: GradGuard / guarded_step): the norm, the clip
factor of torch.nn.utils.clip_grad_norm_, the skip rule, and Adam on the clipped gradient.  The reference project clips nothing,
so this arithmetic - and torch's own clip_grad_norm_ / optim.Adam, which the GPU tests run beside it - is the oracle."""
import numpy as np

CHUNK = 16384          # floats per partial sum of dvg_grad_sumsq


def blocks(n):
    return 0 if n <= 0 else (n + CHUNK - 1) // CHUNK


def sumsq(g):
    """The fp64 sum of squares; each square is formed in fp64 (exact for fp32 inputs)."""
    x = np.asarray(g, dtype=np.float32).astype(np.float64).ravel()
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.sum(x * x))


def norm(g):
    with np.errstate(invalid="ignore"):
        return float(np.sqrt(sumsq(g)))


def scale(nrm, max_norm):
    """min(1, C / (norm + 1e-6)) as torch.clamp(max=1.0) gives it: 0 for an infinite norm, NaN for a NaN one; 1 when C <= 0."""
    if max_norm <= 0:
        return 1.0
    with np.errstate(invalid="ignore"):
        c = np.float64(max_norm) / (np.float64(nrm) + 1e-6)
    return float(c) if not c > 1.0 else 1.0


def verdict(g, max_norm, skip_nonfinite):
    """(norm, scale, skip) of one step site."""
    s = sumsq(g)
    n = norm(g)
    return n, scale(n, max_norm), bool(skip_nonfinite and not np.isfinite(s))


def adam_sequence(params, grads_per_step, max_norm, lrs, betas=(0.9, 0.999), eps=1e-8, weight_decays=None):
    """fp64 Adam (torch.optim.Adam, non-amsgrad) over a list of parameters with ONE clip factor per step over all gradients.
    grads_per_step[t][i]: gradient of parameter i at step t; lrs[t][i] and weight_decays[i] per parameter.  Returns the final
    parameters and the per-step (norm, scale)."""
    p = [np.asarray(x, dtype=np.float64).copy() for x in params]
    m = [np.zeros_like(x) for x in p]
    v = [np.zeros_like(x) for x in p]
    wd = weight_decays or [0.0] * len(p)
    b1, b2 = betas
    trace = []
    for t, grads in enumerate(grads_per_step, 1):
        nrm = float(np.sqrt(sum(sumsq(g) for g in grads)))
        sc = scale(nrm, max_norm)
        trace.append((nrm, sc))
        for i, g in enumerate(grads):
            gg = np.asarray(g, dtype=np.float64) * sc + wd[i] * p[i]
            m[i] = b1 * m[i] + (1 - b1) * gg
            v[i] = b2 * v[i] + (1 - b2) * gg * gg
            bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
            p[i] = p[i] - (lrs[t - 1][i] / bc1) * m[i] / (np.sqrt(v[i]) / np.sqrt(bc2) + eps)
    return p, trace
