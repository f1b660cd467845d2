"""fp64 numpy restatement of the weight average (ema.hip, dvg_amd/ema.py: WeightAverage): the decay schedule, the update on
fp32-rounded inputs and the two sums that measure the lag.  The reference project averages nothing, so this arithmetic is the
oracle."""
import numpy as np

CHUNK = 8192           # floats per pair of partial sums of dvg_ema_update


def blocks(n):
    return 0 if n <= 0 else (n + CHUNK - 1) // CHUNK


def decay_at(decay, k):
    """The decay of the update that follows k applied ones: the warm-up (1 + k) / (10 + k) until it reaches `decay`."""
    return min(float(decay), (1.0 + k) / (10.0 + k))


def update(e, p, decay, k):
    """One update in fp64 on the fp32 values: e + w (p - e) with the weight w = 1 - decay_at(decay, k) rounded to fp32 as the
    kernel holds it.  Returns fp64 (the caller rounds, or keeps the exact chain)."""
    e = np.asarray(e, dtype=np.float64)
    p = np.asarray(p, dtype=np.float32).astype(np.float64)
    w = np.float64(np.float32(1.0 - decay_at(decay, k)))
    with np.errstate(invalid="ignore", over="ignore"):
        return e + w * (p - e)


def sums(p, e):
    """(sum (p - e)^2, sum p^2) in fp64 over the fp32 values, as the kernel forms each term; per chunk with chunk_sums."""
    p = np.asarray(p, dtype=np.float32).astype(np.float64).ravel()
    e = np.asarray(e, dtype=np.float32).astype(np.float64).ravel()
    with np.errstate(invalid="ignore", over="ignore"):
        d = p - e
        return float(np.sum(d * d)), float(np.sum(p * p))


def chunk_sums(p, e):
    p, e = np.asarray(p).ravel(), np.asarray(e).ravel()
    return np.array([sums(p[i:i + CHUNK], e[i:i + CHUNK]) for i in range(0, p.size, CHUNK)]).reshape(-1)


def lag(p, e):
    a, b = sums(p, e)
    return float(np.sqrt(a) / np.sqrt(b))


def closed_form(c, decay, K):
    """A constant parameter c and e_0 = 0: e_K = c (1 - prod_{k < K} d_k)."""
    prod = 1.0
    for k in range(K):
        prod *= decay_at(decay, k)
    return c * (1.0 - prod)
