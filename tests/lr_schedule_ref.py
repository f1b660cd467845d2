"""The learning-rate multiplier of train.py --lr_schedule, restated in fp64 on the host: the oracle of tests/test_lr_schedule_host.py
and tests/test_gpu_lr_schedule.py.  The reference project has no counterpart (its train.py hard-codes lr = 0.002).

k = training iterations completed before this one (iterations whose step a guard skipped included), W = warm-up iterations,
N = total iterations, R = floor ratio in [0, 1]; for `step`: the factor G every K iterations.

    k < W      s = (k + 1) / W
    else       u = min(1, (k - W) / max(1, N - W))
      constant s = 1
      linear   s = R + (1 - R)(1 - u)
      cosine   s = R + (1 - R) . 1/2 (1 + cos(pi u))
      step     s = max(R, G^floor((k - W) / K))

Every operation is a Python float operation - fp64, rounded on its own, no fused multiply-add -, and `s32` rounds the result once to
fp32.  Where cos and pow are exact (constant, linear, and step with dyadic G) a device that does the same operations in the same
order gives the same bits; elsewhere its cos / pow may differ in the last fp64 bits, which moves the fp32 rounding by at most one
step."""
import math

import numpy as np

KINDS = ("constant", "linear", "cosine", "step")
INT_MAX = 2 ** 31 - 1


def s(kind: str, k: int, W: int, N: int, R: float = 0.0, K: int = 1, G: float = 1.0) -> float:
    """The multiplier of the iteration that follows k completed ones, fp64."""
    assert kind in KINDS and k >= 0 and 0 <= W < N and 0.0 <= R <= 1.0
    if k < W:
        return (k + 1.0) / W
    u = min(1.0, float(k - W) / float(max(1, N - W)))
    if kind == "constant":
        return 1.0
    if kind == "linear":
        return R + (1.0 - R) * (1.0 - u)
    if kind == "cosine":
        return R + (1.0 - R) * (0.5 * (1.0 + math.cos(math.pi * u)))
    assert K >= 1 and 0.0 < G <= 1.0
    return max(R, math.pow(G, float((k - W) // K)))


def s32(kind: str, k: int, W: int, N: int, R: float = 0.0, K: int = 1, G: float = 1.0) -> np.float32:
    """s rounded once to fp32: what the device holds."""
    return np.float32(s(kind, k, W, N, R, K, G))


def ulps32(a, b) -> int:
    """The distance of two finite fp32 values of one sign in units of the last place."""
    ia, ib = (int(np.array(x, dtype=np.float32).view(np.int32)) for x in (a, b))
    return abs(ia - ib)
