"""A numpy fp64 restatement of dvg_val_accumulate (include/dvg_hip.h, dvg_amd/csrc/validate.hip) in plain sequential loops - no
np.sum, whose pairwise order would not reproduce the `best` rule's sums - for tests/test_validate_host.py and
tests/test_gpu_validate.py.  Also the inputs the GPU kernel tests use and the bar they hold the kernel to."""
import math

import numpy as np

SHAPES = [(1, 1, 1), (1, 3, 2), (4, 1, 5), (5, 7, 3), (64, 5, 10), (3, 100, 17), (130, 2, 33)]


def best_samples(ssim):
    """best[b]: the sample with the largest fp64 sum over t (from 0.0, t ascending) of ssim[b, s, t]; a NaN sum loses to every
    non-NaN sum, ties go to the lowest s, all NaN gives 0."""
    B, S, T = ssim.shape
    best = np.zeros(B, np.int32)
    for b in range(B):
        top, have = 0.0, False
        for s in range(S):
            tot = np.float64(0.0)
            for t in range(T):
                tot = tot + np.float64(ssim[b, s, t])
            if not math.isnan(tot) and (not have or tot > top):
                best[b], top, have = s, tot, True
    return best


def accumulate(ssim, psnr, mse, acc=None, cnt=None, absolute=False):
    """(acc, cnt, best) after one call: acc (2, 3, T, 2) fp64 and cnt (2, 3, T) int64 are added to (fresh zeros when None), rows in
    ascending b.  absolute: add |v| and |u| instead of v and u (`absum`: what the kernel tests scale their bar with)."""
    B, S, T = ssim.shape
    acc = np.zeros((2, 3, T, 2), np.float64) if acc is None else acc
    cnt = np.zeros((2, 3, T), np.int64) if cnt is None else cnt
    best = best_samples(ssim)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(B):
            for m, arr in enumerate((ssim, psnr, mse)):
                for t in range(T):
                    v = np.float64(arr[b, best[b], t])
                    if math.isfinite(v):
                        acc[0, m, t, 0] += abs(v) if absolute else v
                        acc[0, m, t, 1] += v * v
                        cnt[0, m, t] += 1
                    tot, n = np.float64(0.0), 0
                    for s in range(S):
                        x = np.float64(arr[b, s, t])
                        if math.isfinite(x):
                            tot = tot + x
                            n += 1
                    if n:
                        u = tot / np.float64(n)
                        acc[1, m, t, 0] += abs(u) if absolute else u
                        acc[1, m, t, 1] += u * u
                        cnt[1, m, t] += 1
    return acc, cnt, best


def absum(ssim, psnr, mse):
    """(2, 3, T, 2): per entry of acc, the sum of the absolute values of the terms one call adds to it."""
    return accumulate(ssim, psnr, mse, absolute=True)[0]


def bar(B, S, total_abs):
    """(B + S) 2^-52 sum |terms|: fp64 summation of at most B terms in any order (each side errs by at most (B - 1) 2^-53 of it),
    plus the inner mean over S samples."""
    return (B + S) * 2.0 ** -52 * total_abs


def inputs(B, S, T, seed=0):
    """The kernel tests' inputs: ssim uniform in [-1, 1] with sample 2 a copy of sample 1 when S > 2 (exact ties); about 10 % of
    psnr +inf, and all of step 0 when B > 2; about 5 % of mse NaN."""
    rng = np.random.default_rng(1000 * seed + 100 * B + 10 * S + T)
    ssim = rng.uniform(-1.0, 1.0, (B, S, T)).astype(np.float32)
    if S > 2:
        ssim[:, 2] = ssim[:, 1]
    psnr = rng.uniform(10.0, 40.0, (B, S, T)).astype(np.float32)
    psnr[rng.random((B, S, T)) < 0.10] = np.inf
    if B > 2:
        psnr[:, :, 0] = np.inf
    mse = rng.uniform(0.0, 0.1, (B, S, T)).astype(np.float32)
    mse[rng.random((B, S, T)) < 0.05] = np.nan
    return ssim, psnr, mse
