"""fp64 numpy reference of the sample-diversity numbers (dvg_pairwise_frame_mse, utils.sample_diversity): plain differences,
no norm expansion.  The reference project computes nothing between samples, so this arithmetic is the oracle."""
import numpy as np


def pairwise_frame_mse(samples, lo=None, hi=None):
    """samples (S,T,B,C,H,W) -> (hi - lo, B, S, S) float64: [t, b, i, j] = mean_d (x[i, lo+t, b, d] - x[j, lo+t, b, d])^2."""
    s, t, b = samples.shape[:3]
    lo, hi = 0 if lo is None else lo, t if hi is None else hi
    x = samples[:, lo:hi].reshape(s, hi - lo, b, -1).astype(np.float64)
    out = np.zeros((hi - lo, b, s, s))
    for i in range(s):                      # one row at a time: (S, steps, B, D) doubles, not S times that
        out[:, :, i, :] = np.moveaxis(((x[i][None] - x) ** 2).mean(-1), 0, -1)
    return out


def distinct(matrix):
    """(..., S, S) -> (...) int: samples s with matrix[s, j] > 0 for every j < s, i.e. different frames among the samples."""
    s = matrix.shape[-1]
    first = (matrix > 0) | np.triu(np.ones((s, s), dtype=bool))
    return first.all(-1).sum(-1)


def diversity(matrix):
    """(T_pred, B, S, S) -> pair_mse, pair_psnr (B, T_pred) float64 and distinct (B, T_pred) int, as utils.sample_diversity."""
    s = matrix.shape[-1]
    iu = np.triu_indices(s, 1)
    pair = matrix.astype(np.float64)[..., iu[0], iu[1]].mean(-1) if s > 1 else np.zeros(matrix.shape[:2])
    with np.errstate(divide="ignore"):
        psnr = 10.0 * np.log10(1.0 / pair)
    return pair.T, psnr.T, distinct(matrix).T
