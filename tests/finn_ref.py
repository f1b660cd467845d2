"""CPU restatement (numpy, fp64) of the reference's Finn-style metrics, utils.finn_eval_seq (utils.py:236-301), and the seeded
inputs shared by tests/golden/make_golden_finn.py, tests/test_finn_host.py and tests/test_gpu_finn*.py.

The reference filters with scipy.signal.fftconvolve; here the five moments are DIRECT fp64 sums over the 11x11 window at every
valid position.  tests/golden/reference_finn.npz (written by make_golden_finn.py from the reference's own finn_ssim,
finn_psnr and mse_metric) pins this restatement to 1e-10; the .npz holds outputs only, the inputs come from `case(name)`."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

WIN, SIGMA, K1, K2, L = 11, 1.5, 0.01, 0.03, 1.0


def window():
    """11x11 Gaussian taps exp(-(i^2 + j^2) / (2 sigma^2)), i, j = -5 ... 5, normalised to sum 1."""
    i = np.arange(WIN, dtype=np.float64) - WIN // 2
    g = np.exp(-(i[:, None] ** 2 + i[None, :] ** 2) / (2.0 * SIGMA ** 2))
    return g / g.sum()


def _filter(a, g):
    return np.einsum("ijkl,kl->ij", sliding_window_view(a, (WIN, WIN)), g)


def ssim_map(x, y):
    """The (H-10, W-10) SSIM map of two 2-D images (utils.py:275-301)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    g = window()
    c1, c2 = (K1 * L) ** 2, (K2 * L) ** 2
    mx, my = _filter(x, g), _filter(y, g)
    vx, vy, vxy = _filter(x * x, g) - mx * mx, _filter(y * y, g) - my * my, _filter(x * y, g) - mx * my
    with np.errstate(invalid="ignore"):
        return ((2 * mx * my + c1) * (2 * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def per_channel(gt, pred):
    """gt, pred (N,C,H,W) -> (ssim map means (N,C) - NaN kept -, psnr (N,C), mse (N,)), all fp64."""
    gt, pred = np.asarray(gt, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    n, c = gt.shape[:2]
    ssim, psnr = np.zeros((n, c)), np.zeros((n, c))
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(n):
            for k in range(c):
                ssim[i, k] = ssim_map(gt[i, k], pred[i, k]).mean()
                psnr[i, k] = 10.0 * np.log10(1.0 / ((gt[i, k] - pred[i, k]) ** 2).mean())
        mse = ((gt - pred) ** 2).reshape(n, -1).sum(1) / float(np.prod(gt.shape[1:]))
    return ssim, psnr, mse


def assemble(ssim_c, psnr_c):
    """finn_eval_seq's channel average (utils.py:245-253): a NaN map mean counts as -1."""
    return np.where(np.isnan(ssim_c), -1.0, ssim_c).mean(1), psnr_c.mean(1)


def evaluate(gt, pred):
    """(ssim, psnr, mse), each (N,) fp64, of (N,C,H,W) frames: what finn_eval_seq puts into one column of its arrays."""
    s, p, m = per_channel(gt, pred)
    return assemble(s, p) + (m,)


def eval_seq(gt, pred):
    """utils.finn_eval_seq's return value (mse, ssim, psnr), each (bs, T), from sequences of T (bs,C,H,W) arrays."""
    cols = [evaluate(g, p) for g, p in zip(gt, pred)]
    return tuple(np.stack([c[k] for c in cols], 1) for k in (2, 0, 1))


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------
def _noise(rs, shape, lo=0.0, hi=1.0, sd=0.05):
    gt = rs.uniform(lo, hi, size=shape).astype(np.float32)
    return gt, (gt + rs.normal(0.0, sd, size=shape)).astype(np.float32)


def _sparse(rs, shape):
    """Mostly zero frames with one textured block, against a copy shifted by (2, 3) and scaled by 0.8: most windows are flat
    (sigma^2 ~ 0 against C2 = 9e-4)."""
    n, c, h, w = shape
    gt, pred = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    bh, bw = max(4, h // 3), max(4, w // 3)
    for i in range(n):
        for k in range(c):
            y0, x0 = rs.randint(0, h - bh - 2), rs.randint(0, w - bw - 3)
            blk = rs.uniform(0.2, 1.0, size=(bh, bw)).astype(np.float32)
            gt[i, k, y0:y0 + bh, x0:x0 + bw] = blk
            pred[i, k, y0 + 2:y0 + 2 + bh, x0 + 3:x0 + 3 + bw] = np.float32(0.8) * blk
    return gt, pred


def _const(rs, shape):
    return np.full(shape, 0.25, np.float32), np.full(shape, 0.75, np.float32)


# name: (builder, (N,C,H,W), keyword arguments); the seed is the name's position
CASES = {
    "noise_11x11": (_noise, (2, 1, 11, 11), {}),
    "noise_12x17": (_noise, (2, 1, 12, 17), {}),
    "noise_64_c1": (_noise, (2, 1, 64, 64), {}),
    "noise_64_c3": (_noise, (2, 3, 64, 64), {}),
    "noise_128_c1": (_noise, (1, 1, 128, 128), {}),
    "sparse_12x17": (_sparse, (2, 1, 12, 17), {}),
    "sparse_64_c1": (_sparse, (2, 1, 64, 64), {}),
    "sparse_64_c3": (_sparse, (1, 3, 64, 64), {}),
    "sparse_128_c3": (_sparse, (1, 3, 128, 128), {}),
    "const_11x11": (_const, (1, 1, 11, 11), {}),
    "const_64_c3": (_const, (1, 3, 64, 64), {}),
    "signed_64_c1": (_noise, (2, 1, 64, 64), {"lo": -0.5, "hi": 0.5}),
    "signed_12x17_c3": (_noise, (1, 3, 12, 17), {"lo": -0.5, "hi": 0.5}),
    "noise_16_x130": (_noise, (130, 1, 16, 16), {}),
}


def case(name):
    """(gt, pred), fp32 (N,C,H,W)."""
    fn, shape, kw = CASES[name]
    return fn(np.random.RandomState(9100 + sorted(CASES).index(name)), shape, **kw)
