"""fp64 reference (torch, CPU) of the DSSIM frame term of train.py --ssim_weight (dvg_frame_ssim_loss, dvg_amd.frame_loss.torch_ssim_sum)
and the seeded inputs shared by tests/test_ssim_loss_host.py and tests/test_gpu_ssim_loss.py.

    pred (S, K, planes, H, W), target (S, planes, H, W);  sums[k] = sum over steps, planes and the (H-10) x (W-10) window positions
    of 1 - SSIM(target, pred[:, k]), SSIM = tests/finn_ref.ssim_map;  gradient = d(sum_k w[k] sums[k]) / d pred.

The VALUE is built on finn_ref.ssim_map (direct 121-tap sums; pinned to the reference's own finn_ssim by reference_finn.npz).  The
GRADIENT is the closed form of docs/DESIGN_NOTES_frame_loss.md (`formula`), which tests/test_ssim_loss_host.py checks against fp64
autograd of the slice composition and against central differences.  `formula(..., defect=NAME)` plants one of DEFECTS."""
import numpy as np
import torch

from tests import finn_ref

WIN = finn_ref.WIN
C1, C2 = (finn_ref.K1 * finn_ref.L) ** 2, (finn_ref.K2 * finn_ref.L) ** 2
DEFECTS = ("a_without_its_B2_term", "b_with_the_wrong_sign", "back_filter_shifted_by_one", "factor_2_on_P_full_b_dropped")
KINDS = ("noise", "sparse", "const", "identical")


def taps():
    """The 1-D window: the 11x11 window of finn_ref.window() is its outer product."""
    i = torch.arange(WIN, dtype=torch.float64) - WIN // 2
    g = torch.exp(-i * i / (2.0 * finn_ref.SIGMA ** 2))
    return g / g.sum()


def valid(a):
    """The window over the valid positions of (..., H, W) -> (..., H-10, W-10), separably, fp64."""
    g = taps()
    wo, ho = a.shape[-1] - WIN + 1, a.shape[-2] - WIN + 1
    rows = sum(g[k] * a[..., k:k + wo] for k in range(WIN))
    return sum(g[k] * rows[..., k:k + ho, :] for k in range(WIN))


def full(m, shift=0):
    """The transpose of `valid`: (..., Ho, Wo) -> (..., Ho+10, Wo+10), full(m)[q] = sum_k g[k] m[q - k] along both axes.  `shift`
    = 1 plants the misalignment defect (the map read one position off along x)."""
    g = taps()
    ho, wo = m.shape[-2], m.shape[-1]
    out = m.new_zeros(m.shape[:-2] + (ho + WIN - 1, wo + WIN - 1))
    cols = m.new_zeros(m.shape[:-2] + (ho + WIN - 1, wo))
    for k in range(WIN):
        cols[..., k:k + ho, :] += g[k] * m
    if shift:
        cols = torch.roll(cols, shift, -1)
    for k in range(WIN):
        out[..., k:k + wo] += g[k] * cols
    return out


def sums(pred, target):
    """(K,) fp64: sum (1 - SSIM) per call, every image through finn_ref.ssim_map."""
    S, K, planes = pred.shape[:3]
    out = np.zeros(K)
    p, t = pred.double().numpy(), target.double().numpy()
    for k in range(K):
        for s in range(S):
            for c in range(planes):
                out[k] += float((1.0 - finn_ref.ssim_map(t[s, c], p[s, k, c])).sum())
    return torch.from_numpy(out)


def mean_ssim(pred, target):
    """(K,) fp64: 1 - sums / m, the mean Finn SSIM of each call."""
    S, K, planes, H, W = pred.shape
    return 1.0 - sums(pred, target) / float(S * planes * (H - WIN + 1) * (W - WIN + 1))


def formula(pred, target, weights, defect=None):
    """(sums (K,), gradient like pred) in fp64 by the closed form.  defect: None or one of DEFECTS."""
    assert defect is None or defect in DEFECTS, defect
    x, y = target.double()[:, None], pred.double()
    mx, my, exx, eyy, exy = valid(x), valid(y), valid(x * x), valid(y * y), valid(x * y)
    A1, A2 = 2 * mx * my + C1, 2 * (exy - mx * my) + C2
    B1, B2 = mx * mx + my * my + C1, (exx - mx * mx) + (eyy - my * my) + C2
    S = A1 * A2 / (B1 * B2)
    c = (2 * A1 / (B1 * B2)).expand_as(S)
    b = -S / B2
    a = 2 * mx * (A2 - A1) / (B1 * B2) - 2 * my * S / B1 + 2 * my * S / B2
    if defect == "a_without_its_B2_term":
        a = 2 * mx * (A2 - A1) / (B1 * B2) - 2 * my * S / B1
    if defect == "b_with_the_wrong_sign":
        b = -b
    shift = 1 if defect == "back_filter_shifted_by_one" else 0
    two = 1.0 if defect == "factor_2_on_P_full_b_dropped" else 2.0
    dS = full(a, shift) + two * y * full(b, shift) + x * full(c.contiguous(), shift)
    w = torch.as_tensor(weights, dtype=torch.float64).view(1, -1, 1, 1, 1)
    return (1.0 - S).sum((0, 2, 3, 4)), -w * dS


def gradient(pred, target, weights):
    """d(sum_k weights[k] sums[k]) / d pred, fp64."""
    return formula(pred, target, weights)[1]


def autograd(pred, target, weights):
    """(sums, gradient) in fp64 by autograd of dvg_amd.frame_loss.torch_ssim_sum, the slice composition."""
    from dvg_amd import frame_loss
    p = pred.double().clone().requires_grad_(True)
    t = target.double()
    terms = [frame_loss.torch_ssim_sum(p[:, k], t) for k in range(pred.shape[1])]
    sum(w * v for w, v in zip(weights, terms)).backward()
    return torch.stack([v.detach() for v in terms]), p.grad


def central_difference_gap(pred, target, weights, h=1e-5):
    """max |formula - (f(P + h e) - f(P - h e)) / 2h| over every element e, relative to the largest gradient entry; f in fp64."""
    w = torch.as_tensor(weights, dtype=torch.float64)

    def f(p):
        return float((formula(p, target, weights)[0] * w).sum())
    g = gradient(pred, target, weights)
    p = pred.double().clone()
    flat, worst = p.view(-1), 0.0
    for i in range(flat.numel()):
        keep = float(flat[i])
        flat[i] = keep + h
        up = f(p)
        flat[i] = keep - h
        down = f(p)
        flat[i] = keep
        worst = max(worst, abs((up - down) / (2 * h) - float(g.view(-1)[i])))
    return worst / float(g.abs().max())


# ---- seeded inputs: (pred (S, K, planes, H, W), target (S, planes, H, W)), fp32 -------------------------------------------------------
def _noise(rs, S, K, planes, H, W):
    """Uniform target plus 0.05 normal (finn_ref._noise), a fresh draw per call."""
    t = rs.uniform(0.0, 1.0, size=(S, planes, H, W)).astype(np.float32)
    p = (t[:, None] + rs.normal(0.0, 0.05, size=(S, K, planes, H, W))).astype(np.float32)
    return p, t


def _sparse(rs, S, K, planes, H, W):
    """Mostly zero frames with one textured block, against a copy shifted by (2, 3) and scaled by 0.8 (finn_ref._sparse); call k is
    scaled by 0.8 - 0.1 k.  Most windows are flat: sigma^2 ~ 0 against C2 = 9e-4."""
    t, p = np.zeros((S, planes, H, W), np.float32), np.zeros((S, K, planes, H, W), np.float32)
    bh, bw = max(4, H // 3), max(4, W // 3)
    for s in range(S):
        for c in range(planes):
            y0, x0 = rs.randint(0, H - bh - 2), rs.randint(0, W - bw - 3)
            blk = rs.uniform(0.2, 1.0, size=(bh, bw)).astype(np.float32)
            t[s, c, y0:y0 + bh, x0:x0 + bw] = blk
            for k in range(K):
                p[s, k, c, y0 + 2:y0 + 2 + bh, x0 + 3:x0 + 3 + bw] = np.float32(0.8 - 0.1 * k) * blk
    return p, t


def _const(rs, S, K, planes, H, W):
    return np.full((S, K, planes, H, W), 0.75, np.float32), np.full((S, planes, H, W), 0.25, np.float32)


def _identical(rs, S, K, planes, H, W):
    t = rs.uniform(0.0, 1.0, size=(S, planes, H, W)).astype(np.float32)
    return np.repeat(t[:, None], K, 1).copy(), t


_BUILDERS = {"noise": _noise, "sparse": _sparse, "const": _const, "identical": _identical}


def case(kind, seed, S, K, planes, H, W):
    """(pred, target) fp32 torch tensors of one of KINDS."""
    p, t = _BUILDERS[kind](np.random.RandomState(7300 + seed), S, K, planes, H, W)
    return torch.from_numpy(p), torch.from_numpy(t)
