"""The fp64 reference of the frame losses behind train.py --frame_loss / --gdl_weight, written from the formulas of
docs/DESIGN_NOTES_frame_loss.md and independent of dvg_amd.frame_loss (which the tests compare against it).

For one decoder call k, P and T of shape (planes, H, W), d = P - T:

    pix = sum rho(d)     rho = d^2 (mse) | |d| (l1) | sqrt(d^2 + eps^2) (charbonnier)
    gdl = sum_{x >= 1} | |P[y, x] - P[y, x-1]| - |T[y, x] - T[y, x-1]| | + sum_{y >= 1} | |P[y, x] - P[y-1, x]| - |T[y, x] - T[y-1, x]| |

`sums` gives both per call over steps, planes and pixels; `objective` is sum_k w_k (pix_k + G gdl_k) and `gradient` its
derivative by torch autograd in fp64 (abs has derivative sign, sign(0) = 0).  `central_difference_gap` checks that autograd
gradient against central differences for the smooth kind, so that the reference is not taken on faith."""
import torch

KINDS = ("mse", "l1", "charbonnier")


def rho(d, kind, eps):
    if kind == "mse":
        return d ** 2
    if kind == "l1":
        return torch.abs(d)
    if kind == "charbonnier":
        return torch.sqrt(d ** 2 + eps ** 2)
    raise ValueError(kind)


def sums(pred, target, kind, eps=1e-3):
    """pred (S, K, planes, H, W), target (S, planes, H, W) -> (pix (K,), gdl (K,)) in fp64."""
    P, T = pred.double(), target.double().unsqueeze(1)
    over = (0, 2, 3, 4)
    pix = rho(P - T, kind, eps).sum(over)
    ex = torch.abs(torch.abs(P[..., :, 1:] - P[..., :, :-1]) - torch.abs(T[..., :, 1:] - T[..., :, :-1]))
    ey = torch.abs(torch.abs(P[..., 1:, :] - P[..., :-1, :]) - torch.abs(T[..., 1:, :] - T[..., :-1, :]))
    return pix, ex.sum(over) + ey.sum(over)


def objective(pred, target, kind, weights, gdl, eps=1e-3):
    pix, edge = sums(pred, target, kind, eps)
    w = torch.tensor([float(v) for v in weights], dtype=torch.float64)
    return (w * (pix + float(gdl) * edge)).sum()


def gradient(pred, target, kind, weights, gdl, eps=1e-3):
    """d objective / d pred in fp64, shaped like pred."""
    p = pred.detach().double().clone().requires_grad_(True)
    objective(p, target, kind, weights, gdl, eps).backward()
    return p.grad


def central_difference_gap(pred, target, weights, gdl=0.0, eps=1e-3, h=1e-6, probes=24, seed=0):
    """max over `probes` random elements of |autograd - central difference| / max |autograd| for the charbonnier pixel term (smooth
    everywhere; gdl = 0 keeps the objective smooth)."""
    g = gradient(pred, target, "charbonnier", weights, gdl, eps)
    flat = pred.detach().double().reshape(-1)
    idx = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(seed))[:probes]
    worst = 0.0
    for i in idx.tolist():
        up, dn = flat.clone(), flat.clone()
        up[i] += h
        dn[i] -= h
        fd = (objective(up.view_as(pred), target, "charbonnier", weights, gdl, eps) -
              objective(dn.view_as(pred), target, "charbonnier", weights, gdl, eps)) / (2 * h)
        worst = max(worst, abs(float(fd) - float(g.reshape(-1)[i])))
    return worst / float(g.abs().max())


# ---- the tests' inputs ------------------------------------------------------------------------------------------------------------
def quantised_case(seed, S, K, planes, H, W):
    """(pred, target) in fp32 with every value a multiple of 1/256 in [0, 1) - what uint8 frames hold - and about half the pixels
    blanked to 0 in pred AND target: every difference is exact in fp32 (so every sign is the fp64 reference's) and ties - both
    differences of an edge equal in magnitude - occur in quantity."""
    g = torch.Generator().manual_seed(seed)
    target = torch.randint(0, 256, (S, planes, H, W), generator=g).float() / 256.0
    pred = torch.randint(0, 256, (S, K, planes, H, W), generator=g).float() / 256.0
    keep = (torch.rand((S, planes, H, W), generator=g) < 0.5).float()
    return (pred * keep.unsqueeze(1)).contiguous(), (target * keep).contiguous()


def noisy_case(seed, S, K, planes, H, W):
    """(pred, target) in fp32, unquantised: target uniform in [0, 1), pred = target + 0.1 normal."""
    g = torch.Generator().manual_seed(seed)
    target = torch.rand((S, planes, H, W), generator=g)
    pred = target.unsqueeze(1) + 0.1 * torch.randn((S, K, planes, H, W), generator=g)
    return pred.contiguous(), target.contiguous()


def tied_fraction(pred, target):
    """The share of edges whose two differences are equal in magnitude (gradient exactly 0), over all calls."""
    P, T = pred.double(), target.double().unsqueeze(1)
    ex = torch.abs(P[..., :, 1:] - P[..., :, :-1]) - torch.abs(T[..., :, 1:] - T[..., :, :-1])
    ey = torch.abs(P[..., 1:, :] - P[..., :-1, :]) - torch.abs(T[..., 1:, :] - T[..., :-1, :])
    n = ex.numel() + ey.numel()
    return (float((ex == 0).sum()) + float((ey == 0).sum())) / max(n, 1)
