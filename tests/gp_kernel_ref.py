"""The GP trigger's arithmetic restated in torch, by covariance family: predict (train and eval), the first-call prior
initialisation and the ELBO, in fp64 or fp32.  Written from the equations of docs/DESIGN_NOTES_gp_kernels.md and DESIGN.md's GP
section; it shares no code with oracle/ or with dvg_amd, so the GP kernels' Matern members have a reference of their own (the
oracle states the RBF only; tests/test_gp_kernels_host.py holds this file to it there)."""
import math

import torch
import torch.nn.functional as F

KERNELS = ("rbf", "matern12", "matern32", "matern52")
JITTER = 1e-3
NOISE_FLOOR = 1e-4


def k_of_d(kernel, d, s, ell):
    """k(d), d = z - x signed; s, ell broadcastable against d."""
    r = d.abs() / ell
    if kernel == "rbf":
        return s * torch.exp(-0.5 * d * d / ell ** 2)      # r^2 / 2 with one rounding less: K_ZZ^-1 amplifies each by cond ~ 1e4
    if kernel == "matern12":
        return s * torch.exp(-r)
    if kernel == "matern32":
        a = math.sqrt(3.0) * r
        return s * (1.0 + a) * torch.exp(-a)
    if kernel == "matern52":
        a = math.sqrt(5.0) * r
        return s * (1.0 + a + a * a / 3.0) * torch.exp(-a)
    raise ValueError(kernel)


def rho_of_d(kernel, d, ell):
    """rho(d) = (dk/dd) / k, the table of the design note (sign(0) = 0)."""
    a = math.sqrt({"rbf": 0.0, "matern12": 0.0, "matern32": 3.0, "matern52": 5.0}[kernel]) * d.abs() / ell
    if kernel == "rbf":
        return -d / ell ** 2
    if kernel == "matern12":
        return -torch.sign(d) / ell
    if kernel == "matern32":
        return -3.0 * d / (ell ** 2 * (1.0 + a))
    return -(5.0 * d / (3.0 * ell ** 2)) * (1.0 + a) / (1.0 + a + a * a / 3.0)


def gram(kernel, a, b, s, ell):
    """a (D,Na), b (D,Nb), s, ell (D,) -> (D,Na,Nb)."""
    return k_of_d(kernel, a.unsqueeze(-1) - b.unsqueeze(-2), s.view(-1, 1, 1), ell.view(-1, 1, 1))


def hypers(sd):
    s = F.softplus(sd["covar_module.raw_outputscale"]).reshape(-1)
    ell = F.softplus(sd["covar_module.base_kernel.raw_lengthscale"]).reshape(-1)
    return s, ell, sd["mean_module.constant"].reshape(-1)


def noise_of(lik):
    return F.softplus(lik["noise_covar.raw_noise"]).reshape(-1) + NOISE_FLOOR


def _parts(kernel, h, sd, dtype):
    s, ell, c = [t.to(dtype) for t in hypers(sd)]
    z = sd["variational_strategy.inducing_points"].squeeze(-1).to(dtype)
    m = sd["variational_strategy.variational_distribution.variational_mean"].to(dtype)
    ls = torch.tril(sd["variational_strategy.variational_distribution.chol_variational_covar"].to(dtype))
    x = h.to(dtype).t().contiguous()
    M = z.shape[1]
    kzz = gram(kernel, z, z, s, ell) + JITTER * torch.eye(M, dtype=dtype)
    L = torch.linalg.cholesky(kzz)
    kzx = gram(kernel, z, x, s, ell)
    A = torch.linalg.solve_triangular(L, kzx, upper=False)
    v = torch.linalg.solve_triangular(L, (m - c.view(-1, 1)).unsqueeze(-1), upper=False)
    return s, ell, c, z, x, ls, kzz, L, kzx, A, v


def predict(kernel, h, sd, training, noise=None, dtype=torch.float64):
    """h (B,D) -> mean (D,B), var (D,B) and kl (D) [train] or cov (D,B,B) [eval]; `noise` (D,) is added to var / cov."""
    s, ell, c, z, x, ls, kzz, L, kzx, A, v = _parts(kernel, h, sd, dtype)
    D, M = z.shape
    W = ls.transpose(1, 2) @ kzx
    out = {"mean": c.view(-1, 1) + (A.transpose(1, 2) @ v).squeeze(-1)}
    nz = torch.zeros(D, dtype=dtype) if noise is None else noise.to(dtype).reshape(-1)
    if training:
        gap = s.view(-1, 1) - (A * A).sum(1)
        out["gap"] = gap                                       # s - q: the train-mode clamp acts where this is <= 0
        out["var"] = (W * W).sum(1) + torch.clamp(gap, min=0.0) + nz.view(-1, 1)
        logdet_k = 2.0 * torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1)
        logdet_s = 2.0 * torch.log(torch.diagonal(ls, dim1=1, dim2=2).abs()).sum(1)
        trace = ((ls @ ls.transpose(1, 2)) * kzz).sum((1, 2))
        out["kl"] = 0.5 * (-logdet_k - logdet_s + trace + (v.squeeze(-1) ** 2).sum(1) - M)
    else:
        cov = W.transpose(1, 2) @ W + gram(kernel, x, x, s, ell) - A.transpose(1, 2) @ A
        out["cov"] = cov + nz.view(-1, 1, 1) * torch.eye(x.shape[1], dtype=dtype)
        out["var"] = torch.diagonal(out["cov"], dim1=1, dim2=2)
    return out


def rsample(mean, cov, eps):
    return mean + (torch.linalg.cholesky(cov) @ eps.to(cov.dtype).unsqueeze(-1)).squeeze(-1)


def prior_init(kernel, sd, jitter_terms=1):
    """(variational mean, chol_variational_covar) of the first train-mode call: m <- c, L_S <- chol((K_ZZ + jitter I)^-1), fp64."""
    s, ell, c = [t.double() for t in hypers(sd)]
    z = sd["variational_strategy.inducing_points"].squeeze(-1).double()
    M = z.shape[1]
    kzz = gram(kernel, z, z, s, ell) + jitter_terms * JITTER * torch.eye(M, dtype=torch.float64)
    return c.view(-1, 1).expand(-1, M).clone(), torch.linalg.cholesky(torch.linalg.inv(kzz))


def elbo(pred, target, noise, num_data):
    """(D,): (1/B) sum_b E_q[log N(y_b | f_b, sigma^2)] - KL / num_data from a train-mode prediction WITHOUT noise."""
    mean, var = pred["mean"], pred["var"]
    nz = noise.to(mean.dtype).view(-1, 1)
    ll = -0.5 * ((target.to(mean.dtype) - mean) ** 2 + var) / nz - 0.5 * torch.log(nz) - 0.5 * math.log(2 * math.pi)
    return ll.sum(-1) / mean.shape[-1] - pred["kl"] / num_data


def min_gap_to_inducing(h, sd):
    """min |z - x| over every latent dim: the Matern kernels have a kink at 0."""
    z = sd["variational_strategy.inducing_points"].squeeze(-1).double()
    return float((z.unsqueeze(-1) - h.double().t().unsqueeze(-2)).abs().min())
