"""The four update rules of dvg_optim_step restated in numpy fp64 from the formulas of the torch.optim documentation (Adam,
AdamW, SGD, RMSprop: default, non-amsgrad, non-centered, no dampening), with what the kernel adds to them: the decay mask per
16-byte piece, the gradient guard's factor and the schedule's rate multiplier.  A plain module (`from tests import optim_ref`)."""
import numpy as np

ADAM, ADAMW, SGD, RMSPROP = 0, 1, 2, 3
NAMES = {ADAM: "adam", ADAMW: "adamw", SGD: "sgd", RMSPROP: "rmsprop"}


def piece_decay(n, weight_decay, mask):
    """The weight decay of every element: `weight_decay` where the element's piece (4 floats) has a non-zero mask byte (mask
    None: everywhere), else 0."""
    wd = np.full(n, float(weight_decay), dtype=np.float64)
    if mask is not None:
        mask = np.asarray(mask)
        assert mask.shape == ((n + 3) // 4,)
        wd[np.repeat(mask, 4)[:n] == 0] = 0.0
    return wd


def step(rule, p, g, m, v, t, lr, a, b, eps=1e-8, weight_decay=0.0, nesterov=False, mask=None, grad_scale=1.0, lr_scale=1.0):
    """One step; p, g, m, v: fp64 arrays (m, v are updated copies; v may be None for SGD); t: the 1-based count of steps applied.
    Returns (p, m, v)."""
    p, g = np.array(p, dtype=np.float64), np.asarray(g, dtype=np.float64) * float(grad_scale)
    m = None if m is None else np.array(m, dtype=np.float64)
    v = None if v is None else np.array(v, dtype=np.float64)
    lr = float(lr) * float(lr_scale)
    wd = piece_decay(p.size, weight_decay, mask)
    if rule in (ADAM, ADAMW):
        if rule == ADAMW:
            p = p * (1.0 - lr * wd)
        else:
            g = g + wd * p
        m = a * m + (1.0 - a) * g
        v = b * v + (1.0 - b) * g * g
        bc1, bc2 = 1.0 - a ** t, 1.0 - b ** t
        p = p - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    elif rule == SGD:
        g = g + wd * p
        if a != 0:
            m = a * m + g                  # torch's first step sets the buffer to g: the same from a zero buffer
            g = g + a * m if nesterov else m
        p = p - lr * g
    elif rule == RMSPROP:
        g = g + wd * p
        v = a * v + (1.0 - a) * g * g
        avg = np.sqrt(v) + eps
        if b > 0:
            m = b * m + g / avg
            p = p - lr * m
        else:
            p = p - lr * g / avg
    else:
        raise ValueError(rule)
    return p, m, v


def run(rule, p0, grads, lr, a, b, eps=1e-8, weight_decay=0.0, nesterov=False, mask=None, grad_scale=1.0, lr_scale=1.0):
    """len(grads) steps from zero state; returns (p, m, v) in fp64."""
    p = np.array(p0, dtype=np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t, g in enumerate(grads, 1):
        p, m, v = step(rule, p, g, m, v, t, lr, a, b, eps, weight_decay, nesterov, mask, grad_scale, lr_scale)
    return p, m, v


# every rule / flag combination the GPU tests use: (name, rule, a, b, nesterov) and the weight decays
CASES = [("adam", ADAM, 0.9, 0.999, False), ("adamw", ADAMW, 0.9, 0.999, False),
         ("sgd", SGD, 0.0, 0.0, False), ("sgd_momentum", SGD, 0.9, 0.0, False), ("sgd_nesterov", SGD, 0.9, 0.0, True),
         ("rmsprop", RMSPROP, 0.99, 0.0, False), ("rmsprop_momentum", RMSPROP, 0.99, 0.9, False)]
DECAYS = (0.0, 0.01)


def torch_optimizer(rule, params, lr, a, b, eps=1e-8, weight_decay=0.0, nesterov=False):
    """The torch class `rule` restates, over `params` (parameters or parameter groups)."""
    import torch
    if rule == ADAM:
        return torch.optim.Adam(params, lr=lr, betas=(a, b), eps=eps, weight_decay=weight_decay)
    if rule == ADAMW:
        return torch.optim.AdamW(params, lr=lr, betas=(a, b), eps=eps, weight_decay=weight_decay)
    if rule == SGD:
        return torch.optim.SGD(params, lr=lr, momentum=a, weight_decay=weight_decay, nesterov=nesterov)
    return torch.optim.RMSprop(params, lr=lr, alpha=a, eps=eps, weight_decay=weight_decay, momentum=b)
