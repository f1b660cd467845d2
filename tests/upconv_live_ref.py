"""Host restatement of the live-only form of an upsampled F(4x4,3x3) layer (docs/DESIGN_NOTES_upconv_live.md): which of the
36 transform positions are dead, where a live one sits in the compact (25, T, C) tensors, the fp32 input transform the way
winograd.hip's bt4 writes it, and the inputs the tests share.  Nothing in here touches a GPU."""
import numpy as np
import torch

DEAD = 2            # row / column of B^T that cancels on a repeated low-res row: [0 4 -4 -1 1 0]


PLANTED = 1         # the planted defect: the compact index taken as a - (a > 1).  On the live rows {0, 1, 3, 4, 5} that is the same
#                     number as a - (a > 2), so the index alone plants nothing; the defect it stands for is the one in which that
#                     index is right - row / column 1 taken for the dead one - and that is what the tests plant.


def compact_axis(a, dead=DEAD):
    """a' of a live row / column a (a != dead): the rows above the dead one move down by one."""
    return a - (a > dead)


def live_pairs(dead=DEAD):
    return [(a, b) for a in range(6) if a != dead for b in range(6) if b != dead]


def dead_positions(dead=DEAD):
    return [a * 6 + b for a in range(6) for b in range(6) if a == dead or b == dead]


def live_slices(dense, dead=DEAD):
    """The compact (25, ...) tensor of a dense (36, ...) one: position (a, b) goes to a' * 5 + b'."""
    out = torch.zeros((25,) + tuple(dense.shape[1:]), dtype=dense.dtype, device=dense.device)
    for a, b in live_pairs(dead):
        out[compact_axis(a, dead) * 5 + compact_axis(b, dead)] = dense[a * 6 + b]
    return out


def zero_filled(compact, dead=DEAD):
    """The dense (36, ...) tensor of a compact one: +0 at the 11 dead positions."""
    out = torch.zeros((36,) + tuple(compact.shape[1:]), dtype=compact.dtype, device=compact.device)
    for a, b in live_pairs(dead):
        out[a * 6 + b] = compact[compact_axis(a, dead) * 5 + compact_axis(b, dead)]
    return out


def mixed(shape, seed, device="cpu"):
    """Random values of both signs with magnitudes 1e-3 ... 1e3 (log-uniform), made on `device`."""
    g = torch.Generator(device=device).manual_seed(seed)
    mag = torch.pow(10.0, torch.rand(shape, generator=g, device=device) * 6.0 - 3.0)
    sign = (torch.rand(shape, generator=g, device=device) < 0.5).float() * 2.0 - 1.0
    return (mag * sign).float()


def bt4_f32(d):
    """winograd.hip's bt4 on axis 0 of a float32 array (6, ...): the same expressions, every operation rounded to fp32."""
    f = np.float32
    e = np.empty_like(d)
    e[0] = f(4) * d[0] - f(5) * d[2] + d[4]
    e[1] = f(-4) * (d[1] + d[2]) + d[3] + d[4]
    e[2] = f(4) * (d[1] - d[2]) - d[3] + d[4]
    e[3] = f(2) * (d[3] - d[1]) - d[2] + d[4]
    e[4] = f(2) * (d[1] - d[3]) - d[2] + d[4]
    e[5] = f(4) * d[1] - f(5) * d[3] + d[5]
    return e


def input_transform_up_f32(x):
    """V (36, tiles, C) float32 of nearest-x2-upsampled x (N, h, w, C) float32, zero padding 1, tile by tile as
    winograd4_input_kernel(up = 1) takes it: columns first, then rows."""
    n, h, w, c = x.shape
    up = np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)
    pad = np.zeros((n, 2 * h + 2, 2 * w + 2, c), np.float32)
    pad[:, 1:-1, 1:-1] = up
    ht, wt = 2 * h // 4, 2 * w // 4
    v = np.empty((36, n * ht * wt, c), np.float32)
    for i in range(n):
        for ty in range(ht):
            for tx in range(wt):
                d = pad[i, 4 * ty:4 * ty + 6, 4 * tx:4 * tx + 6]          # [a][b][c]
                e = bt4_f32(d)                                            # rows a transformed, per column b
                o = bt4_f32(np.ascontiguousarray(e.transpose(1, 0, 2)))   # [b'][a'][c]
                v[:, (i * ht + ty) * wt + tx] = o.transpose(1, 0, 2).reshape(36, c)
    return v
