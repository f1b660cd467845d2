"""Not a test: the semantics of dvg_clip_gather_aug_u8 in numpy, shared by tests/test_augment_host.py and
tests/test_gpu_augment.py.  Every step is an index permutation or ONE IEEE float32 operation, so the kernel is held to it bit
for bit."""
import numpy as np
import torch

MAX_SHIFT = 16


def reference_aug_batch(pool, first, geom, photo, T, C):
    """pool (n,H,W,pool_c) uint8, first (B,), geom (B,4) [hflip, reverse, dy, dx], photo (B,2) float32 [gain, bias] ->
    (T,B,C,H,W) float32 torch tensor, normalize_data's layout.  Wild values are read as the kernel reads them: first clamped to
    [0, n - T], dy / dx to +-16, hflip / reverse as != 0."""
    pool = np.asarray(pool)
    n, H, W, _ = pool.shape
    first, geom = np.asarray(first, np.int64), np.asarray(geom, np.int64)
    photo = np.asarray(photo, np.float32)
    B = len(first)
    out = np.empty((T, B, C, H, W), np.float32)
    y, x = np.arange(H), np.arange(W)
    for b in range(B):
        f = int(np.clip(first[b], 0, n - T))
        hflip, reverse = geom[b, 0] != 0, geom[b, 1] != 0
        dy, dx = (int(np.clip(v, -MAX_SHIFT, MAX_SHIFT)) for v in geom[b, 2:])
        ts = np.arange(T)[::-1] if reverse else np.arange(T)
        sy = np.clip(y + dy, 0, H - 1)
        sx = np.clip((W - 1 - x if hflip else x) + dx, 0, W - 1)
        src = pool[f + ts][:, sy][:, :, sx][..., :C]                            # (T,H,W,C) bytes
        v = (src.astype(np.float64) / 255.).astype(np.float32)
        m = v * photo[b, 0]                                                     # float32 multiply ...
        a = m + photo[b, 1]                                                     # ... then float32 add
        assert m.dtype == np.float32 and a.dtype == np.float32
        out[:, b] = np.clip(a, np.float32(0), np.float32(1)).transpose(0, 3, 1, 2)
    return torch.from_numpy(out)
