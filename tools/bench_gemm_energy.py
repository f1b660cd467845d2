"""The batched Winograd GEMM under the ENERGY tile policy (the 128 x 128 tile), one launch at a time per vgg_64 B = 64 layer
shape - 36 dense positions and the 25 live ones on the tile of the 36 (dvg_gemm_batched_k16_as) - back to back at steady
clocks (GPU only).  A/B workload for builds of the library:

    DVG_HIP_LIB=<path> python tools/bench_gemm_energy.py        two passes, one line each

(The rejected variants of docs/DESIGN_NOTES_gemm_wreg.md §3 were source edits in a copy of the tree, built with `make` there and
loaded through DVG_HIP_LIB: Cfg2::GT 2 -> 4 for the NT = 2 tile; the kernel's launch bound 2 -> 3.)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvg_amd import ops                      # noqa: E402
from dvg_amd._lib import lib                 # noqa: E402
from tools.bench_small import time_fn        # noqa: E402

# (positions, batch, map side, Cin, Cout)
SHAPES = [(36, 64, 32, 128, 128), (36, 64, 16, 256, 256), (36, 64, 8, 512, 512), (25, 64, 16, 512, 256), (25, 64, 32, 256, 128)]


def time_shape(nb, n, h, c, cout):
    dev = torch.device("cuda:0")
    t = n * (h // 4) ** 2
    v = torch.randn((nb, t, c), device=dev)
    m = torch.empty((nb, t, cout), device=dev)
    u = ops.winograd_weight(torch.randn(cout, c, 3, 3, device=dev) * 0.02, 4)[:nb].contiguous()
    us = time_fn(lambda: lib().dvg_gemm_batched_k16_as(ops._p(v), ops._p(u), ops._p(m), nb, 36, t // 16, 16, c, cout, ops._stream()),
                 iters=100)
    return f"{nb}x{h}^2 {c}->{cout}: {us:6.1f} us {2e-6 * nb * t * c * cout / us:5.1f} TF"


if __name__ == "__main__":
    name = os.path.basename(os.environ.get("DVG_HIP_LIB", "libdvg_hip.so"))
    with ops.tile_policy(True):
        for _ in range(2):
            print(name, " | ".join(time_shape(*s) for s in SHAPES))
