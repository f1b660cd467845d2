"""CPU: the identity behind the live-only form of the upsampled F(4x4,3x3) layers (docs/DESIGN_NOTES_upconv_live.md), the compact
index, and the tile the 25-position batched GEMM is pinned to (host-only plan calls: no GPU is touched)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import upconv_live_ref as ulr


@pytest.mark.parametrize("n,h,c", [(2, 4, 8), (1, 8, 4)])
def test_the_eleven_positions_are_exactly_zero_in_fp32_and_no_other_is(n, h, c):
    """bt4 restated in float32 over upsampled maps of mixed magnitudes (1e-3 ... 1e3, both signs): every tile's positions with
    a == 2 or b == 2 are exactly zero - border tiles (4^2 -> 8^2: all of them) and interior ones (8^2 -> 16^2) alike - and
    every other position is non-zero somewhere."""
    x = ulr.mixed((n, h, h, c), 8600 + h).numpy()
    v = ulr.input_transform_up_f32(x)
    dead = ulr.dead_positions()
    assert len(dead) == 11
    assert not v[dead].any()
    for p in range(36):
        if p not in dead:
            assert v[p].any(), p


def test_compact_index_is_a_bijection_onto_25_in_the_order_of_the_wrapper():
    from dvg_amd import ops
    pairs = ulr.live_pairs()
    ix = [ulr.compact_axis(a) * 5 + ulr.compact_axis(b) for a, b in pairs]
    assert ix == list(range(25))
    assert list(ops.LIVE_POSITIONS) == [a * 6 + b for a, b in pairs]
    assert sorted(set(range(36)) - set(ops.LIVE_POSITIONS)) == ulr.dead_positions()
    d = torch.arange(36.0).view(36, 1)
    assert torch.equal(ulr.live_slices(d).view(-1), torch.tensor(ops.LIVE_POSITIONS, dtype=torch.float32))
    assert torch.equal(ulr.live_slices(ulr.zero_filled(ulr.live_slices(d))), ulr.live_slices(d))


def test_the_planted_index_is_caught_by_the_host_restatement():
    """a - (a > 1) equals a - (a > 2) on the live rows, so the planted defect is the one that index belongs to: row / column 1
    dropped instead of row / column 2 (upconv_live_ref.PLANTED)."""
    assert [a - (a > 1) for a in range(6) if a != 2] == [ulr.compact_axis(a) for a in range(6) if a != 2]
    d = torch.arange(1.0, 37.0).view(36, 1)
    assert not torch.equal(ulr.live_slices(d, ulr.PLANTED), ulr.live_slices(d))
    assert not torch.equal(ulr.zero_filled(ulr.live_slices(d), ulr.PLANTED), ulr.zero_filled(ulr.live_slices(d)))


def _plan(lib, fn, *shape):
    tw, nt, ni = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = fn(*shape, ctypes.byref(tw), ctypes.byref(nt), ctypes.byref(ni))
    return rc, (tw.value, nt.value, ni.value)


@pytest.mark.parametrize("energy", [0, 1])
@pytest.mark.parametrize("shape", [(16, 16, 512, 512), (64, 16, 256, 256)])
def test_the_25_position_gemm_is_planned_on_the_tile_of_the_36(shape, energy):
    """(NB 25 as 36): (tile_w, nt) of the plan equal those of the NB = 36 plan under both tile policies; the images per pipeline
    follow the launcher's rule on the real count."""
    from dvg_amd import _lib
    lib = _lib.lib()
    prev = lib.dvg_tile_policy()
    lib.dvg_set_tile_policy(energy)
    try:
        rc36, p36 = _plan(lib, lib.dvg_gemm_batched_plan, 36, *shape)
        rc25, p25 = _plan(lib, lib.dvg_gemm_batched_plan, 25, *shape)
        rca, pa = _plan(lib, lib.dvg_gemm_batched_plan_as, 25, 36, *shape)
        rcs, ps = _plan(lib, lib.dvg_gemm_batched_plan_as, 36, 36, *shape)
    finally:
        lib.dvg_set_tile_policy(prev)
    assert rc36 == rc25 == rca == rcs == 0
    assert pa[:2] == p36[:2], (pa, p36)
    assert ps == p36
    if pa[:2] == p25[:2]:
        assert pa[2] == p25[2]                   # same tile: the launcher's own rule on 25 images
    if energy and shape == (16, 16, 512, 512) and lib.dvg_mfma_mode() == 1:
        # the case the pinning exists for: 36 * 2 * 4 = 288 >= 256 workgroups of the 128 x 128 tile, 25 * 2 * 4 = 200 are not
        assert p36[:2] == (16, 2) and p25[:2] != (16, 2), (p36, p25)


def test_the_plan_refuses_a_nominal_count_below_the_real_one():
    from dvg_amd import _lib
    lib = _lib.lib()
    assert _plan(lib, lib.dvg_gemm_batched_plan_as, 36, 25, 16, 16, 512, 512)[0] == -1
    assert _plan(lib, lib.dvg_gemm_batched_plan_as, 0, 36, 16, 16, 512, 512)[0] == -1
    assert lib.dvg_gemm_batched_plan_as(25, 36, 16, 16, 512, 512, None, None, None) == -1


def test_wrapper_refuses_inconsistent_live_arguments():
    """A WinoV is live only through the upsampling; the argument checks of conv3x3_winograd come before any launch."""
    from dvg_amd import ops
    with pytest.raises(RuntimeError):
        ops.WinoV(torch.zeros(25, 4, 4), (1, 4, 8, 8), up=False, live=True)
    assert ops.WinoV(torch.zeros(25, 4, 4), (1, 4, 8, 8), up=True, live=True).live
    assert np.prod(ops.WinoV(torch.zeros(36, 4, 4), (1, 4, 8, 8)).v.shape) == 36 * 16
