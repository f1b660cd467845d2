"""GPU: the 128 x 128 batched-GEMM tile (ENERGY tile policy, bf16-triple build) loads its weight fragments from global memory
into the registers the MFMAs read, not through LDS (conv_igemm2.hip: Cfg2::WREG, docs/DESIGN_NOTES_gemm_wreg.md).  dvg_gemm_batched_k16
and dvg_gemm_batched_k16_as through the C ABI at the smallest shapes that take that tile - 288 ... 300 workgroups, just over the
256 of DVG_GEMM_NT2 - and reach each edge of its pipeline:

    dense, 36 positions   T = 1024  Cin =  64  Cout = 128   two K = 32 stages: the prologue's slab, one looping stage, the last
                          T = 1024  Cin = 128  Cout = 128   four stages: the looping stage repeats
                          T = 1024  Cin = 192  Cout = 128   six stages: five looping stages and the last
                          T =  512  Cin =  64  Cout = 256   two column blocks per position
    live, 25 as 36        T = 1536  Cin =  64  Cout = 128   dvg_gemm_batched_k16_as

(The launcher takes Cin % 64 == 0 only - gemm_plan - so Cin = 64 is the shortest pipeline there is.)  Each result: against the
fp64 product of the same fp32 operands under the bar tests/test_gpu_winograd_stages.py holds the batched GEMM to
(winograd_ref.ratio_bar of the case's own figures and winograd_ref.gemm_worst), against the LATENCY-policy result of the same
call at the 5e-6 max-norm the project uses across tile policies, and twice for equal bits."""
import ctypes
import functools

import pytest
import torch

from oracle import params
from tests import winograd_ref as wr
from tests.common import dev, rel_err

pytestmark = pytest.mark.gpu

_ops, _lib, _call, _nan = wr.gpu_ops, wr.gpu_lib, wr.gpu_call, wr.nan_filled

# name -> (NB, NB_as, T, Cin, Cout): NB positions of T tiles on the tile of an NB_as-position launch
CASES = {"k64": (36, 36, 1024, 64, 128), "k128": (36, 36, 1024, 128, 128), "k192": (36, 36, 1024, 192, 128),
         "o256": (36, 36, 512, 64, 256), "live": (25, 36, 1536, 64, 128)}
POLICY_TOL = 5e-6          # tests.common.rel_err between the tile policies (tests/test_gpu_headline.py, test_gpu_modules.py)


def _skip_unless_x3():
    if _lib().dvg_mfma_mode() != 1:
        pytest.skip("the 128 x 128 tile exists in the bf16-triple build only")


@functools.lru_cache(maxsize=None)
def _inputs(name):
    nb, _, t, cin, cout = CASES[name]
    k = list(CASES).index(name)
    return params.normal(9950 + 10 * k, nb, t // 16, 16, cin), params.normal(9951 + 10 * k, nb, cin, cout, scale=cin ** -0.5)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(fp64 product, bar): the figures of winograd_ref.gemm_figures for this case's operands at the (16, 2, 1) plan."""
    x, u = _inputs(name)
    plan = (16, 2, 1)
    ref = wr.gemm_ref(x, u)
    e_plane = min(wr.gemm_err(wr.gemm_plant(kind, x, u, plan), ref, plan) for kind in ("plane_x", "plane_u"))
    nb, h, w, cin = x.shape
    tiles = wr.emu_tiles(h, w, 16)
    pick = lambda t: torch.stack([t[:, 8 * ty:8 * ty + 8, 16 * tx:16 * tx + 16] for ty, tx in tiles], 1)      # noqa: E731
    emu = wr.gemm_ordered(pick(x).reshape(nb, -1, cin), u, wr.plane_pairs(plan)).reshape(nb, len(tiles) * 8, 16, -1)
    e_y = wr.gemm_err(emu, pick(ref).reshape(emu.shape), plan)
    return ref, wr.ratio_bar(e_y, wr.gemm_worst(True), e_plane, True), e_y, e_plane


def _launch(name, energy):
    """The case's launch under the policy: (y, (tile_w, nt, ni))."""
    nb, nb_as, t, cin, cout = CASES[name]
    lib = _lib()
    x, u = _inputs(name)
    xd, wd = x.to(dev()), wr.pack_rows(u, int(lib.dvg_packed_row_floats())).to(dev())
    y = _nan(nb, t // 16, 16, cout)
    tw, nt, ni = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    with _ops().tile_policy(energy):
        assert lib.dvg_gemm_batched_plan_as(nb, nb_as, t // 16, 16, cin, cout, ctypes.byref(tw), ctypes.byref(nt), ctypes.byref(ni)) == 0
        if nb == nb_as:
            _call(lib.dvg_gemm_batched_k16, xd, wd, y, nb, t // 16, 16, cin, cout)
        else:
            _call(lib.dvg_gemm_batched_k16_as, xd, wd, y, nb, nb_as, t // 16, 16, cin, cout)
    return y, (tw.value, nt.value, ni.value)


@pytest.mark.parametrize("name", list(CASES))
def test_the_cases_sit_just_over_the_tile_threshold(name):
    nb, nb_as, t, cin, cout = CASES[name]
    assert 288 <= nb * (t // 128) * (cout // 128) <= 300 and nb_as * (t // 128) * (cout // 128) >= 256


@pytest.mark.parametrize("name", list(CASES))
def test_energy_tile_against_fp64_and_against_the_latency_tile(name):
    _skip_unless_x3()
    ref, bar, e_y, e_plane = _reference(name)
    y, plan = _launch(name, True)
    assert plan == (16, 2, 1), plan
    e_hip = wr.gemm_err(y.cpu(), ref, plan)
    y_lat, plan_lat = _launch(name, False)
    assert plan_lat[1] == 1, plan_lat
    d = rel_err(y, y_lat)
    print(f"{name} {CASES[name]}: e_hip {e_hip:.2e} e_y {e_y:.2e} e_plane {e_plane:.2e} bar {bar:.2e}; "
          f"energy against latency, max-norm {d:.2e}")
    assert e_hip <= bar, (name, e_hip, bar)
    assert d < POLICY_TOL, (name, d)


@pytest.mark.parametrize("name", ["k128", "live"])
def test_energy_tile_gives_equal_bits_twice(name):
    _skip_unless_x3()
    a, _ = _launch(name, True)
    b, _ = _launch(name, True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
