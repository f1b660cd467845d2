"""The Winograd-form weight gradient's own kernels (dvg_amd/csrc/wino_wgrad.hip) against fp64, stage by stage on synthetic
operands: the stream-K product dvg_winograd_wgrad_gemm / dvg_winograd_wgrad_gemm_items per (position, 64 x 64 block) under the
bar of docs/DESIGN_NOTES_winograd_tests.md - with every element of every slab written, at plans that hand over from block to
block inside a workgroup, cut blocks across workgroups, end in a short workgroup and cross from one V buffer into the next -
dvg_winograd_wgrad_reduce within its derived bound, and ops.winograd_wgrad_partial_multi end to end (padding, packing at
t_off, the slab reduction, the saved-V path) block by block against the direct form's fp64 gradient.  The operand transforms are in tests/test_gpu_winograd_stages.py;
tests/test_winograd_ref_host.py asserts the plans and that the bar rejects every planted defect."""
import ctypes

import pytest
import torch

from oracle import params
from tests import winograd_ref as wr
from tests.backward_ref import blockwise_err, sum_bound
from tests.common import dev

pytestmark = pytest.mark.gpu

_lib, _call, _nan, _report = wr.gpu_lib, wr.gpu_call, wr.nan_filled, wr.report


def _x3():
    return _lib().dvg_mfma_mode() == 1


def _slabs(name):
    """One launch of the case's product: the S slabs (S, 36, Cout, Cin) on the device, NaN-prefilled before the launch."""
    lib, c = _lib(), wr.WGEMM_BY_NAME[name]
    plan = wr.ww_plan(c["tp"], c["cin"], c["cout"])
    s = lib.dvg_winograd_wgrad_splits(c["tp"], c["cin"], c["cout"])
    assert s == plan["S"] == c["plan"][3], (name, s, plan["S"])
    dm, vs = wr.wgemm_inputs(name)
    dmd, vd = dm.to(dev()), [v.to(dev()) for v in vs]
    part = _nan(s, 36, c["cout"], c["cin"])
    if len(vd) == 1:
        _call(lib.dvg_winograd_wgrad_gemm, dmd, vd[0], part, c["tp"], c["cin"], c["cout"])
    else:
        ptrs = (ctypes.c_void_p * len(vd))(*[v.data_ptr() for v in vd])
        _call(lib.dvg_winograd_wgrad_gemm_items, dmd, ptrs, len(vd), c["t_item"], part, c["cin"], c["cout"])
    return part, plan


@pytest.mark.parametrize("name", wr.WGEMM_NAMES)
def test_wgrad_gemm_against_fp64_block_by_block(name):
    """The slabs summed in fp64 against P = sum_t dM V.  Every element of every slab is written (the prefill was NaN); the slabs
    beyond a block's last segment are exact zeros, and a block that is cut has data in as many slabs as it has segments."""
    c = wr.WGEMM_BY_NAME[name]
    part, plan = _slabs(name)
    assert bool(torch.isfinite(part).all()), "an element of a slab was not written"
    f, b = wr.wgemm_figures(name), wr.wgemm_bar(name, _x3())
    ref = wr.wgemm_ref(*wr.wgemm_inputs(name))
    e_hip = blockwise_err(part.double().sum(0).cpu(), ref)
    print(f"{name} plan {c['plan']}: e_hip {e_hip:.2e} e32 {f['e32']:.2e} e_plane {f['e_plane']:.2e} bar {b:.2e}")
    assert e_hip <= b, (name, e_hip, b)
    nbj, nbi = c["cin"] // 128, c["cout"] // 128
    used = (part.reshape(plan["S"], 36, nbi, 128, nbj, 128) != 0).any(5).any(3).cpu()          # (S, xi, bi, bj)
    for blk, segs in enumerate(plan["segs"]):
        bj, bi, xi = blk % nbj, (blk // nbj) % nbi, blk // (nbj * nbi)
        assert used[:, xi, bi, bj].tolist() == [k < segs for k in range(plan["S"])], (name, blk, segs)


def test_wgrad_gemm_slabs_reduce_as_the_wrapper_reduces_them():
    """S > 2: ops.winograd_wgrad_partial_multi sums the slabs with dvg_reduce_partials before the transform - the sum of the
    short-tail case's five slabs within sum_bound of their fp64 sum, and under the product's bar against fp64."""
    part, plan = _slabs("short-tail")
    s = plan["S"]
    assert s > 2
    summed = _nan(*part.shape[1:])
    _call(_lib().dvg_reduce_partials, part, summed, s, summed.numel())
    want = part.double().sum(0).cpu()
    bound = sum_bound(part.double().abs().sum(0).cpu(), s)
    _report("reduce_partials over 5 slabs", summed, want, bound)
    assert blockwise_err(summed.cpu(), wr.wgemm_ref(*wr.wgemm_inputs("short-tail"))) <= wr.wgemm_bar("short-tail", _x3())


def test_wgrad_gemm_is_deterministic():
    a, _ = _slabs("cut-blocks")
    b, _ = _slabs("cut-blocks")
    assert torch.equal(a, b)


@pytest.mark.parametrize("s", [1, 2, 3])
def test_wgrad_reduce_transform(s):
    """packed = G^T (sum_s P[s]) G at Cin * Cout = 48, no multiple of the kernel's 256 threads, within the transform's bound plus
    sum_bound over the S slabs."""
    cout, cin = 4, 12
    part = params.normal(9960 + s, s, 36, cout, cin)
    packed = _nan(9, cout, cin)
    _call(_lib().dvg_winograd_wgrad_reduce, part.to(dev()), s, packed, cin, cout)
    ref, bound = wr.reduce_ref(part)
    _report(f"reduce S={s}", packed, ref, bound)


# ---- end to end: the wrapper's padding, packing at t_off, slab reduction and saved-V path -----------------------------------------
@pytest.mark.parametrize("k", range(len(wr.WGRAD_E2E)), ids=wr.WGRAD_E2E_IDS)
def test_wgrad_end_to_end_block_by_block(k):
    """ops.winograd_wgrad_partial_multi against backward_ref.wgrad_ref(MODE_CONV3) in fp64 per (tap, 64 x 64 block), under 1.5 x
    the fp32 Winograd form's own error (floored at the worst case, capped at half a lost plane of dM / V in the product).  The
    saved-V case hands the wrapper the input transforms the forward's kernel makes, one buffer per item."""
    from dvg_amd import ops
    from tests.backward_ref import MODE_CONV3, wgrad_ref
    from tests.common import nhwc
    n, h, cin, cout, items, saved = wr.WGRAD_E2E[k]
    xs, dus = wr.wgrad_e2e_inputs(k)
    xd, dd = [nhwc(x) for x in xs], [nhwc(d) for d in dus]
    t = n * (h // 4) ** 2
    s = _lib().dvg_winograd_wgrad_splits(-(-items * t // 64) * 64, cin, cout)
    assert (s > 2) == (n == 9)          # the last case alone goes through dvg_reduce_partials
    vs = None
    if saved:
        assert t % 64 == 0
        vs = [_nan(36, t, cin) for _ in range(items)]
        for x, v in zip(xd, vs):
            _call(_lib().dvg_winograd_input, x, v, n, h, h, cin, 4, 0)
    packed = ops.winograd_wgrad_partial_multi(xd, dd, vs=vs)
    torch.cuda.synchronize()
    assert tuple(packed.shape) == (1, 9, cout, cin)
    f, b = wr.wgrad_e2e_figures(k), wr.wgrad_e2e_bar(k)
    e_hip = blockwise_err(packed[0].cpu(), wgrad_ref(MODE_CONV3, xs, None, dus))
    print(f"{wr.WGRAD_E2E_IDS[k]} S={s}: e_hip {e_hip:.2e} e32 {f['e32']:.2e} e_plane {f['e_plane']:.2e} bar {b:.2e}")
    assert e_hip <= b, (k, e_hip, b)
