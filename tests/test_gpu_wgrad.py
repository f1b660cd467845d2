"""The weight-gradient and gradient-routing KERNELS alone against the fp64 references of tests/backward_ref.py.

Direct weight gradient (dvg_conv_wgrad_multi, all three modes): block-wise error per (tap, 64x64 tile) against a bar that
comes from the fp32 yardstick at the same shape and is capped at half the error of a lost bf16 plane
(tests/test_backward_ref_host.py shows on the CPU that the cap never bites and that every planted defect fails the bar).
The small kernels (slab reductions, K4 -> W3, upsampling / activation backward, group sums): derived rounding bounds -
an n-term fp32 sum in any order is within gamma_(n-1) * sum |v| of the exact sum.  docs/DESIGN_NOTES_backward_tests.md has
the cases and the measured figures."""
import pytest
import torch

from oracle import params
from tests import backward_ref as br
from tests.common import dev, yardstick

pytestmark = pytest.mark.gpu


def nhwc_dev(t):
    """An NCHW-shaped CPU tensor as an NHWC-in-memory device tensor (plain torch: no kernel of ours on the way in)."""
    return t.to(dev()).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _partials(case):
    from dvg_amd import ops
    xs, skips, dus = br.wgrad_inputs(case)
    part = ops.conv_wgrad_partial_multi(case["mode"], [nhwc_dev(x) for x in xs],
                                        None if skips is None else [nhwc_dev(s) for s in skips],
                                        [nhwc_dev(d) for d in dus], upsample=case["up"])
    torch.cuda.synchronize()
    return part


@pytest.mark.parametrize("name", br.CASE_NAMES)
def test_direct_weight_gradient_against_fp64(name):
    from dvg_amd._lib import lib
    case = br.CASE_BY_NAME[name]
    part = _partials(case)
    taps = br.KSIZE[case["mode"]] ** 2
    assert tuple(part.shape[1:]) == (taps, case["cout"], case["c1"] + case["c2"])
    if lib().dvg_mfma_mode() == 1:
        assert part.shape[0] == case["splits"]
    f = br.case_figures(name)
    e_hip = br.blockwise_err(part.cpu().double().sum(0), f["ref"])
    b = br.case_bar(name)
    print(f"wgrad {name}: e_hip {e_hip:.2e} e_32 {f['e32']:.2e} e_plane {f['e_plane']:.2e} bar {b:.2e} "
          f"(splits {part.shape[0]})")
    assert e_hip <= b, (name, e_hip, f["e32"], f["e_plane"], b)


@pytest.mark.parametrize("name", ["conv3-n5-h8-c512+0-o512-x3", "conv4s2-n3-h8-c64+0-o128", "convT4s2-n7-h4-c64+0-o64-x3"])
def test_direct_weight_gradient_is_deterministic(name):
    """"deterministic, no atomics": the same launch twice gives the same bits, slab by slab."""
    a, b = _partials(br.CASE_BY_NAME[name]), _partials(br.CASE_BY_NAME[name])
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)


# ---- slab reductions -------------------------------------------------------------------------------------------------------
S_LIST = [1, 15, 16, 17, 63, 64, 65, 130]      # both sides of the 16-lane and the 64-stride loop boundaries
SLABS = [(9, 3, 4), (16, 8, 64)]                # n4 = 27 (not a multiple of the 16 columns of a workgroup) and 2048


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("S", S_LIST)
def test_reduce_partials_against_fp64(S):
    from dvg_amd import ops
    for taps, cout, cin in SLABS:
        part = params.normal(8000 + S, S, taps, cout, cin)
        ref, mag = br.reduce_partials_ref(part)
        d = part.to(dev())
        out = torch.full((taps, cout, cin), float("nan"), device=dev())
        ops.check(ops.lib().dvg_reduce_partials(ops._p(d), ops._p(out), S, out.numel(), ops._stream()), "reduce_partials")
        err = (out.cpu().double() - ref).abs()
        assert bool((err <= br.sum_bound(mag, S)).all()), (S, float(err.max()))
        if S == 1:
            assert torch.equal(out.cpu(), part[0])


@pytest.mark.parametrize("S", S_LIST)
def test_wgrad_finish_against_fp64(S):
    """Kinds 0, 1, 2; channel slices c_lo in {0, 64} of Ctot in {Cin, Cin + 64}; beta 0 (the slice prefilled with NaN: any read
    of it would show), 1 and 0.5 (random prefill); outside the slice the destination keeps its bits."""
    from dvg_amd import ops
    for taps, cout, cin in SLABS:
        k = 3 if taps == 9 else 4
        part = params.normal(8100 + S, S, taps, cout, cin)
        d_part = part.to(dev())
        for kind in (0, 1, 2):
            slices = [(0, cin)] if kind == 2 else [(0, cin), (0, cin + 64), (64, cin + 64)]
            for c_lo, ctot in slices:
                shape = {0: (cout, ctot, k, k), 1: (ctot, cout, k, k), 2: (taps, cout, cin)}[kind]
                for beta in (0.0, 1.0, 0.5):
                    dst0 = params.normal(8200 + S + kind, *shape)
                    exp, terms, mask = br.wgrad_finish_ref(part, dst0, kind, k, k, ctot, c_lo, beta)
                    if beta == 0.0:
                        dst0 = torch.where(mask, torch.full_like(dst0, float("nan")), dst0)
                    dst = dst0.to(dev())
                    ops.wgrad_finish(d_part, dst, kind, k, k, ctot=ctot, c_lo=c_lo, beta=beta)
                    got = dst.cpu()
                    tag = (S, taps, kind, c_lo, ctot, beta)
                    assert torch.equal(_bits(got)[~mask], _bits(dst0)[~mask]), tag
                    err = (got.double() - exp).abs()[mask]
                    bound = br.sum_bound(terms, S + (1 if beta != 0.0 else 0))[mask]
                    assert bool((err <= bound).all()), tag + (float(err.max()),)      # (a NaN fails the comparison)


# ---- K4 -> W3 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout,c1,c_lo,ctot", [(64, 64, 0, 64), (64, 64, 0, 128), (128, 64, 64, 192), (5, 7, 3, 12)])
def test_k4_to_w3_against_fp64_and_its_adjoint_identity(cout, c1, c_lo, ctot):
    """The 2x2 window sums (3 roundings per entry, one more for the beta * old term), into channel slices with beta 0 (NaN
    prefill) and 1, and <dK4, K4(W)> == <k4_to_w3(dK4), W> with K4(W) as the forward builds it (weights.k4_weight)."""
    from dvg_amd import ops, weights
    dk4p = params.normal(8300 + cout, 16, cout, c1)
    ref, mag = br.k4_to_w3_ref(dk4p)
    d_dk4p = dk4p.to(dev())
    mask = torch.zeros(cout, ctot, 3, 3, dtype=torch.bool)
    mask[:, c_lo:c_lo + c1] = True
    for beta in (0.0, 1.0):
        dw0 = params.normal(8301 + cout, cout, ctot, 3, 3)
        exp = dw0.double().clone()
        exp[:, c_lo:c_lo + c1] = ref + (dw0.double()[:, c_lo:c_lo + c1] if beta else 0.0)
        terms = mag + (dw0.double()[:, c_lo:c_lo + c1].abs() if beta else 0.0)
        if not beta:
            dw0 = torch.where(mask, torch.full_like(dw0, float("nan")), dw0)
        dw = dw0.to(dev())
        ops.k4_to_w3(d_dk4p, dw, c_lo, beta)
        got = dw.cpu()
        assert torch.equal(_bits(got)[~mask], _bits(dw0)[~mask])
        err = (got.double()[:, c_lo:c_lo + c1] - exp[:, c_lo:c_lo + c1]).abs()
        assert bool((err <= br.sum_bound(terms, 5 if beta else 4)).all()), (beta, float(err.max()))
        if not beta:
            hip_dw = got.double()[:, c_lo:c_lo + c1]
    # the forward's K4 against the fp64 construction (up to 4 terms per entry, fp32), then the adjoint identity
    w = params.normal(8302 + cout, cout, ctot, 3, 3, scale=0.05)
    k4 = weights.k4_weight(torch.nn.Parameter(w.to(dev())), c1).cpu().double().permute(1, 0, 2, 3)       # (Cout, C1, 4, 4)
    k4_ref, k4_mag = br.k4_of_w3(w[:, :c1]), br.k4_of_w3(w[:, :c1].abs())
    assert bool(((k4 - k4_ref).abs() <= br.sum_bound(k4_mag, 4)).all())
    lhs = float((br.k4_unpack(dk4p.double()) * k4_ref).sum())
    rhs = float((hip_dw * w[:, :c1].double()).sum())
    slack = float((br.sum_bound(mag, 4) * w[:, :c1].double().abs()).sum())
    print(f"k4 adjoint identity: {lhs:.9e} vs {rhs:.9e} (allowed {slack:.2e})")
    assert abs(lhs - rhs) <= slack


# ---- upsampling / group sums / activations -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,C", [(1, 3, 5, 4), (2, 8, 8, 64), (3, 4, 4, 68)])
def test_upsample2x_bwd_against_fp64(N, H, W, C):
    from dvg_amd import ops
    dxu = params.normal(8400 + C, N, C, 2 * H, 2 * W)
    ref, mag = br.upsample2x_bwd_ref(dxu)
    dx = ops.upsample2x_bwd(nhwc_dev(dxu))
    assert tuple(dx.shape) == (N, C, H, W) and ops.is_nhwc(dx)
    err = (dx.cpu().double() - ref).abs()
    assert bool((err <= br.sum_bound(mag, 4)).all()), float(err.max())


@pytest.mark.parametrize("gmap,blocks,block,shape", [((2, 0, 2, 1, 0), 4, 2, (6, 5, 7)), ((2, 0, 2, 1, 0), 4, 3, (68, 5, 7)),
                                                     ((0,), 1, 2, (6, 5, 7)), ((0, 1, 0), 2, 3, (64, 8, 8))])
def test_group_sum_against_fp64(gmap, blocks, block, shape):
    """dst[b] = the sum of the groups mapped to b; a block no group reads comes back as exact zeros; block_elems 420 and 7140
    are not multiples of the 1024 elements a workgroup pass covers."""
    from dvg_amd import ops
    g = len(gmap)
    src = params.normal(8500 + g + block, g * block, *shape)
    ref, mag, counts = br.group_sum_ref(src, gmap, blocks)
    shared = ops.SharedBlocks(torch.empty((blocks * block,) + shape, device=dev()), block, ops.shared_map(gmap, dev()), gmap)
    out = ops.group_sum(src.to(dev()), shared)
    assert tuple(out.shape) == (blocks * block,) + shape
    got = out.cpu().double().reshape(blocks, -1)
    ref, mag = ref.reshape(blocks, -1), mag.reshape(blocks, -1)
    for b in range(blocks):
        if counts[b] == 0:
            assert torch.equal(out.cpu().reshape(blocks, -1)[b], torch.zeros_like(out.cpu().reshape(blocks, -1)[b]))
        assert bool(((got[b] - ref[b]).abs() <= br.sum_bound(mag[b], counts[b])).all()), b
    if gmap == (0,):
        assert torch.equal(out.cpu(), src)


@pytest.mark.parametrize("act", [br.ACT_NONE, br.ACT_LRELU, br.ACT_TANH, br.ACT_SIGMOID])
@pytest.mark.parametrize("n", [1, 255, 257, 4097])
def test_act_bwd_against_the_fp64_derivative_from_y(act, n):
    """dy * act'(.) with the derivative evaluated from the saved OUTPUT y, within 4 ulp - of dy: the derivative factors are at
    most 1, and 1 - y * y near saturation cancels, so the factor's absolute error is that of a number near 1 (derivation in
    docs/DESIGN_NOTES_backward_tests.md)."""
    from dvg_amd import ops
    pre = params.normal(8600 + n, n, scale=2.0)
    y = {br.ACT_NONE: pre, br.ACT_LRELU: torch.nn.functional.leaky_relu(pre, 0.2), br.ACT_TANH: pre.tanh(),
         br.ACT_SIGMOID: pre.sigmoid()}[act]
    if n > 4:
        y[3] = 0.0              # LeakyReLU's branch at exactly 0 is the slope's (y > 0 is false)
    dy = params.normal(8601 + n, n)
    out = ops.act_bwd(dy.to(dev()), y.to(dev()), act, 0.2)
    ref = br.act_bwd_ref(dy, y, act, 0.2)
    err = (out.cpu().double() - ref).abs()
    assert out.shape == dy.shape and bool((err <= 4 * br.ulp32(dy)).all()), float((err / br.ulp32(dy)).max())


# ---- thin layers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks,N,nc,H,W,C", [(3, 2, 1, 64, 64, 64), (3, 3, 3, 24, 24, 64), (3, 2, 3, 10, 40, 128),
                                           (4, 2, 1, 64, 64, 64), (4, 3, 3, 40, 40, 128)])
def test_wgrad_thin_against_fp64(ks, N, nc, H, W, C):
    """dvg_wgrad_thin + its finish, as _LastLayer uses it: beta 0 and 1 into the row slice [64, 64 + C) of a wider
    ConvTranspose2d weight gradient; partial 4x32 tiles (24, 10 and 40 are not multiples of the tile), nc = 3."""
    from dvg_amd import ops
    ho, wo = (H, W) if ks == 3 else (H // 2, W // 2)
    inp = params.normal(8700 + H, N, nc, H, W)
    dout = params.normal(8701 + H, N, C, ho, wo)
    ref64, ref32 = br.wgrad_thin_ref(inp, dout, ks), br.wgrad_thin_ref(inp, dout, ks, dtype=torch.float32)
    d_inp, d_dout = inp.to(dev()), nhwc_dev(dout)
    for beta in (0.0, 1.0):
        big0 = params.normal(8702 + H, C + 128, nc, ks, ks)
        old = big0[64:64 + C].clone()
        if beta == 0.0:
            big0[64:64 + C] = float("nan")
        big = big0.to(dev())
        out = ops.wgrad_thin(d_inp, d_dout, ks, out=big[64:64 + C], beta=beta)
        got = big.cpu()
        assert out.data_ptr() == big[64:64 + C].data_ptr()
        assert torch.equal(_bits(got[:64]), _bits(big0[:64])) and torch.equal(_bits(got[64 + C:]), _bits(big0[64 + C:]))
        r64 = ref64 + (old.double() if beta else 0.0)
        r32 = ref32 + old if beta else ref32
        yardstick(f"wgrad_thin ks={ks} {(N, nc, H, W, C)} beta={beta}", got[64:64 + C], r32, r64, ratio=1.5)
