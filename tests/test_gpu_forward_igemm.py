"""The forward implicit-GEMM convolutions (dvg_conv3x3_bn_act_v2, dvg_conv4x4s2_bn_act_v2, dvg_convT4x4s2_bn_act_v2 and
splitk_finish_kernel in dvg_amd/csrc/conv_igemm2.hip) against fp64, workgroup tile by workgroup tile, at the cases of
tests/forward_ref.py: the raw arithmetic under the bar of docs/DESIGN_NOTES_forward_tests.md, the epilogue separately from the
kernel's own raw result within a derived bound, the split-K finish against the sum of its own partial tiles, the statistics rows
per run of images, and determinism.  tests/test_forward_ref_host.py shows on the CPU that the bar used here rejects every
planted defect and that each case still reaches the dispatch edge it was chosen for.  The yardstick of conv3 and conv4s2 emulates
the product build's arithmetic (bf16 triples, six MFMAs per tap): the figures and bars are that build's."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import params
from tests import forward_ref as fr
from tests.backward_ref import MODE_CONV3, MODE_CONV4S2, MODE_CONVT4S2, U32, sum_bound
from tests.common import dev, nhwc
from tests.forward_ref import ENERGY, LATENCY

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _operands(name):
    """The case's operands on the device: NHWC activations, the packed weight, the shared addend."""
    from dvg_amd import ops
    case = fr.CASE_BY_NAME[name]
    i = fr.fwd_inputs(case)
    add = None
    if i["addend"] is not None:
        t, block, gmap = i["addend"]
        add = ops.SharedBlocks(nhwc(t), block, ops.shared_map(gmap, dev()), gmap)
    return {"x": nhwc(i["x"]), "skip": None if i["skip"] is None else nhwc(i["skip"]),
            "wp": ops.pack_igemm_weight(i["w"].to(dev()), case["mode"] == MODE_CONVT4S2), "addend": add}


def _launch(name, policy, scale=None, shift=None, act=None, stats=False):
    """One call of the case's wrapper under the policy; returns (y, pooled y or None, statistics rows or None) on the device."""
    from dvg_amd import ops
    case, o = fr.CASE_BY_NAME[name], _operands(name)
    act = ops.ACT_NONE if act is None else act
    with ops.tile_policy(policy == ENERGY):
        if case["mode"] == MODE_CONV3:
            out = ops.conv3x3(o["x"], o["skip"], o["wp"], scale, shift, upsample=case["up"], act=act, pool=case["pool"],
                              stats=stats, addend=o["addend"])
        elif case["mode"] == MODE_CONV4S2:
            out = ops.conv4x4s2(o["x"], o["wp"], scale, shift, act=act, stats=stats)
        else:
            out = ops.convT4x4s2(o["x"], o["skip"], o["wp"], scale, shift, act=act, stats=stats, addend=o["addend"])
    out, st = out if stats else (out, None)
    y, yp = out if case["pool"] else (out, None)
    return y, yp, st


def _host(t):
    return t.detach().cpu().contiguous()


@functools.lru_cache(maxsize=None)
def _raw(name, policy):
    """The kernel's raw result u (ACT_NONE, unit scale, zero shift), NCHW on the CPU; shared, not to be modified."""
    cout = fr.CASE_BY_NAME[name]["cout"]
    y, yp, _ = _launch(name, policy, torch.ones(cout, device=dev()), torch.zeros(cout, device=dev()))
    if yp is not None:
        assert torch.equal(yp, F.max_pool2d(y, 2, 2)), "the fused max-pool must be bit-exact w.r.t. its own y"
    return _host(y)


def _scale_shift(name):
    k, cout = fr.CASE_NAMES.index(name), fr.CASE_BY_NAME[name]["cout"]
    return 1.0 + 0.1 * params.normal(9050 + 100 * k, cout), 0.1 * params.normal(9051 + 100 * k, cout)


# ---- the raw arithmetic ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,policy", fr.VARIANTS, ids=fr.VARIANT_IDS)
def test_raw_convolution_against_fp64_tile_by_tile(name, policy):
    """Both policies of the three 8 x 16 cases are variants of their own: each against fp64, not against each other."""
    f, b = fr.case_figures(name, policy), fr.case_bar(name, policy)
    u = _raw(name, policy)
    e_hip = fr.case_err(name, policy, u)
    case = fr.CASE_BY_NAME[name]
    same = float((u == fr.case_ordered(name, policy, True)).double().mean())
    print(f"{name} policy {policy}: {100 * same:.1f} % of the outputs bit-equal to ordered_fp32_ref(per_mfma=True)")
    print(f"{name} policy {policy} tile {case['tile'][policy]} splits {case['splits'][policy]}: e_hip {e_hip:.2e} e32 {f['e32']:.2e} "
          f"e_ord {f['e_ord']:.2e} e_mfma {f['e_mfma']:.2e} e_plane {f['e_plane']:.2e} bar {b:.2e} "
          f"(yardstick {fr.YARDSTICK[case['mode']]})")
    assert e_hip <= b, (name, e_hip, b)


# ---- the epilogue, separated from the arithmetic ---------------------------------------------------------------------------
@pytest.mark.parametrize("lrelu", [False, True], ids=["none", "lrelu"])
@pytest.mark.parametrize("name,policy", fr.VARIANTS, ids=fr.VARIANT_IDS)
def test_epilogue_from_the_kernels_own_raw_result(name, policy, lrelu):
    """y == act(u sc + sh) evaluated in fp64 from the kernel's OWN u.  Roundings, from the epilogue's code (the main kernel's
    `v = acc * sc + sf` - with an addend `(acc + av) * sc + sf`, whose inner sum IS the raw u - and the finish kernel's
    `u = v * sc + sf`): a product and a sum, at most two (one where the compiler fuses them), each of a quantity no larger than
    |u sc| + |sh|: 2 u32 (|u sc| + |sh|).  LeakyReLU's negative branch `v * slope` is a third: the result is within
    slope * (error of v) + u32 |slope v|; where the fp32 v and the fp64 v fall on different sides of 0 both are within the error of
    v of 0 and the results differ by at most 1.2 x it.  3 u32 (|u sc| + |sh|) covers all of them."""
    from dvg_amd import ops
    sc, sh = _scale_shift(name)
    u = _raw(name, policy).double()
    y, yp, _ = _launch(name, policy, sc.to(dev()), sh.to(dev()), ops.ACT_LRELU if lrelu else ops.ACT_NONE)
    v = u * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    slope = float(torch.tensor(0.2, dtype=torch.float32))          # the kernel's slope is an fp32 argument
    want = torch.where(v > 0, v, v * slope) if lrelu else v
    bound = (3 if lrelu else 2) * U32 * ((u * sc.double().view(1, -1, 1, 1)).abs() + sh.double().abs().view(1, -1, 1, 1))
    excess = ((_host(y).double() - want).abs() - bound).max()
    print(f"{name} policy {policy} lrelu {lrelu}: max (|y - want| - bound) {float(excess):.2e}, max bound {float(bound.max()):.2e}")
    assert bool(torch.isfinite(y).all()) and float(excess) <= 0.0
    if yp is not None:
        assert torch.equal(yp, F.max_pool2d(y, 2, 2))


# ---- split K against the unsplit sum ---------------------------------------------------------------------------------------
_SPLIT = [c["name"] for c in fr.FWD_CASES if c["splits"][LATENCY] > 1]


@pytest.mark.parametrize("name", _SPLIT)
def test_splitk_finish_sums_its_partials(name):
    """The finish kernel's result lies within sum_bound of the fp64 sum of the S partial tiles the main kernel left in the
    workspace (+ the addend): S (+ 1) terms in a fixed order.  That the total agrees with fp64 within the bar is
    test_raw_convolution_against_fp64_tile_by_tile's assertion at the same case; here additionally every partial must be
    the convolution over its own chunks within the bar formula evaluated for that convolution."""
    from dvg_amd import ops
    case = fr.CASE_BY_NAME[name]
    s, cout, n = case["splits"][LATENCY], case["cout"], case["n"]
    ho, wo = fr.out_hw(case)
    y, _, _ = _launch(name, LATENCY, torch.ones(cout, device=dev()), torch.zeros(cout, device=dev()))
    torch.cuda.synchronize()
    # the launch's workspace: one buffer per (stream, size), handed out again by the call that sized the launch
    ws = ops._splitk_ws(case["mode"], n, case["h"], case["w"], case["c1"] + case["c2"], cout, y.numel(), y.device)
    assert ws is not None and ws.numel() == s * y.numel()
    parts = _host(ws.view(s, n, ho, wo, cout).permute(0, 1, 4, 2, 3)).double()
    u = _host(y)
    assert torch.equal(u, _raw(name, LATENCY))
    args = fr.case_args(case)
    a = fr.addend_images(args[5], n)
    exact, mag, terms = parts.sum(0), parts.abs().sum(0), s
    if a is not None:
        exact, mag, terms = exact + a.double(), mag + a.double().abs(), s + 1
    excess = ((u.double() - exact).abs() - sum_bound(mag, terms)).max()
    print(f"{name}: {terms} terms, max (|u - sum| - bound) {float(excess):.2e}")
    assert float(excess) <= 0.0
    mode, x, skip, w = args[:4]
    tile, par = case["tile"][LATENCY], mode == MODE_CONVT4S2
    emu = fr.case_ordered_parts(name, LATENCY, True)[1]
    for k, (lo, hi) in enumerate(fr.split_chunks((case["c1"] + case["c2"]) // 16, s)):
        wk = torch.zeros_like(w)
        if mode == MODE_CONVT4S2:
            wk[16 * lo:16 * hi] = w[16 * lo:16 * hi]
        else:
            wk[:, 16 * lo:16 * hi] = w[:, 16 * lo:16 * hi]
        # the partial is a convolution of its own: the case's bar formula evaluated for it
        ref = fr.forward_ref(mode, x, skip, wk, case["up"])
        yard = emu[k] if fr.YARDSTICK[mode] == "mfma" else fr.forward_ref(mode, x, skip, wk, case["up"], dtype=torch.float32)
        e_y = fr.tilewise_err(yard, ref, *tile, parity=par)
        e_pl = min(fr.tilewise_err(fr.plant("plane_w", mode, x, skip, wk, case["up"]), ref, *tile, parity=par),
                   fr.tilewise_err(fr.plant("plane_x", mode, x, skip, wk, case["up"]), ref, *tile, parity=par))
        b = fr.bar(e_y, fr.mode_worst(mode), e_pl)
        e = fr.tilewise_err(parts[k], ref, *tile, parity=par)
        print(f"{name}: split {k} chunks [{lo}, {hi}): e_hip {e:.2e} yardstick {e_y:.2e} e_plane {e_pl:.2e} bar {b:.2e}")
        assert e <= b


# ---- the statistics rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,policy", fr.VARIANTS, ids=fr.VARIANT_IDS)
def test_statistics_rows_per_run_of_images(name, policy):
    """The rows hold, per channel, the sum and the sum of squares of the PRE-ACTIVATION v = (acc + addend) * scale + shift
    (conv_igemm2_kernel: s1 += v, s2 += v * v before the activation; splitk_finish_kernel likewise) - with ACT_NONE exactly the
    stored y.  Without a split they are per tile in image-major order, a tile spanning st.tile_images images: each run's column
    sums against the fp64 sums of the stored fp32 y over exactly the run's PRESENT images (so the values' own rounding does
    not enter), within sum_bound - n terms for the sums, n + 1 for the squares (each square is rounded before it is added).
    With a split the rows are the finish blocks': totals only, and tile_images == 0."""
    from dvg_amd import ops
    case = fr.CASE_BY_NAME[name]
    sc, sh = _scale_shift(name)
    y, yp, st = _launch(name, policy, sc.to(dev()), sh.to(dev()), ops.ACT_NONE, stats=True)
    y0, _, _ = _launch(name, policy, sc.to(dev()), sh.to(dev()), ops.ACT_NONE)
    assert torch.equal(y, y0), "asking for statistics must not change the output"
    v, rows = _host(y).double(), _host(st).double()
    n, (ho, wo) = case["n"], fr.out_hw(case)
    ti = case["tile"][policy][0]
    if case["splits"][policy] > 1:
        assert st.tile_images == 0
        runs = [range(n)]
        got = rows.sum(0, keepdim=True)
    else:
        assert st.tile_images == ti
        nruns = -(-n // ti)
        assert rows.shape[0] % nruns == 0
        runs = [range(r * ti, min(n, (r + 1) * ti)) for r in range(nruns)]
        got = rows.reshape(nruns, rows.shape[0] // nruns, 2, case["cout"]).sum(1)
    worst = 0.0
    for r, imgs in enumerate(runs):
        vi = v[list(imgs)]
        terms = len(imgs) * ho * wo
        for j, (q, extra) in enumerate(((vi, 0), (vi * vi, 1))):
            d = (got[r, j] - q.sum((0, 2, 3))).abs()
            bound = sum_bound(q.abs().sum((0, 2, 3)), terms + extra)
            worst = max(worst, float((d / bound.clamp_min(1e-300)).max()))
            assert bool((d <= bound).all()), (name, r, j, float((d - bound).max()))
    print(f"{name} policy {policy}: {rows.shape[0]} rows, {len(runs)} runs of {st.tile_images} images, worst |d| / bound {worst:.3f}")


# ---- determinism -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["conv3-n2-8x8-c208+0-o64-pool", "conv4s2-n3-8x8-c144+0-o64", "convT4s2-n2-8x8-c256+0-o64"])
def test_two_launches_agree_bit_for_bit(name):
    sc, sh = _scale_shift(name)
    a = _launch(name, LATENCY, sc.to(dev()), sh.to(dev()), None, stats=True)
    b = _launch(name, LATENCY, sc.to(dev()), sh.to(dev()), None, stats=True)
    for t, r in zip(a, b):
        assert (t is None and r is None) or torch.equal(t, r)
