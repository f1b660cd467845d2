"""GPU: train.py --ssim_weight - dvg_frame_ssim_loss against the fp64 reference (tests/ssim_loss_ref.py), on identical images, under
`accumulate`, its determinism, against torch_ssim_sum in fp64 on the device, and its argument checks; and the Trainer: --ssim_weight 0
changes no bit, fused against unfused losses, the step-by-step path against the batched one, three replays of one hipGraph against
eager iterations, the epoch line.

Shapes of the Trainer tests: tests/test_gpu_frame_loss.py's (dcgan_64, batch 4, 2 + 2 frames, the in-repo synthetic smmnist)."""
import ctypes
import math

import pytest
import torch

from tests import frame_loss_ref, ssim_loss_ref as ref, train_harness
from tests.common import rel_err, rel_err_elem

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (S, K, planes, H, W).  The kernel holds 5 MR + 3 RS fp64 rows of W - 10 in 150 KiB of LDS: one workgroup per image while the 5 (H - 10)
# map rows and a strip of min(H, 16) rows or more fit (strips of up to RS = 30 rows: RS - 10 map rows forward, RS pixel rows backward),
# else bands of R pixel rows with strips of 16 (W = 128: R = 12), or of 11 for very wide rows (W = 200: R = 3).
CASES = {
    "row": (1, 1, 1, 11, 12),        # one output row, two positions
    "small": (1, 1, 1, 12, 16),
    "shared": (2, 3, 1, 12, 16),     # the target is shared by three calls
    "odd": (1, 2, 3, 21, 20),        # odd planes, H neither a strip nor a power of two
    "strip+1": (1, 1, 1, 31, 16),    # whole image, RS = 30: one input row more than a forward strip AND one pixel row more than a backward one
    "whole128": (1, 1, 1, 32, 128),  # the tallest 128-wide image one workgroup takes (RS = 17: 7 + 7 + 7 + 1 map rows forward, 17 + 15 backward)
    "bands128": (1, 1, 1, 33, 128),  # one row more: three bands of 12 rows (12 + 12 + 9)
    "band+1": (1, 2, 1, 37, 128),    # one pixel row more than three bands: the fourth band owns one row and its 10 halo map rows
    "wide": (1, 1, 1, 21, 200),      # strips of the window's 11 rows, bands of 3
    "f": (1, 3, 2, 64, 64),
    "g": (1, 1, 1, 128, 128),
    "h": (3, 3, 4, 64, 64),          # training-like: B = 4, C = 1
}
BAR = 1e-6                           # the project's bars for dvg_frame_losses_ext: fp64 arithmetic and ONE fp32 store is 6e-8


def _weights(shape):
    S, K, planes, H, W = shape
    m = planes * (H - 10) * (W - 10)
    return [1.0 / m, 0.5 / m, 2.0 / m][:K]


_REF = {}


def _reference(case, kind):
    """(pred, target, sums, gradient) of a seeded case: computed once per (case, kind), shared, never modified."""
    key = (case, kind)
    if key not in _REF:
        shape = CASES[case]
        pred, target = ref.case(kind, 20 + sorted(CASES).index(case), *shape)
        _REF[key] = (pred, target, ref.sums(pred, target), ref.gradient(pred, target, _weights(shape)))
    return _REF[key]


def test_the_cases_sit_on_the_boundaries_they_name():
    from dvg_amd import _lib
    blocks = _lib.lib().dvg_frame_ssim_loss_blocks       # S x planes x bands: the K calls share a workgroup
    want = {"strip+1": 1, "whole128": 1, "bands128": 3, "band+1": 4, "wide": 7, "f": 2, "g": 11, "h": 12}
    for case, n in want.items():
        S, K, planes, H, W = CASES[case]
        assert blocks(S, planes, H, W) == n, case


# ---- 1. against the fp64 reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "sparse", "const"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_against_the_fp64_reference(case, kind):
    """Every element compared.  The same formulas in fp32 miss these bars on `const` by more than 100 x (tests/test_ssim_loss_host.py)."""
    from dvg_amd import ops
    shape = CASES[case]
    K = shape[1]
    pred, target, sums_ref, grad = _reference(case, kind)
    sums, dpred = ops.frame_ssim_loss(pred.to(DEV), target.to(DEV), _weights(shape))
    assert sums.shape == (K,) and dpred.shape == pred.shape and sums.dtype == dpred.dtype == torch.float32
    e_sums, e_grad = rel_err_elem(sums, sums_ref), rel_err(dpred, grad)
    print(f"\nframe_ssim_loss {case} {shape} {kind}: sums rel_err_elem {e_sums:.2e}  dpred rel_err {e_grad:.2e}")
    assert bool(torch.isfinite(dpred).all()) and bool(torch.isfinite(sums).all())
    assert e_sums < BAR, (sums.cpu(), sums_ref)
    assert e_grad < BAR


@pytest.mark.parametrize("case", sorted(CASES))
def test_identical_images_give_an_exact_zero(case):
    """pred == target: S = 1 exactly at every position (the contraction-off ratio), so the sums are 0.0; the gradient is a difference of
    equal terms: |dpred| <= 1e-9 per unit weight (the fp64 formulas give 5e-15 at 64 x 64)."""
    from dvg_amd import ops
    shape = CASES[case]
    pred, target = ref.case("identical", 3, *shape)
    sums, dpred = ops.frame_ssim_loss(pred.to(DEV), target.to(DEV), [1.0] * shape[1])
    worst = float(dpred.abs().max())
    print(f"\nframe_ssim_loss {case} identical: sums {sums.tolist()}  max |dpred| per unit weight {worst:.2e}")
    assert bool(torch.isfinite(dpred).all()) and bool(torch.isfinite(sums).all())
    assert float(sums.abs().max()) == 0.0
    assert worst <= 1e-9


# ---- 2. accumulate ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["odd", "band+1", "h"])
def test_accumulate_adds_to_what_frame_losses_ext_wrote(case):
    """dpred of frame_losses_ext(l1, G = 1) on quantised inputs (where its signs are the reference's), then the DSSIM gradient added by
    its owner: against the fp64 sum of both gradients."""
    from dvg_amd import ops
    shape = CASES[case]
    S, K, planes, H, W = shape
    pred, target = frame_loss_ref.quantised_case(61, *shape)
    n = planes * H * W
    w_pix, w_ssim = [1.0 / n, 0.5 / n, 2.0 / n][:K], _weights(shape)
    want = frame_loss_ref.gradient(pred, target, "l1", w_pix, 1.0, 1e-3).double() + ref.gradient(pred, target, w_ssim)
    p, t = pred.to(DEV), target.to(DEV)
    _, d = ops.frame_losses_ext(p, t, "l1", w_pix, gdl=1.0)
    before = d.clone()
    sums, d2 = ops.frame_ssim_loss(p, t, w_ssim, dpred=d)
    assert d2 is d and not torch.equal(d, before)
    e = rel_err(d, want)
    print(f"\naccumulate {case}: rel_err {e:.2e}  sums rel_err_elem {rel_err_elem(sums, ref.sums(pred, target)):.2e}")
    assert e < BAR
    assert rel_err_elem(sums, ref.sums(pred, target)) < BAR


def test_no_accumulate_overwrites_and_a_zero_weight_adds_an_exact_zero():
    from dvg_amd import _lib, ops
    shape = CASES["shared"]
    S, K, planes, H, W = shape
    pred, target, sums_ref, _ = _reference("shared", "noise")
    p, t = pred.to(DEV), target.to(DEV)
    # accumulate = 0 into a NaN-filled buffer (the C ABI: the wrapper allocates its own)
    lib = _lib.lib()
    d = torch.full_like(p, float("nan"))
    sums = torch.empty(K, device=DEV)
    w = torch.tensor(_weights(shape), device=DEV)
    part = torch.empty(lib.dvg_frame_ssim_loss_blocks(S, planes, H, W) * K, dtype=torch.float64, device=DEV)
    rc = lib.dvg_frame_ssim_loss(p.data_ptr(), t.data_ptr(), sums.data_ptr(), d.data_ptr(), S, K, planes, H, W, w.data_ptr(), 0,
                                 part.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isfinite(d).all())
    assert torch.equal(d, ops.frame_ssim_loss(p, t, _weights(shape))[1])
    # w_ssim[1] = 0: call 1's dpred keeps its bits under accumulate, is 0 without, and sums[1] is still reported
    w0 = [_weights(shape)[0], 0.0, _weights(shape)[2]]
    base = torch.randn_like(p)
    acc = base.clone()
    sums_a, _ = ops.frame_ssim_loss(p, t, w0, dpred=acc)
    assert torch.equal(acc[:, 1], base[:, 1]) and not torch.equal(acc[:, 0], base[:, 0]) and not torch.equal(acc[:, 2], base[:, 2])
    sums_b, fresh = ops.frame_ssim_loss(p, t, w0)
    assert float(fresh[:, 1].abs().max()) == 0.0 and float(fresh[:, 0].abs().max()) > 0.0
    assert rel_err_elem(sums_a, sums_ref) < BAR and torch.equal(sums_a, sums_b)


# ---- 3. determinism, the torch composition -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["odd", "h"])
def test_two_calls_give_the_same_bits(case):
    from dvg_amd import ops
    shape = CASES[case]
    pred, target, _, _ = _reference(case, "noise")
    p, t = pred.to(DEV), target.to(DEV)
    a = ops.frame_ssim_loss(p, t, _weights(shape))
    b = ops.frame_ssim_loss(p, t, _weights(shape))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float(a[0].min()) > 0.0


@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_against_torch_ssim_sum_in_fp64_on_the_device(case):
    """The slice composition in fp64 on the GPU (no convolution library involved) and its autograd: the bars of the reference test."""
    from dvg_amd import frame_loss, ops
    shape = CASES[case]
    K = shape[1]
    pred, target, _, _ = _reference(case, "noise")
    p32, t32 = pred.to(DEV), target.to(DEV)
    w = _weights(shape)
    sums, dpred = ops.frame_ssim_loss(p32, t32, w)
    p = p32.double().requires_grad_(True)
    terms = [frame_loss.torch_ssim_sum(p[:, k], t32.double()) for k in range(K)]
    sum(wk * v for wk, v in zip(w, terms)).backward()
    e_sums, e_grad = rel_err_elem(sums, torch.stack(terms).detach()), rel_err(dpred, p.grad)
    print(f"\nframe_ssim_loss vs torch fp64 on the device {case}: sums rel_err_elem {e_sums:.2e}  dpred rel_err {e_grad:.2e}")
    assert e_sums < BAR and e_grad < BAR


# ---- 4. argument checks -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_their_code_and_launch_nothing():
    from dvg_amd import _lib, ops
    lib = _lib.lib()
    pred, target = ref.case("noise", 1, 1, 1, 1, 12, 16)
    pred, target = pred.to(DEV), target.to(DEV)
    sums = torch.full((3,), -7.0, device=DEV)
    dpred = torch.full((1, 4, 1, 12, 16), -7.0, device=DEV)
    w = torch.ones(4, device=DEV)
    part = torch.full((64,), -7.0, device=DEV, dtype=torch.float64)

    def call(p=None, t=None, S=1, K=1, planes=1, H=12, W=16):
        return lib.dvg_frame_ssim_loss(p or pred.data_ptr(), t if t is not None else target.data_ptr(), sums.data_ptr(),
                                       dpred.data_ptr(), S, K, planes, H, W, w.data_ptr(), 0, part.data_ptr(), None)
    assert call(H=10) == 1 and call(H=10, W=12) == 1 and call(W=14) == 1 and call(K=4) == 1      # DVG_ERR_SHAPE
    for H, W in ((10, 16), (10, 12), (12, 14)):
        assert lib.dvg_frame_ssim_loss_blocks(1, 1, H, W) <= 0
    assert call(t=ctypes.c_void_p(0)) == 2                                                        # DVG_ERR_NULL
    assert call(p=ctypes.c_void_p(pred.data_ptr() + 4)) == 4                                      # DVG_ERR_ALIGN
    torch.cuda.synchronize()
    assert float(sums.max()) == -7.0 and float(dpred.max()) == -7.0 and float(part.max()) == -7.0
    assert call() == 0                                       # the same buffers, a served shape: it does launch
    torch.cuda.synchronize()
    assert float(sums[0]) > 0.0
    for bad in ((1, 1, 1, 10, 16), (1, 1, 1, 12, 14), (1, 4, 1, 12, 16)):                         # no fallback behind the op: it raises
        with pytest.raises(RuntimeError, match="unsupported shape"):
            ops.frame_ssim_loss(torch.zeros(bad, device=DEV), torch.zeros(bad[:1] + bad[2:], device=DEV), [1.0] * bad[1])
    with pytest.raises(RuntimeError, match="shaped like pred"):
        ops.frame_ssim_loss(pred, target, [1.0], dpred=torch.zeros(1, 1, 1, 12, 12, device=DEV))


def test_new_weights_during_a_capture_are_refused():
    from dvg_amd import graphs, ops
    pred, target = ref.case("noise", 1, 1, 1, 1, 12, 16)
    pred, target = pred.to(DEV), target.to(DEV)
    ops.frame_ssim_loss(pred, target, [0.125])
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="capture"):
        with graphs.capturing():
            ops.frame_ssim_loss(pred, target, [0.377])


# ---- the Trainer ---------------------------------------------------------------------------------------------------------------------
L1_SSIM = ["--frame_loss", "l1", "--ssim_weight", "0.2"]


@pytest.fixture(scope="module")
def batches():
    return train_harness.make_batches(5)


def _one_train_model(tr, x):
    """(loss, gradient arena) of one train_model from the Trainer's initial state."""
    tr.arena.g.zero_()
    torch.manual_seed(77)
    tr.train_model(x)
    torch.cuda.synchronize()
    return tr.last_loss, tr.arena.g.clone()


def _compare_ranges(tr, ga, gb, bar):
    for name, (lo, hi) in {"gp": tr.rng_gp, "fp": tr.rng_fp, "dec": tr.rng_dec, "enc": tr.rng_enc}.items():
        na, d = float(ga[lo:hi].double().norm()), float((ga[lo:hi].double() - gb[lo:hi].double()).norm())
        print(f"gradient range {name}: |a| {na:.3e}  |a - b| / |a| {d / max(na, 1e-30):.2e}")
        assert na > 0 and d <= bar * na, (name, d / max(na, 1e-30))


def test_ssim_weight_zero_changes_no_bit(batches):
    """--ssim_weight 0 is the run without the flag: no spec, the same code path, loss and parameters bit-equal."""
    res = []
    for extra in ([], ["--ssim_weight", "0"]):
        tr = train_harness.trainer(extra)
        assert tr.frame_loss is None and tr.frame_terms is None
        loss, _ = _one_train_model(tr, batches[0])
        res.append((loss, tr.arena.p.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])
    tr = train_harness.trainer(L1_SSIM)
    assert tr.frame_loss.label() == "l1 + 0.2 ssim" and tr.frame_terms.epoch_line() == "     frame loss: l1 + 0.2 ssim   pixel 0  gdl 0  ssim 1"


def test_fused_losses_match_the_torch_composition(batches):
    """--frame_loss l1 --ssim_weight 0.2, one train_model from the same initial state with fused_losses True (dvg_frame_losses_ext +
    dvg_frame_ssim_loss) against False (torch_terms + torch_ssim_sum in fp32 + a scalar autograd graph).  Bars: the sibling test's
    (tests/test_gpu_frame_loss.py::test_fused_losses_match_the_torch_composition): value 1e-4 max(1, |u|), gradient ranges 2e-3.  The
    fp32 composition does not need more: tests/test_ssim_loss_host.py prints, for torch_ssim_sum in fp32 against fp64 on noise at this
    frame size, a mean-SSIM error of 6.7e-9 and a gradient rel_err of 1.6e-6 (sparse: 9.1e-9 and 5.0e-7), three orders under 2e-3."""
    res, stats = [], []
    for fused in (True, False):
        tr = train_harness.trainer(L1_SSIM)
        tr.fused_losses = fused
        res.append(_one_train_model(tr, batches[0]))
        stats.append(tr.frame_terms.read_and_reset())
    (la, ga), (lb, gb) = res
    print(f"\nfused {la!r} torch {lb!r}  stats {stats}")
    assert abs(la - lb) <= 1e-4 * max(1.0, abs(la)), (la, lb)
    _compare_ranges(tr, ga, gb, 2e-3)
    assert stats[0]["iterations"] == stats[1]["iterations"] == 1
    assert stats[0]["pixel"] > 0 and abs(stats[0]["pixel"] - stats[1]["pixel"]) <= 1e-4 * stats[0]["pixel"], stats
    assert -1.0 < stats[0]["ssim"] <= 1.0 and abs(stats[0]["ssim"] - stats[1]["ssim"]) <= 1e-4, stats


def test_step_by_step_path_matches_the_batched_one(batches):
    """time_batched False (one decoder call per step, torch_terms + torch_ssim_sum per call) against the batched path (the two
    kernels), with the sibling test's bars and its split: under l1 a last-bit difference of the two forward passes may flip a sign, so
    --frame_loss l1 --ssim_weight 0.2 compares the value (1e-4 max(1, |u|)); --frame_loss charbonnier --ssim_weight 0.2 is smooth and
    compares the gradient ranges too (2e-3).  No wider: see test_fused_losses_match_the_torch_composition for the fp32 figures."""
    vals = []
    for tb in (False, True):
        tr = train_harness.trainer(L1_SSIM)
        tr.time_batched = tb
        vals.append(_one_train_model(tr, batches[0])[0])
    print(f"\nl1 + ssim: step by step {vals[0]!r} batched {vals[1]!r}")
    assert abs(vals[0] - vals[1]) <= 1e-4 * max(1.0, abs(vals[0])), vals
    res = []
    for tb in (False, True):
        tr = train_harness.trainer(["--frame_loss", "charbonnier", "--ssim_weight", "0.2"])
        tr.time_batched = tb
        res.append(_one_train_model(tr, batches[0]))
    (la, ga), (lb, gb) = res
    print(f"charbonnier + ssim: step by step {la!r} batched {lb!r}")
    assert abs(la - lb) <= 1e-4 * max(1.0, abs(la)), (la, lb)
    _compare_ranges(tr, ga, gb, 2e-3)


def test_graph_replay_matches_eager_with_the_flag_on(batches):
    """GraphedIteration under --frame_loss l1 --ssim_weight 0.2: two eager warm-up iterations, then three replays of one captured
    hipGraph, against five eager iterations: the same launches on the same bits, so values, parameters, buffers, moments and the
    epoch line's device sums are bit-equal.  The SSIM sums advance inside the replayed graph."""
    res = []
    for graphed in (False, True):
        tr = train_harness.trainer(L1_SSIM, seed=11)
        step, out = train_harness.iterate(tr, batches[:5], graphed, warmup=2,
                                          each=lambda tr, step, i: (tr.last_loss, step.graph if graphed else None))
        out = [(r + (loss,), graph) for r, (loss, graph) in out]
        if graphed:
            assert not step.failed and out[2][1] is not None and all(g is out[2][1] for _, g in out[2:])
            assert out[0][1] is None and out[1][1] is None and step.calls == 5
        res.append(([o[0] for o in out], [{k: t.detach().clone() for k, t in m.state_dict().items()} for m in tr.modules],
                    {n: getattr(tr.arena, n).clone() for n in ("p", "m", "v")}, tr.frame_terms.acc.tolist(),
                    tr.frame_terms.acc_ssim.tolist(), tr.frame_terms.epoch_line()))
    (la, sa, aa, ca, ssa, linea), (lb, sb, ab, cb, ssb, lineb) = res
    print(f"\neager  {linea}\ngraph  {lineb}\nvalues eager {la}\nvalues graph {lb}")
    for n in ("p", "m", "v"):
        print(f"arena {n}: max |eager - graph| {float((aa[n] - ab[n]).abs().max()):.3e}")
    assert la == lb
    for a, b in zip(sa, sb):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    for n in ("p", "m", "v"):
        assert torch.equal(aa[n], ab[n]), n
    assert ca == cb and ssa == ssb and linea == lineb
    assert ca[2] == 5.0 and ca[3] == 5.0 * 3 * 4 * 64 * 64 and ssa[1] == 5.0 * 3 * 4 * 54 * 54
    assert linea.startswith("     frame loss: l1 + 0.2 ssim   pixel ")
    ssim = float(linea.split("  ssim ")[1])
    assert -1.0 < ssim <= 1.0 and math.isfinite(ssim)
