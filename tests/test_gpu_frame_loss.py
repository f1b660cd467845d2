"""GPU: train.py --frame_loss / --gdl_weight - dvg_frame_losses_ext against the fp64 reference (tests/frame_loss_ref.py) on inputs
whose differences are exact in fp32, against the torch composition (dvg_amd.frame_loss.torch_terms) in fp32 on the device, its
determinism and argument checks; and the Trainer: the default flags change no bit, fused against unfused losses, the step-by-step
path against the batched one, and three iterations replayed from one hipGraph against three eager ones.

Shapes of the Trainer tests: tests/test_gpu_lr_schedule.py's (dcgan_64, batch 4, 2 + 2 frames, the in-repo synthetic smmnist)."""
import ctypes

import pytest
import torch

from tests import frame_loss_ref as ref, train_harness
from tests.common import rel_err, rel_err_elem

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (S, K, planes, H, W): the smallest shapes at which the decomposition into (step, plane, 16-row band) workgroups of 4-pixel
# vectors can go wrong
CASES = {
    "a": (1, 1, 1, 1, 4),        # no vertical edge, one vector per row
    "b": (1, 1, 1, 2, 4),
    "c": (2, 3, 1, 4, 4),
    "d": (1, 2, 3, 5, 8),        # H not a multiple of any band; a wave spans several rows
    "e": (2, 3, 5, 17, 12),      # odd planes, W not a power of two, one row past a 16-row band
    "f": (1, 3, 2, 64, 64),
    "g": (1, 1, 1, 128, 128),
    "h": (3, 3, 4, 64, 64),      # training-like: B = 4, C = 1
}
KINDS = ["l1", "charbonnier"]
EPS = 1e-3


def _weights(shape):
    S, K, planes, H, W = shape
    n = planes * H * W
    return [1.0 / n, 0.5 / n, 2.0 / n][:K]


_REF = {}


def _reference(case, kind, G):
    """(pred, target, pix, gdl, gradient) of a quantised case: computed once per (case, kind, G), shared, never modified."""
    key = (case, kind, G)
    if key not in _REF:
        shape = CASES[case]
        pred, target = ref.quantised_case(40 + ord(case), *shape)
        pix, gdl = ref.sums(pred, target, kind, EPS)
        _REF[key] = (pred, target, pix, gdl, ref.gradient(pred, target, kind, _weights(shape), G, EPS))
    return _REF[key]


# ---- 1. against the fp64 reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [0.0, 1.0])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_against_the_fp64_reference(case, kind, G):
    """Inputs quantised to multiples of 1/256 with about half the pixels blank in both tensors: every difference is exact in fp32,
    so every sign is the reference's, and tied edges (gradient exactly 0) occur in quantity.  Every element is compared; the bars
    are tests/test_gpu_batchnorm.py::test_frame_losses's."""
    from dvg_amd import ops
    shape = CASES[case]
    K = shape[1]
    pred, target, pix, gdl, grad = _reference(case, kind, G)
    sums, dpred = ops.frame_losses_ext(pred.to(DEV), target.to(DEV), kind, _weights(shape), eps=EPS, gdl=G)
    assert sums.shape == (2, K) and dpred.shape == pred.shape
    ties = ref.tied_fraction(pred, target)
    e_pix = rel_err_elem(sums[0], pix)
    e_gdl = rel_err_elem(sums[1], gdl) if G and float(gdl.abs().max()) > 0 else 0.0
    e_grad = rel_err(dpred, grad)
    print(f"\nframe_losses_ext {case} {shape} {kind} G={G}: tied edges {100 * ties:.1f} %  sums rel_err_elem pix {e_pix:.2e} "
          f"gdl {e_gdl:.2e}  dpred rel_err {e_grad:.2e}")
    assert e_pix < 1e-6, (sums.cpu(), pix)
    if G:
        assert rel_err_elem(sums, torch.stack([pix, gdl])) < 1e-6, (sums.cpu(), pix, gdl)
    else:
        assert float(sums[1].abs().max()) == 0.0             # no edge work: an exact 0
    assert e_grad < 1e-6
    assert bool(torch.isfinite(dpred).all())
    if G and shape[3] * shape[4] >= 16:
        assert ties > 0.03, ties                               # the case does exercise sign(0) = 0


# ---- 2. against the torch composition in fp32 on the device -----------------------------------------------------------------------
@pytest.mark.parametrize("G", [0.0, 1.0])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_against_torch_terms_in_fp32(case, kind, G):
    """Unquantised inputs, pred = target + 0.1 normal.  Both sides form every difference by ONE IEEE subtraction of the same two
    floats, so the signs are identical by construction; every element is compared."""
    from dvg_amd import frame_loss, ops
    shape = CASES[case]
    K = shape[1]
    pred, target = ref.noisy_case(80 + ord(case), *shape)
    pred, target = pred.to(DEV), target.to(DEV)
    w = _weights(shape)
    spec = frame_loss.FrameLossSpec(kind, EPS, G)
    sums, dpred = ops.frame_losses_ext(pred, target, spec, w)
    p = pred.clone().requires_grad_(True)
    total, terms = 0, []
    for k in range(K):
        pix, gdl = frame_loss.torch_terms(p[:, k], target, spec)
        terms.append(torch.stack([pix.detach(), gdl.detach()]))
        total = total + w[k] * (pix + G * gdl)
    total.backward()
    e_grad, e_sums = rel_err(dpred, p.grad), rel_err_elem(sums, torch.stack(terms, 1))
    print(f"\nframe_losses_ext vs torch fp32 {case} {kind} G={G}: dpred rel_err {e_grad:.2e}  sums rel_err_elem {e_sums:.2e}")
    assert e_grad < 1e-6
    # the sums of two fp32 summation orders: n values of one sign, each side within ~sqrt(n) ulp-sized steps of the truth
    assert e_sums < 1e-5


# ---- 3. determinism, argument checks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["e", "h"])
def test_two_calls_give_the_same_bits(case):
    from dvg_amd import ops
    shape = CASES[case]
    pred, target = ref.noisy_case(7, *shape)
    pred, target = pred.to(DEV), target.to(DEV)
    a = ops.frame_losses_ext(pred, target, "charbonnier", _weights(shape), eps=EPS, gdl=1.0)
    b = ops.frame_losses_ext(pred, target, "charbonnier", _weights(shape), eps=EPS, gdl=1.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float(a[0][1].min()) > 0.0


def test_mse_with_gdl_matches_the_reference_and_the_mse_kernel():
    """--gdl_weight on top of the reference's MSE: the pixel sums and, with G = 0, the gradient are dvg_frame_losses's."""
    from dvg_amd import ops
    shape = CASES["e"]
    pred, target = ref.noisy_case(9, *shape)
    w = _weights(shape)
    S, K = shape[:2]
    sums, dpred = ops.frame_losses_ext(pred.to(DEV), target.to(DEV), "mse", w, gdl=1.0)
    pix, gdl = ref.sums(pred, target, "mse")
    assert rel_err_elem(sums, torch.stack([pix, gdl])) < 1e-6
    old_sums, old_dpred = ops.frame_losses(pred.to(DEV).view(S, K, -1), target.to(DEV).view(S, -1), w)
    assert rel_err_elem(sums[0], old_sums) < 1e-6
    sums0, dpred0 = ops.frame_losses_ext(pred.to(DEV), target.to(DEV), "mse", w, gdl=0.0)
    assert torch.equal(dpred0.view_as(old_dpred), old_dpred) and float(sums0[1].abs().max()) == 0.0


def test_bad_arguments_return_their_code_and_launch_nothing():
    from dvg_amd import _lib
    lib = _lib.lib()
    pred, target = ref.noisy_case(1, 1, 1, 1, 4, 8)
    pred, target = pred.to(DEV), target.to(DEV)
    sums = torch.full((2, 3), -7.0, device=DEV)
    dpred = torch.full((1, 4, 1, 4, 8), -7.0, device=DEV)
    w = torch.ones(2, 4, device=DEV)
    part = torch.full((64,), -7.0, device=DEV)

    def call(p=None, S=1, K=1, planes=1, H=4, W=8):
        return lib.dvg_frame_losses_ext(p or pred.data_ptr(), target.data_ptr(), sums.data_ptr(), dpred.data_ptr(), S, K, planes, H, W,
                                        1, EPS, w[0].data_ptr(), w[1].data_ptr(), part.data_ptr(), None)
    assert call(W=6) == 1                                    # DVG_ERR_SHAPE
    assert call(K=4) == 1
    assert call(p=ctypes.c_void_p(pred.data_ptr() + 4)) == 4     # DVG_ERR_ALIGN
    torch.cuda.synchronize()
    assert float(sums.max()) == -7.0 and float(dpred.max()) == -7.0 and float(part.max()) == -7.0
    assert call() == 0                                       # the same buffers, a served shape: it does launch
    torch.cuda.synchronize()
    assert float(sums[0, 0]) > 0.0


# ---- the Trainer ---------------------------------------------------------------------------------------------------------------------
L1_GDL = ["--frame_loss", "l1", "--gdl_weight", "1"]


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


def test_trainer_builds_a_spec_only_when_asked():
    plain = train_harness.trainer()
    assert plain.frame_loss is None and plain.frame_terms is None
    tr = train_harness.trainer(L1_GDL)
    assert tr.frame_loss.label() == "l1 + 1 gdl" and float(tr.frame_terms.acc.abs().max()) == 0.0
    assert tr.frame_terms.epoch_line() == "     frame loss: l1 + 1 gdl   pixel 0  gdl 0"
    from dvg_amd import graphs
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="capture"):
        with graphs.capturing():
            tr.frame_terms.epoch_line()


def test_the_default_flags_change_no_bit(batches):
    """--frame_loss mse --gdl_weight 0 is the run without the flags: the same code path, loss and parameters bit-equal."""
    res = []
    for extra in ([], ["--frame_loss", "mse", "--gdl_weight", "0"]):
        tr = train_harness.trainer(extra)
        assert tr.frame_loss is None
        loss, _ = _one_train_model(tr, batches[0])
        res.append((loss, tr.arena.p.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])


def test_fused_losses_match_the_torch_composition(batches):
    """--frame_loss l1 --gdl_weight 1, one train_model from the same initial state with fused_losses True (dvg_frame_losses_ext)
    against False (torch_terms + a scalar autograd graph).  The forward pass is the same launches on the same bits, so only the
    loss arithmetic differs.  Bars: tests/test_gpu_train.py::test_time_batched_encoder_matches_the_per_frame_path's for its
    path-against-path comparison - the closure value `abs(u - v) <= 1e-4 * max(1.0, abs(u))` (its line 513) and per optimiser
    range of the gradient arena `d <= 2e-3 * na` for dcgan (lines 526-527)."""
    res, stats = [], []
    for fused in (True, False):
        tr = train_harness.trainer(L1_GDL)
        tr.fused_losses = fused
        res.append(_one_train_model(tr, batches[0]))
        stats.append(tr.frame_terms.read_and_reset())
    (la, ga), (lb, gb) = res
    print(f"\nfused {la!r} torch {lb!r}  stats {stats}")
    assert abs(la - lb) <= 1e-4 * max(1.0, abs(la)), (la, lb)
    _compare_ranges(tr, ga, gb, 2e-3)
    assert stats[0]["iterations"] == stats[1]["iterations"] == 1
    for k in ("pixel", "gdl"):                               # the same sums by two fp32 summation orders: the value bar above
        assert stats[0][k] > 0 and abs(stats[0][k] - stats[1][k]) <= 1e-4 * stats[0][k], (k, stats)


def test_step_by_step_path_matches_the_batched_one(batches):
    """time_batched False (one decoder call per step, torch_terms per call) against the batched path (dvg_frame_losses_ext).
    --frame_loss charbonnier is smooth, so the gradients are comparable: the bars test_time_batched_encoder_matches_the_per_frame_path
    applies to this pair under MSE (value 1e-4, its line 513; gradient ranges 2e-3 for dcgan, lines 526-527).  Under l1 + gdl a
    last-bit difference of the two forward passes may flip a sign: the value only."""
    res = []
    for tb in (False, True):
        tr = train_harness.trainer(["--frame_loss", "charbonnier"])
        tr.time_batched = tb
        res.append(_one_train_model(tr, batches[0]))
    (la, ga), (lb, gb) = res
    print(f"\ncharbonnier: step by step {la!r} batched {lb!r}")
    assert abs(la - lb) <= 1e-4 * max(1.0, abs(la)), (la, lb)
    _compare_ranges(tr, ga, gb, 2e-3)
    vals = []
    for tb in (False, True):
        tr = train_harness.trainer(L1_GDL)
        tr.time_batched = tb
        vals.append(_one_train_model(tr, batches[0])[0])
    print(f"l1 + gdl: step by step {vals[0]!r} batched {vals[1]!r}")
    assert abs(vals[0] - vals[1]) <= 1e-4 * max(1.0, abs(vals[0])), vals


def test_graph_replay_matches_eager_with_the_flags_on(batches):
    """GraphedIteration under --frame_loss l1 --gdl_weight 1: two eager warm-up iterations, then three replays of one captured
    hipGraph, against five eager iterations - within the bars of test_one_capture_serves_a_multiplier_that_moves_every_iteration
    (tests/test_gpu_lr_schedule.py) and of the EMA graph test: values 2e-4, parameters / buffers / moments rtol 2e-3 atol 2e-5.
    The epoch line's device sums advance inside the replayed graph: the counts are equal and the means agree like the values."""
    res = []
    for graphed in (False, True):
        tr = train_harness.trainer(L1_GDL, seed=11)
        step, out = train_harness.iterate(tr, batches[:5], graphed, warmup=2,
                                          each=lambda tr, step, i: (tr.last_loss, step.graph if graphed else None))
        out = [(r + (loss,), graph) for r, (loss, graph) in out]
        if graphed:
            assert not step.failed and out[2][1] is not None and all(g is out[2][1] for _, g in out[2:])
            assert out[0][1] is None and out[1][1] is None and step.calls == 5
        res.append(([o[0] for o in out], [{k: t.detach().clone() for k, t in m.state_dict().items()} for m in tr.modules],
                    {n: getattr(tr.arena, n).clone() for n in ("m", "v")}, tr.frame_terms.acc.tolist(),
                    tr.frame_terms.epoch_line()))
    (la, sa, aa, ca, linea), (lb, sb, ab, cb, lineb) = res
    print(f"\neager  {linea}\ngraph  {lineb}")
    for a, b in zip(la, lb):
        for u, v in zip(a, b):
            assert abs(u - v) <= 2e-4 * max(1.0, abs(u)), (la, lb)
    for a, b in zip(sa, sb):
        for k in a:
            assert torch.allclose(a[k].float(), b[k].float(), rtol=2e-3, atol=2e-5), k
    for n in ("m", "v"):
        assert torch.allclose(aa[n], ab[n], rtol=2e-3, atol=2e-5), n
    assert ca[2] == cb[2] == 5.0 and ca[3] == cb[3] == 5.0 * 3 * 4 * 64 * 64      # iterations; pixels of the x_pred calls
    assert ca[0] > 0 and ca[1] > 0
    assert abs(ca[0] - cb[0]) <= 2e-4 * ca[0] and abs(ca[1] - cb[1]) <= 2e-4 * ca[1], (ca, cb)
    assert linea.startswith("     frame loss: l1 + 1 gdl   pixel ")
