"""CPU: the host side of train.py --ssim_weight - the fp64 reference (tests/ssim_loss_ref.py) against finn_ref, fp64 autograd and central
differences; the bars of tests/test_gpu_ssim_loss.py shown to catch every planted defect; the option, the spec and the epoch line;
torch_ssim_sum in fp32 against fp64 (the figures the Trainer tolerances of the GPU file cite); the entry points' host-side checks."""
import ctypes
import os

import pytest
import torch

from tests import finn_ref, ssim_loss_ref as ref
from tests.common import rel_err, rel_err_elem

GPU_BAR = 1e-6          # tests/test_gpu_ssim_loss.py: rel_err_elem on the sums, rel_err on dpred


def _parse(argv):
    import train
    return train.build_parser().parse_args(list(argv))


def _weights(shape):
    S, K, planes, H, W = shape
    m = planes * (H - 10) * (W - 10)
    return [1.0 / m, 0.5 / m, 2.0 / m][:K]


# ---- the reference -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noise_11x11", "noise_12x17", "noise_64_c3", "sparse_12x17", "sparse_64_c3", "const_11x11",
                                  "const_64_c3", "signed_12x17_c3"])
def test_the_value_is_finn_refs(name):
    """1 - sums / positions against finn_ref.per_channel on finn_ref's own cases, for the closed form (separable filters) and for
    torch_ssim_sum in fp64: 1e-10, the bar reference_finn.npz pins finn_ref to the reference's finn_ssim with."""
    from dvg_amd import frame_loss
    gt, pred = finn_ref.case(name)
    want = finn_ref.per_channel(gt, pred)[0]                                 # (N, C) map means
    N, C, H, W = gt.shape
    p, t = torch.from_numpy(pred).view(N, 1, C, H, W), torch.from_numpy(gt)
    pos = (H - 10) * (W - 10)
    worst = 0.0
    for n in range(N):
        for c in range(C):
            one_p, one_t = p[n:n + 1, :, c:c + 1], t[n:n + 1, c:c + 1]
            got = [1.0 - float(ref.sums(one_p, one_t)[0]) / pos, 1.0 - float(ref.formula(one_p, one_t, [1.0])[0][0]) / pos,
                   1.0 - float(frame_loss.torch_ssim_sum(one_p[:, 0].double(), one_t.double())) / pos]
            worst = max(worst, max(abs(g - want[n, c]) for g in got))
    print(f"\n{name}: |mean SSIM - finn_ref.per_channel| {worst:.2e}")
    assert worst < 1e-10


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("shape", [(1, 1, 1, 11, 12), (2, 3, 1, 12, 16), (1, 2, 3, 21, 20), (1, 1, 2, 64, 64)])
def test_the_formula_gradient_is_fp64_autograds(kind, shape):
    """The closed form against autograd of the slice composition, both fp64: 1e-10 of the largest gradient entry (absolute 1e-10 per
    unit weight on identical images, whose gradient is 0 up to rounding)."""
    pred, target = ref.case(kind, 1, *shape)
    w = _weights(shape)
    s_f, g_f = ref.formula(pred, target, w)
    s_a, g_a = ref.autograd(pred, target, w)
    scale = max(float(g_a.abs().max()), max(w)) if kind == "identical" else float(g_a.abs().max())
    gap = float((g_f - g_a).abs().max()) / scale
    print(f"\n{kind} {shape}: formula against autograd {gap:.2e} of max |gradient| {float(g_a.abs().max()):.2e}")
    assert gap < 1e-10
    assert rel_err_elem(s_f, s_a) < 1e-10 or float(s_a.abs().max()) < 1e-10
    assert rel_err_elem(s_f, ref.sums(pred, target)) < 1e-10 or kind == "identical"
    if kind == "identical":
        assert float(ref.sums(pred, target).abs().max()) < 1e-12


@pytest.mark.parametrize("shape", [(1, 1, 1, 11, 12), (1, 2, 1, 12, 16)])
def test_the_formula_gradient_agrees_with_central_differences(shape):
    """(f(P + h) - f(P - h)) / 2h with h = 1e-5 in fp64 on noise: the rounding error is ~1e-16 |f| / h = 1e-11 for f of order 1, the
    truncation error h^2 |f'''| / 6 = 2e-11 |f'''| with third derivatives bounded by a few 1 / C2 = 1.1e3 times the 1 / positions
    weights: 1e-6 of the largest gradient entry leaves two orders of magnitude, and the planted defects below move it by > 1e-4."""
    pred, target = ref.case("noise", 2, *shape)
    gap = ref.central_difference_gap(pred, target, _weights(shape))
    print(f"\n{shape}: formula against central differences {gap:.2e}")
    assert gap < 1e-6, gap


@pytest.mark.parametrize("shape", [(1, 1, 1, 11, 12), (2, 3, 1, 12, 16), (1, 2, 3, 21, 20), (1, 3, 2, 64, 64)])
def test_the_gpu_bars_catch_every_planted_defect(shape):
    """Each defect of ssim_loss_ref.DEFECTS misses the GPU file's bar on dpred by more than 100 x on the noise inputs of its shapes."""
    pred, target = ref.case("noise", 3, *shape)
    w = _weights(shape)
    good = ref.gradient(pred, target, w)
    for defect in ref.DEFECTS:
        bad = ref.formula(pred, target, w, defect=defect)[1]
        miss = rel_err(bad, good)
        print(f"{shape} {defect}: rel_err {miss:.2e}")
        assert miss > 100 * GPU_BAR, (defect, miss)


def test_fp32_arithmetic_would_miss_the_gpu_bars_on_constant_images():
    """Why the kernel is fp64 inside: the closed form evaluated in fp32 (torch_ssim_sum's autograd) against fp64 on const."""
    from dvg_amd import frame_loss
    shape = (1, 1, 1, 64, 64)
    pred, target = ref.case("const", 4, *shape)
    p = pred.clone().requires_grad_(True)
    frame_loss.torch_ssim_sum(p[:, 0], target).backward()
    good = ref.gradient(pred, target, [1.0])
    miss = rel_err(p.grad, good)
    print(f"\nfp32 autograd against fp64 on const 64x64: {miss:.2e}")
    assert miss > 10 * GPU_BAR


# ---- torch_ssim_sum ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "sparse", "const"])
def test_torch_ssim_sum_in_fp32_against_fp64(kind):
    """The fp32 composition (what the unfused and step-by-step Trainer paths run) against the fp64 reference, on the Trainer tests'
    frame size.  Prints the figures tests/test_gpu_ssim_loss.py's Trainer tolerances cite; asserts only what fp32 guarantees on
    every kind: the value to 1e-3 of the positions (the variances' cancellation against C2 on flat windows costs ~1e-4)."""
    from dvg_amd import frame_loss
    shape = (2, 3, 4, 64, 64)
    pred, target = ref.case(kind, 5, *shape)
    w = _weights(shape)
    p = pred.clone().requires_grad_(True)
    terms = [frame_loss.torch_ssim_sum(p[:, k], target) for k in range(3)]
    sum(wk * v for wk, v in zip(w, terms)).backward()
    s_ref, g_ref = ref.formula(pred, target, w)
    pos = 2 * 4 * 54 * 54
    e_val = float((torch.stack(terms).detach().double() - s_ref).abs().max()) / pos
    e_grad = rel_err(p.grad, g_ref)
    print(f"\ntorch_ssim_sum fp32 against fp64, {kind}: |mean SSIM error| {e_val:.2e}  gradient rel_err {e_grad:.2e}")
    assert e_val < 1e-3 and bool(torch.isfinite(p.grad).all())


def test_torch_ssim_sum_broadcasts_and_refuses_small_frames():
    from dvg_amd import frame_loss
    pred, target = ref.case("noise", 6, 2, 1, 3, 12, 16)
    a = frame_loss.torch_ssim_sum(pred[:, 0].double(), target.double())
    b = frame_loss.torch_ssim_sum(pred.double(), target.double()[:, None])
    assert abs(float(a) - float(b)) < 1e-12
    with pytest.raises(ValueError, match="11x11"):
        frame_loss.ssim_positions((4, 1, 10, 16))
    assert frame_loss.ssim_positions((4, 2, 64, 64)) == 4 * 2 * 54 * 54


# ---- options -------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_capture(monkeypatch):
    """FrameTerms asks torch whether a capture is under way, which needs a device: here there is none, and no capture."""
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)


def test_make_returns_none_only_at_all_default_values():
    import argparse
    from dvg_amd import frame_loss as F
    o = _parse([])
    assert o.ssim_weight == 0.0 and F.make(o) is None
    assert F.make(_parse(["--ssim_weight", "0"])) is None and F.make(argparse.Namespace()) is None
    assert F.make(_parse(["--frame_loss", "mse", "--gdl_weight", "0", "--ssim_weight", "0.0"])) is None
    s = F.make(_parse(["--ssim_weight", "0.2"]))
    assert (s.kind, s.gdl, s.ssim, s.label()) == ("mse", 0.0, 0.2, "mse + 0.2 ssim")
    s = F.make(_parse(["--frame_loss", "l1", "--ssim_weight", "0.2"]))
    assert (s.kind, s.kind_id, s.ssim, s.label()) == ("l1", 1, 0.2, "l1 + 0.2 ssim")
    s = F.make(_parse(["--frame_loss", "l1", "--gdl_weight", "1", "--ssim_weight", "0.5"]))
    assert s.label() == "l1 + 1 gdl + 0.5 ssim"
    assert F.make(_parse(["--gdl_weight", "1"])).ssim == 0.0
    assert F.KINDS == ("mse", "l1", "charbonnier")


@pytest.mark.parametrize("argv,says", [
    (["--ssim_weight", "-0.5"], "must be a finite number >= 0"), (["--ssim_weight", "inf"], "must be a finite number >= 0"),
    (["--ssim_weight", "nan"], "must be a finite number >= 0"), (["--ssim_weight", ""], "is not a number"),
    (["--ssim_weight", "x"], "is not a number")])
def test_bad_values_end_with_one_argparse_line(argv, says, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(argv)
    assert e.value.code == 2
    err = [line for line in capsys.readouterr().err.splitlines() if "error:" in line]
    assert len(err) == 1 and "--ssim_weight" in err[0] and says in err[0] and "unrecognized" not in err[0], err


def test_a_spec_refuses_what_the_parser_refuses():
    from dvg_amd import frame_loss as F
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="ssim"):
            F.FrameLossSpec("l1", 1e-3, 0.0, bad)
    assert F.FrameLossSpec("l1", 1e-3, 1.0).ssim == 0.0            # the three-argument form of before


def test_label_and_epoch_line_without_ssim_are_what_they_were(no_capture):
    """W_s = 0: the label and the epoch line are character-equal to the ones before the option existed (the strings below are
    tests/test_gpu_frame_loss.py's), there is no fifth sum, and `acc` keeps its four elements with W_s > 0 too."""
    from dvg_amd import frame_loss as F
    t = F.FrameTerms(F.FrameLossSpec("l1", 1e-3, 1.0), "cpu")
    assert t.spec.label() == "l1 + 1 gdl" and t.acc_ssim is None and t.acc.shape == (4,)
    assert t.epoch_line() == "     frame loss: l1 + 1 gdl   pixel 0  gdl 0"
    assert F.FrameLossSpec("charbonnier", 0.01).label() == "charbonnier" and F.FrameLossSpec("mse", 1e-3, 0.25).label() == "mse + 0.25 gdl"
    assert repr(F.FrameLossSpec("l1", 1e-3, 1.0)) == "FrameLossSpec('l1', eps=0.001, gdl=1.0)"
    t.add(torch.tensor(8.0), torch.tensor(2.0), 16)
    assert t.epoch_line() == "     frame loss: l1 + 1 gdl   pixel 0.5  gdl 0.125"
    s = F.FrameTerms(F.FrameLossSpec("l1", 1e-3, 0.0, 0.2), "cpu")
    assert s.acc.shape == (4,) and s.acc_ssim.shape == (2,)
    assert s.epoch_line() == "     frame loss: l1 + 0.2 ssim   pixel 0  gdl 0  ssim 1"
    s.add(torch.tensor(8.0), torch.tensor(0.0), 16)
    s.add_ssim(torch.tensor(3.0), 12)
    s.add_ssim(torch.tensor(0.0), 12)
    assert s.acc.tolist() == [8.0, 0.0, 1.0, 16.0] and s.acc_ssim.tolist() == [3.0, 24.0]
    assert s.epoch_line() == "     frame loss: l1 + 0.2 ssim   pixel 0.5  gdl 0  ssim 0.875"
    assert s.acc_ssim.tolist() == [0.0, 0.0]


def test_the_torch_terms_add_w_s_times_the_mean_dssim(no_capture):
    """FrameTerms.torch_calls and torch_step in fp64 on the CPU against the reference: term_k = pix / n + W_s dssim_k / m."""
    from dvg_amd import frame_loss as F
    S, K, B, C, H, W = 2, 3, 2, 1, 12, 16
    pred, target = ref.case("noise", 8, S, K, B * C, H, W)
    calls, tgt = pred.double().view(S, K, B, C, H, W), target.double().view(S, B, C, H, W)
    n, m = B * C * H * W, B * C * 2 * 6
    dssim = ref.sums(pred, target)
    want = [float((calls[:, k] - tgt).abs().sum()) / n + 0.2 * float(dssim[k]) / m for k in range(K)]
    t = F.FrameTerms(F.FrameLossSpec("l1", 1e-3, 0.0, 0.2), "cpu")
    got = t.torch_calls(calls, tgt)
    assert max(abs(float(g) - w) for g, w in zip(got, want)) < 1e-12
    assert abs(t.read_and_reset()["ssim"] - float(ref.mean_ssim(pred, target)[0])) < 1e-12
    run = (0.0, 0.0, 0.0)
    for s in range(S):
        run = t.torch_step(run, [calls[s, k] for k in range(K)], tgt[s])
    assert max(abs(float(g) - w) for g, w in zip(run, want)) < 1e-12
    d = t.read_and_reset()
    assert d["iterations"] == S and abs(d["ssim"] - float(ref.mean_ssim(pred, target)[0])) < 1e-12


def test_the_flag_is_no_part_of_the_resume_fingerprint():
    from dvg_amd import train_state
    assert "ssim_weight" not in train_state.OPTION_FIELDS

    def opt(extra):
        o = _parse(["--model", "dcgan", "--batch_size", "4"] + extra)
        o.ft, o.world = not o.no_ft, 1
        return o
    assert train_state.option_fingerprint(opt([])) == train_state.option_fingerprint(opt(["--frame_loss", "l1", "--ssim_weight", "0.2"]))


# ---- the entry points ----------------------------------------------------------------------------------------------------------------
def test_blocks_are_a_function_of_the_shapes_alone():
    """One workgroup per image while 5 (H - 10) + 3 min(H, 16) fp64 rows of W - 10 fit 150 KiB, else bands (12 rows at W = 128)."""
    from dvg_amd import _lib
    blocks = _lib.lib().dvg_frame_ssim_loss_blocks
    assert blocks(19, 64, 64, 64) == 19 * 64 and blocks(1, 1, 11, 12) == 1 and blocks(2, 3, 31, 16) == 6
    assert blocks(1, 1, 128, 128) == 11 and blocks(1, 1, 37, 128) == 4 and blocks(1, 1, 36, 128) == 3 and blocks(1, 1, 33, 128) == 3
    assert blocks(1, 1, 32, 128) == 1
    for H, W in ((10, 12), (10, 16), (12, 10), (12, 18), (11, 11), (0, 16), (16, 0)):
        assert blocks(1, 1, H, W) <= 0, (H, W)
    assert blocks(0, 1, 16, 16) <= 0 and blocks(1, 0, 16, 16) <= 0
    assert blocks(1, 1, 16, 228) > 0 and blocks(1, 1, 16, 2048) <= 0      # 11 strip rows + 11 map rows of a row must fit
    assert blocks(2 ** 20, 2 ** 20, 16, 16) <= 0


def test_argument_checks_fire_before_any_launch():
    """Fake pointers that are never dereferenced: every call must fail in the checks, with the header's error codes."""
    from dvg_amd import _lib
    lib = _lib.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)

    def call(pred=one, target=one, sums=one, dpred=one, S=1, K=1, planes=1, H=12, W=16, w=one, acc=0, part=one):
        return lib.dvg_frame_ssim_loss(pred, target, sums, dpred, S, K, planes, H, W, w, acc, part, None)
    assert call(H=10) == 1 and b"11" in lib.dvg_last_error()
    assert call(H=10, W=12) == 1 and call(W=18) == 1 and call(W=8) == 1 and call(K=4) == 1 and call(K=0) == 1
    assert call(S=0) == 1 and call(planes=0) == 1 and call(W=2048) == 1
    assert call(S=2 ** 10, planes=2 ** 10, H=64, W=64) == 1 and b"32-bit" in lib.dvg_last_error()
    for name in ("pred", "target", "sums", "dpred", "w", "part"):
        assert call(**{name: None}) == 2, name
    for name in ("pred", "target", "dpred"):
        assert call(**{name: odd}) == 4, name
    with pytest.raises(RuntimeError, match="alignment"):
        _lib.check(call(pred=odd), "frame_ssim_loss")


def test_the_wrapper_has_no_cpu_fallback():
    from dvg_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_ssim_loss(torch.zeros(1, 1, 1, 12, 16), torch.zeros(1, 1, 12, 16), [1.0])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "ssim_loss.hip" in open(os.path.join(root, "dvg_amd", "csrc", "Makefile")).read().split("SRCS")[1].splitlines()[0]
