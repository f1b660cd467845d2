"""CPU: the host side of train.py --frame_loss / --gdl_weight - the fp64 reference checked against central differences, the
options and the rule that builds a spec, the torch composition against the reference, the resume fingerprint untouched by the
flags, and the two entry points: header, binding table, built library and their argument checks (which fire before any launch)."""
import ctypes
import math

import pytest
import torch

from tests import frame_loss_ref as ref


def _parse(argv):
    import train
    return train.build_parser().parse_args(list(argv))


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def test_the_reference_gradient_agrees_with_central_differences():
    """Charbonnier is smooth: autograd's fp64 gradient against (f(x + h) - f(x - h)) / 2h, h = 1e-6.  The truncation error is
    h^2 f''' / 6 <= 1e-12 / eps^2-scaled curvature and the rounding error ~1e-16 / h = 1e-10 of the objective: 1e-6 of the largest
    gradient entry leaves both two orders of magnitude."""
    pred, target = ref.noisy_case(5, 2, 3, 2, 5, 8)
    n = 2 * 5 * 8
    gap = ref.central_difference_gap(pred, target, [1.0 / n, 0.5 / n, 2.0 / n], eps=1e-2)
    assert gap < 1e-6, gap


def test_the_reference_on_a_case_worked_by_hand():
    """One 2 x 4 plane.  P = [[0, 1, 1, 3], [0, 0, 2, 3]], T = 0: horizontal |dP| = 1 0 2 / 0 2 1, vertical 0 1 1 0."""
    P = torch.tensor([[0.0, 1.0, 1.0, 3.0], [0.0, 0.0, 2.0, 3.0]]).view(1, 1, 1, 2, 4)
    T = torch.zeros(1, 1, 2, 4)
    pix, gdl = ref.sums(P, T, "l1")
    assert float(pix) == 10.0 and float(gdl) == 6.0 + 2.0
    assert float(ref.sums(P, T, "mse")[0]) == 1 + 1 + 9 + 4 + 9
    assert abs(float(ref.sums(P, T, "charbonnier", eps=4.0)[0]) - (3 * 4.0 + 2 * math.sqrt(17) + 2 * 5.0 + math.sqrt(20))) < 1e-12
    g = ref.gradient(P, T, "l1", [1.0], 1.0).view(2, 4)
    # pixel (0, 1): l1 +1; left edge a = +1 -> +1; right edge a = 0: tie with T -> 0; lower edge a = P[1,1] - P[0,1] = -1 -> the
    # subtrahend of an edge with sign(e) sign(a) = -1 gets +1
    assert float(g[0, 1]) == 3.0
    assert float(g[0, 0]) == 0.0 - 1.0 + 0.0          # sign(0) = 0 for the pixel term; minus the right edge; the tied lower edge


# ---- options -------------------------------------------------------------------------------------------------------------------
def test_defaults_build_no_spec():
    from dvg_amd import frame_loss as F
    o = _parse([])
    assert (o.frame_loss, o.charbonnier_eps, o.gdl_weight) == ("mse", 1e-3, 0.0)
    assert F.make(o) is None
    assert F.make(_parse(["--frame_loss", "mse", "--gdl_weight", "0"])) is None
    assert F.make(_parse(["--frame_loss", "mse", "--charbonnier_eps", "0.5"])) is None
    import argparse
    assert F.make(argparse.Namespace()) is None          # an options object from before the flags
    from dvg_amd import ops
    assert F.KINDS is ops.FRAME_LOSS_KINDS and F.KINDS == ref.KINDS


def test_flags_build_a_spec():
    from dvg_amd import frame_loss as F
    s = F.make(_parse(["--frame_loss", "l1", "--gdl_weight", "1"]))
    assert (s.kind, s.kind_id, s.eps, s.gdl, s.label()) == ("l1", 1, 1e-3, 1.0, "l1 + 1 gdl")
    s = F.make(_parse(["--frame_loss", "charbonnier", "--charbonnier_eps", "0.01"]))
    assert (s.kind, s.kind_id, s.eps, s.gdl, s.label()) == ("charbonnier", 2, 0.01, 0.0, "charbonnier")
    s = F.make(_parse(["--gdl_weight", "0.25"]))         # the gradient-difference loss on top of the reference's MSE
    assert (s.kind, s.kind_id, s.gdl, s.label()) == ("mse", 0, 0.25, "mse + 0.25 gdl")


@pytest.mark.parametrize("argv,says", [
    (["--frame_loss", "huber"], "invalid choice"),
    (["--charbonnier_eps", "0"], "must be a finite number > 0"), (["--charbonnier_eps=-1e-3"], "must be a finite number > 0"),
    (["--charbonnier_eps", "nan"], "must be a finite number > 0"), (["--charbonnier_eps", "inf"], "must be a finite number > 0"),
    (["--charbonnier_eps", "x"], "is not a number"),
    (["--gdl_weight", "-0.5"], "must be a finite number >= 0"), (["--gdl_weight", "inf"], "must be a finite number >= 0"),
    (["--gdl_weight", "nan"], "must be a finite number >= 0"), (["--gdl_weight", ""], "is not a number")])
def test_bad_values_end_with_one_argparse_line(argv, says, capsys):
    """The validator's own wording: an unknown flag would also exit with 2 and one error line."""
    with pytest.raises(SystemExit) as e:
        _parse(argv)
    assert e.value.code == 2
    err = [line for line in capsys.readouterr().err.splitlines() if "error:" in line]
    assert len(err) == 1 and argv[0].split("=")[0] in err[0] and says in err[0] and "unrecognized" not in err[0], err


def test_a_spec_refuses_what_the_parser_refuses():
    from dvg_amd import frame_loss as F
    for bad in (("huber", 1e-3, 0.0), ("l1", 0.0, 0.0), ("l1", float("nan"), 0.0), ("l1", 1e-3, -1.0), ("l1", 1e-3, float("inf"))):
        with pytest.raises(ValueError):
            F.FrameLossSpec(*bad)


# ---- torch_terms against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("G", [0.0, 0.5])
def test_torch_terms_against_the_reference(kind, G):
    """fp64 on the CPU, S = 2 steps of K = 3 calls on 3 planes of 5 x 8; plane 1 is constant and equal in prediction and target:
    every edge there is a tie and the pixel difference is 0, so the gradient on it is exactly 0 for every kind."""
    from dvg_amd import frame_loss as F
    S, K, planes, H, W = 2, 3, 3, 5, 8
    pred, target = ref.quantised_case(11, S, K, planes, H, W)
    pred, target = pred.double(), target.double()
    pred[:, :, 1], target[:, 1] = 0.375, 0.375
    n = planes * H * W
    weights = [1.0 / n, 0.5 / n, 2.0 / n]
    spec = F.FrameLossSpec(kind, 1e-3, G)
    p = pred.clone().requires_grad_(True)
    total, got = 0, []
    for k in range(K):
        pix, gdl = F.torch_terms(p[:, k], target, spec)
        got.append((float(pix.detach()), float(gdl.detach())))
        total = total + weights[k] * n * F.term(pix, gdl, spec, n)
    total.backward()
    want_pix, want_gdl = ref.sums(pred, target, kind)
    for k in range(K):
        assert abs(got[k][0] - float(want_pix[k])) <= 1e-13 * float(want_pix[k])
        if G == 0.0:
            assert got[k][1] == 0.0
        else:
            assert abs(got[k][1] - float(want_gdl[k])) <= 1e-13 * float(want_gdl[k])
    want = ref.gradient(pred, target, kind, weights, G)
    assert abs(float(total.detach()) - float(ref.objective(pred, target, kind, weights, G))) <= 1e-13 * float(total.detach())
    assert float((p.grad - want).abs().max()) <= 1e-15 * max(1.0, float(want.abs().max())) + 1e-18
    assert float(p.grad[:, :, 1].abs().max()) == 0.0 and float(want[:, :, 1].abs().max()) == 0.0
    assert float(p.grad.abs().max()) > 0.0
    assert G == 0.0 or ref.tied_fraction(pred, target) > 0.04


def test_torch_terms_on_one_row_has_no_vertical_edge():
    from dvg_amd import frame_loss as F
    pred, target = ref.noisy_case(3, 1, 1, 1, 1, 4)
    pix, gdl = F.torch_terms(pred[:, 0].double(), target.double(), F.FrameLossSpec("l1", 1e-3, 1.0))
    want = ref.sums(pred, target, "l1")
    assert abs(float(pix) - float(want[0])) < 1e-14 and abs(float(gdl) - float(want[1])) < 1e-14 and float(gdl) > 0


# ---- resume ----------------------------------------------------------------------------------------------------------------------
def test_the_flags_are_no_part_of_the_resume_fingerprint():
    """A state saved by an MSE run resumes under --frame_loss l1 --gdl_weight 1: sharpening a trained model is a use."""
    from dvg_amd import train_state
    assert not {"frame_loss", "charbonnier_eps", "gdl_weight"} & set(train_state.OPTION_FIELDS)

    def opt(extra):
        o = _parse(["--model", "dcgan", "--batch_size", "4"] + extra)
        o.ft, o.world = not o.no_ft, 1
        return o
    saved = train_state.option_fingerprint(opt([]))
    now = train_state.option_fingerprint(opt(["--frame_loss", "l1", "--gdl_weight", "1", "--charbonnier_eps", "0.01"]))
    assert saved == now
    train_state.check_fingerprint(saved, now, "train_state.pth")            # does not end the program
    assert "fingerprint" in _help("--frame_loss") and "--resume" in _help("--gdl_weight")


def _help(flag):
    import train
    for a in train.build_parser()._actions:
        if flag in a.option_strings:
            return a.help
    raise AssertionError(flag)


# ---- the entry points ----------------------------------------------------------------------------------------------------------------
def test_blocks_are_a_function_of_the_shapes_alone():
    from dvg_amd import _lib
    blocks = _lib.lib().dvg_frame_losses_ext_blocks
    assert blocks(19, 64, 64, 64) == 19 * 64 * 4          # 16-row bands
    assert blocks(1, 1, 1, 4) == 1 and blocks(2, 5, 17, 12) == 2 * 5 * 2 and blocks(1, 1, 128, 128) == 8
    assert blocks(1, 1, 64, 256) == 8                     # 8-row bands: the staged band must fit in LDS
    assert blocks(1, 1, 4, 6) == 0 and blocks(1, 1, 4, 0) == 0 and blocks(0, 1, 4, 4) == 0 and blocks(1, 1, 0, 4) == 0
    assert blocks(1, 1, 4, 1336) == 0 and blocks(1, 1, 4, 1332) == 4
    assert blocks(2 ** 20, 2 ** 20, 16, 4) == 0           # more workgroups than a grid holds


def test_argument_checks_fire_before_any_launch():
    """Fake pointers that are never dereferenced: every call must fail in the checks, with the header's error codes."""
    from dvg_amd import _lib
    lib = _lib.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)

    def call(pred=one, target=one, sums=one, dpred=one, S=1, K=1, planes=1, H=4, W=4, kind=1, eps=1e-3, wp=one, wg=one, part=one):
        return lib.dvg_frame_losses_ext(pred, target, sums, dpred, S, K, planes, H, W, kind, eps, wp, wg, part, None)
    assert call(W=6) == 1 and b"W" in lib.dvg_last_error()
    assert call(W=0) == 1 and call(H=0) == 1 and call(K=4) == 1 and call(K=0) == 1 and call(S=0) == 1 and call(planes=0) == 1
    assert call(kind=3) == 1 and call(kind=-1) == 1
    assert call(kind=2, eps=0.0) == 1 and call(kind=2, eps=float("nan")) == 1 and call(kind=2, eps=-1.0) == 1
    assert call(W=1336) == 1
    for name in ("pred", "target", "sums", "dpred", "wp", "wg", "part"):
        assert call(**{name: None}) == 2, name
    for name in ("pred", "target", "dpred"):
        assert call(**{name: odd}) == 4, name
    with pytest.raises(RuntimeError, match="alignment"):
        _lib.check(call(pred=odd), "frame_losses_ext")


def test_the_wrapper_has_no_cpu_fallback():
    from dvg_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_losses_ext(torch.zeros(1, 1, 1, 4, 4), torch.zeros(1, 1, 4, 4), "l1", [1.0])
