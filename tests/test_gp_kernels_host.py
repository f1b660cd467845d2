"""CPU: the covariance families of the GP trigger (--gp_kernel).  The torch restatement the GPU tests compare against
(tests/gp_kernel_ref.py) is held to the oracle where the oracle speaks (rbf), the Matern closed forms and the rho table of the
backward kernel to fp64 autograd, and the flag's way through the header codes, both command lines, the resume fingerprint and
the argument checks of the two new entry points (no launch)."""
import ctypes

import pytest
import torch

from oracle import dvg_oracle as orc
from oracle import params
from tests import gp_kernel_ref as ref

MATERN = ("matern12", "matern32", "matern52")


@pytest.mark.parametrize("training", [True, False])
def test_restatement_with_rbf_equals_the_oracle(training):
    B, D, M = 16, 12, 40
    sd, lik = params.gp_state(90, D=D, M=M)
    h = params.normal(91, B, D, scale=0.7).tanh()
    noise = orc.likelihood_noise(lik)
    want = orc.gp_predict(h, sd, training=training, noise=noise)
    got = ref.predict("rbf", h, sd, training, noise=noise)
    for k in want:
        scale = float(want[k].abs().max())
        assert float((got[k] - want[k]).abs().max()) <= 1e-12 * scale, k
    if training:
        tgt = params.normal(92, D, B, scale=0.5)
        a, b = orc.variational_elbo(want, tgt.double(), noise, num_data=B), ref.elbo(got, tgt.double(), noise, num_data=B)
        assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())


def test_prior_init_with_rbf_equals_the_oracle():
    sd, _ = params.gp_state(96, D=12, M=40, trained=False)
    want = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}       # fp64 in, fp64 out: nothing is rounded
    m, ls = ref.prior_init("rbf", dict(want), 1)
    orc.gp_prior_init(want, 1)
    lw = want["variational_strategy.variational_distribution.chol_variational_covar"]
    assert lw.dtype == torch.float64 and float((ls - lw).abs().max()) <= 1e-12 * float(lw.abs().max())
    assert torch.equal(m, want["variational_strategy.variational_distribution.variational_mean"])


@pytest.mark.parametrize("kernel", MATERN)
def test_matern_value_at_zero_is_the_output_scale(kernel):
    s, ell = torch.tensor([0.3, 1.0, 2.5], dtype=torch.float64), torch.tensor([0.2, 1.0, 3.0], dtype=torch.float64)
    assert torch.equal(ref.k_of_d(kernel, torch.zeros(3, dtype=torch.float64), s, ell), s)
    from dvg_amd.models.gp_models import covariance
    k = covariance(kernel, torch.zeros(3, 2, 2, dtype=torch.float64), s, ell)
    assert torch.equal(k, s.view(-1, 1, 1).expand(3, 2, 2))


def test_matern12_is_the_exponential_kernel():
    g = torch.Generator().manual_seed(7)
    d = torch.randn(1000, generator=g, dtype=torch.float64) * 2
    s, ell = torch.tensor(1.7, dtype=torch.float64), torch.tensor(0.6, dtype=torch.float64)
    assert torch.allclose(ref.k_of_d("matern12", d, s, ell), s * torch.exp(-d.abs() / ell), rtol=1e-15, atol=0)


@pytest.mark.parametrize("kernel", ref.KERNELS)
def test_rho_table_equals_autograd_of_k(kernel):
    """rho(d) = (dk/dd) / k - what gp_train_bwd_kernel multiplies K by - against fp64 autograd of k on 1 000 seeded d, and the
    three derivatives the chain rule takes from it: dk/dz = k rho, dk/dell = -(d / ell) k rho, dk/ds = k / s."""
    g = torch.Generator().manual_seed(11)
    d = (torch.randn(1000, generator=g, dtype=torch.float64) * 1.5).requires_grad_(True)
    s = torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
    ell = torch.tensor(0.45, dtype=torch.float64, requires_grad=True)
    k = ref.k_of_d(kernel, d, s, ell)
    dk_dd, = torch.autograd.grad(k.sum(), d, retain_graph=True)
    rho = ref.rho_of_d(kernel, d.detach(), ell.detach())
    scale = float(dk_dd.abs().max())
    assert float((k.detach() * rho - dk_dd).abs().max()) <= 1e-9 * scale
    for j in range(0, 1000, 100):       # the parameter derivatives, entry by entry
        ds, dl = torch.autograd.grad(k[j], (s, ell), retain_graph=True)
        assert abs(float(ds) - float(k[j].detach() / s.detach())) <= 1e-9 * abs(float(ds)) + 1e-300
        want = float((-(d[j] / ell) * k[j] * rho[j]).detach())
        assert abs(float(dl) - want) <= 1e-9 * max(abs(float(dl)), 1e-300)
    assert float(ref.rho_of_d(kernel, torch.zeros(1, dtype=torch.float64), ell.detach())) == 0.0       # sign(0) = 0


def test_layer_covariance_equals_the_restatement():
    """dvg_amd.models.gp_models.covariance (the host-side K_ZZ of the prior initialisation) against the restatement."""
    from dvg_amd.models.gp_models import covariance
    sd, _ = params.gp_state(96, D=5, M=24, trained=False)
    s, ell, _ = [t.double() for t in ref.hypers(sd)]
    z = sd["variational_strategy.inducing_points"].squeeze(-1).double()
    for kernel in ref.KERNELS:
        got = covariance(kernel, z.unsqueeze(-1) - z.unsqueeze(-2), s, ell)
        assert torch.allclose(got, ref.gram(kernel, z, z, s, ell), rtol=1e-14, atol=0), kernel
    with pytest.raises(RuntimeError, match="matern72"):
        covariance("matern72", z.unsqueeze(-1) - z.unsqueeze(-2), s, ell)


def test_header_codes_equal_the_python_names():
    """The codes are baked into the built kernels: literal values here, the header's enum read without the parser, and the names
    the Python side derives from it."""
    import re
    from dvg_amd import _lib, ops
    from tests.common import header_text
    codes = {"rbf": 0, "matern12": 1, "matern32": 2, "matern52": 3}
    assert ops.GP_KERNELS == codes and list(ops.GP_KERNELS) == list(codes) == list(ref.KERNELS)
    assert _lib.ENUMS == {"GP_KERNEL_" + k.upper(): v for k, v in codes.items()}
    assert {k: int(v) for k, v in re.findall(r"DVG_(GP_KERNEL_\w+)\s*=\s*(\d+)", header_text())} == _lib.ENUMS
    assert not set(_lib.ENUMS) & set(_lib.CONSTANTS)
    assert all(ops.gp_kernel_code(k) == v for k, v in codes.items())
    with pytest.raises(RuntimeError, match="foo"):
        ops.gp_kernel_code("foo")
    for name, n in (("dvg_gp_predict", 22), ("dvg_gp_train_bwd", 24)):       # the new entry points: the old arguments + the kind
        old, new = _lib.SIGNATURES[name][1], _lib.SIGNATURES[name + "_cov"][1]
        assert len(old) == n and new == old[:-1] + [ctypes.c_int, ctypes.c_void_p]


@pytest.mark.parametrize("text,offending", [
    ("enum { DVG_A = 0, };", "enum { DVG_A = 0, }"), ("enum dvg_kind { DVG_A = 0 };", "enum dvg_kind { DVG_A = 0 }"),
    ("enum { DVG_A };", "enum { DVG_A }"), ("enum { OTHER = 1 };", "enum { OTHER = 1 }"),
    ("enum { DVG_A = 1, DVG_A = 2 };", "enum { DVG_A = 1, DVG_A = 2 }"), ("#define DVG_A 1\nenum { DVG_A = 1 };", "enum { DVG_A = 1 }"),
    ("enum { DVG_A = 1 << 2 };", "enum { DVG_A = 1 << 2 }")])
def test_parser_reads_enums_and_refuses_what_it_does_not_understand(text, offending):
    from dvg_amd import _lib
    assert _lib.parse_header_enums("int dvg_a(void);\nenum { DVG_X = 0, DVG_Y = 0x10,\n DVG_Z = -1 };") == {"X": 0, "Y": 16, "Z": -1}
    assert _lib.parse_header("enum { DVG_X = 3 };") == ({}, {})        # enumerators are no CONSTANTS
    with pytest.raises(_lib.DvgLibraryError) as e:
        _lib.parse_header(text, "synthetic.h")
    assert offending in str(e.value) and str(e.value).startswith("synthetic.h: ")


def test_flag_parses_in_both_command_lines_and_an_unknown_kernel_is_refused(capsys):
    import argparse
    import generate_frames
    import train
    from dvg_amd.models.gp_models import GPRegressionLayer1
    assert "gp_kernel" not in vars(train.options([]))         # absent means rbf: the options of a run without the flag do not change
    assert generate_frames.build_parser().parse_args([]).gp_kernel == "rbf"
    for kernel in ref.KERNELS:
        assert train.options(["--gp_kernel", kernel]).gp_kernel == kernel
        assert generate_frames.build_parser().parse_args(["--gp_kernel", kernel]).gp_kernel == kernel
        assert GPRegressionLayer1(3, 4, kernel=kernel).kernel == kernel
    for parse in (train.options, generate_frames.build_parser().parse_args):
        with pytest.raises(SystemExit):
            parse(["--gp_kernel", "foo"])
        assert "--gp_kernel" in capsys.readouterr().err
    with pytest.raises(RuntimeError, match="foo"):
        GPRegressionLayer1(3, 4, kernel="foo")
    layer = GPRegressionLayer1(3, 4, kernel="matern32")
    assert GPRegressionLayer1(3, 4).kernel == "rbf" and list(layer.state_dict()) == list(GPRegressionLayer1(3, 4).state_dict())
    opt = argparse.Namespace(model="dcgan", image_width=64, g_dim=90, channels=1, rnn_size=64, predictor_rnn_layers=2, batch_size=4)
    assert list(generate_frames.synthetic_checkpoint(opt)["gp_layer"]) == list(GPRegressionLayer1(90).state_dict())


def test_resume_fingerprint_carries_the_kernel():
    """A state without the field is an `rbf` state: a run without the flag and one with --gp_kernel rbf write the fingerprint
    they always did; a matern52 state and an rbf run refuse each other, naming the field."""
    import train
    from dvg_amd import train_state
    assert train_state.ABSENT_MEANS["gp_kernel"] == "rbf"
    plain = train_state.option_fingerprint(train.options([]))
    assert "gp_kernel" not in plain and plain == train_state.option_fingerprint(train.options(["--gp_kernel", "rbf"]))
    new = train_state.option_fingerprint(train.options(["--gp_kernel", "matern52"]))
    assert new["gp_kernel"] == "matern52" and {k: v for k, v in new.items() if k != "gp_kernel"} == plain
    train_state.check_fingerprint(plain, plain, "<state>")
    train_state.check_fingerprint(new, new, "<state>")
    with pytest.raises(SystemExit, match=r"gp_kernel is 'matern52' in the file and 'rbf' in this run"):
        train_state.check_fingerprint(new, plain, "<state>")
    with pytest.raises(SystemExit, match=r"gp_kernel is 'rbf' in the file and 'matern52' in this run"):
        train_state.check_fingerprint(plain, new, "<state>")
    with pytest.raises(SystemExit, match=r"gp_kernel is 'matern52' in the file and 'matern32' in this run"):
        train_state.check_fingerprint(new, train_state.option_fingerprint(train.options(["--gp_kernel", "matern32"])), "<state>")


def test_new_entry_points_refuse_an_unknown_kind_without_a_device():
    """The argument checks run before anything is launched (as tests/test_abi.py does for the other entry points)."""
    from dvg_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(16)       # never dereferenced
    gp = [one] * 7 + [None, None, one, one, None, None, one]       # h .. lengthscale, noise, eps, mean, var, sample, cov, kl
    assert lib.dvg_gp_predict_cov(*gp, 16, 90, 40, 1, 1e-3, 0, 1, 7, None) == _lib.CONSTANTS["ERR_SHAPE"] == 1
    assert b"kind 7" in lib.dvg_last_error(), lib.dvg_last_error()
    bwd = [one] * 7 + [one, one, one] + [one] * 7
    assert lib.dvg_gp_train_bwd_cov(*bwd, 16, 90, 40, 1e-3, 0, 1, 7, None) == 1
    assert b"kind 7" in lib.dvg_last_error() and b"dvg_gp_train_bwd" in lib.dvg_last_error()
    assert lib.dvg_gp_predict_cov(*gp, 16, 90, 40, 1, 1e-3, 0, 1, -1, None) == 1 and b"kind -1" in lib.dvg_last_error()
    # a known kind passes that check and fails the next one (B = 200 > 128), like the RBF entry point
    assert lib.dvg_gp_predict_cov(*gp, 200, 90, 40, 1, 1e-3, 0, 1, 3, None) == 1 and b"B=200" in lib.dvg_last_error()
