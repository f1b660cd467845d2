"""CPU: the Finn-style metrics (utils.finn_eval_seq, utils.py:236-301) off the device - the fp64 restatement of
tests/finn_ref.py against the reference's own outputs (tests/golden/reference_finn.npz), dvg_eval_frames_finn's host-side
checks, the two command lines' --metrics flag, and the "no CPU fallback" rule."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import finn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden_finn():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_finn.npz"))


def test_golden_file_holds_every_case_and_nothing_else(golden_finn):
    assert sorted(golden_finn.files) == sorted(f"{n}/{k}" for n in finn_ref.CASES for k in ("ssim", "psnr", "mse"))


@pytest.mark.parametrize("name", sorted(finn_ref.CASES))
def test_restatement_matches_the_reference_outputs(name, golden_finn):
    """Direct fp64 window sums against the reference's fftconvolve: 1e-10 (observed agreement of the two forms: 2.5e-13 on
    the constant images, <= 5e-15 elsewhere)."""
    gt, pred = finn_ref.case(name)
    ssim, psnr, mse = finn_ref.per_channel(gt, pred)
    for k, v in (("ssim", ssim), ("psnr", psnr), ("mse", mse)):
        ref = golden_finn[f"{name}/{k}"]
        assert ref.shape == v.shape and np.isfinite(ref).all(), (name, k)
        print(f"{name}/{k}: max |restatement - reference| = {np.abs(v - ref).max():.3e}")
        np.testing.assert_allclose(v, ref, rtol=0, atol=1e-10)


def test_window_is_the_outer_product_of_the_normalised_1d_gaussian():
    i = np.arange(11) - 5.0
    g1 = np.exp(-i * i / (2 * 1.5 ** 2))
    g1 /= g1.sum()
    np.testing.assert_allclose(finn_ref.window(), np.outer(g1, g1), rtol=1e-14)
    assert abs(finn_ref.window().sum() - 1.0) < 1e-15


def test_assembly_counts_a_nan_map_mean_as_minus_one():
    s, p = finn_ref.assemble(np.array([[0.5, np.nan, 0.9], [0.25, 0.5, 0.75]]), np.array([[10.0, 20.0, 30.0], [1.0, 2.0, 3.0]]))
    np.testing.assert_allclose(s, [(0.5 - 1 + 0.9) / 3, 0.5])
    np.testing.assert_allclose(p, [20.0, 2.0])


def test_host_side_checks_reject_bad_arguments_without_gpu():
    from dvg_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(16)  # fake, never dereferenced: the call must fail in the checks
    rc = lib.dvg_eval_frames_finn(one, one, one, one, one, 4, 1, 10, 64, None)
    assert rc == 1 and b"11x11" in lib.dvg_last_error(), lib.dvg_last_error()
    rc = lib.dvg_eval_frames_finn(one, one, one, one, one, 4, 1, 64, 10, None)
    assert rc == 1 and b"11x11" in lib.dvg_last_error(), lib.dvg_last_error()
    for null in (2, 3, 4):      # ssim, psnr, mse
        args = [one] * 5
        args[null] = None
        rc = lib.dvg_eval_frames_finn(*args, 4, 1, 64, 64, None)
        assert rc != 0 and b"NULL" in lib.dvg_last_error(), (null, lib.dvg_last_error())
    for null in (0, 1):
        args = [one] * 5
        args[null] = None
        assert lib.dvg_eval_frames_finn(*args, 4, 1, 64, 64, None) != 0
    # 32-bit offsets, the LDS strip, empty batches
    assert lib.dvg_eval_frames_finn(one, one, one, one, one, 70000, 3, 128, 128, None) == 1 and b"32-bit" in lib.dvg_last_error()
    assert lib.dvg_eval_frames_finn(one, one, one, one, one, 1, 1, 64, 400, None) == 1 and b"LDS" in lib.dvg_last_error()
    assert lib.dvg_eval_frames_finn(one, one, one, one, one, 0, 1, 64, 64, None) == 1
    assert lib.dvg_eval_frames_finn(one, one, one, one, one, 1, 0, 64, 64, None) == 1
    with pytest.raises(RuntimeError):
        _lib.check(1, "dvg_eval_frames_finn")


def _bench_tool():
    spec = importlib.util.spec_from_file_location("bench_make_gifs", os.path.join(ROOT, "tools", "bench_make_gifs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("which", ["generate_frames", "bench_make_gifs"])
def test_metrics_flag(which, capsys):
    if which == "generate_frames":
        import generate_frames
        parser = generate_frames.build_parser()
    else:
        parser = _bench_tool().build_parser()
    assert parser.parse_args([]).metrics == "skimage"
    assert parser.parse_args(["--metrics", "skimage"]).metrics == "skimage"
    assert parser.parse_args(["--metrics", "finn"]).metrics == "finn"
    with pytest.raises(SystemExit) as e:
        parser.parse_args(["--metrics", "ms-ssim"])
    assert e.value.code == 2
    assert "--metrics" in capsys.readouterr().err


def test_finn_eval_seq_has_no_cpu_fallback():
    import utils
    from dvg_amd import ops
    gt = [torch.zeros(2, 1, 16, 16) for _ in range(3)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        utils.finn_eval_seq(gt, gt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.eval_frames_finn(gt[0], gt[0])


def test_sampler_rejects_an_unknown_metric_name():
    from dvg_amd import rollout
    with pytest.raises(ValueError, match="metrics"):
        rollout.GraphedSampler(None, None, None, None, None, None, 2, 17, metrics="ms-ssim")
