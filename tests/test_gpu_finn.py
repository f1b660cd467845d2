"""GPU: dvg_eval_frames_finn - utils.finn_eval_seq's SSIM (11x11 Gaussian window), PSNR and MSE (utils.py:236-301) - against
the reference's own outputs (tests/golden/reference_finn.npz) where the case is in that file, else against the fp64
restatement tests/finn_ref.py that the file pins; then end to end through rollout.GraphedSampler, generate_frames.Generator
and utils.finn_eval_seq.

Bars (the kernel computes in fp64 and stores fp32): SSIM atol 2e-6 (the bar of the sibling kernel's test), PSNR atol 2e-5 dB
on finite values (half an fp32 ulp below 128 is 3.8e-6), MSE rtol 1e-6 (fp32 output rounding)."""
import os

import numpy as np
import pytest
import torch

from tests import finn_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SSIM_ATOL, PSNR_ATOL, MSE_RTOL = 2e-6, 2e-5, 1e-6


@pytest.fixture(scope="module")
def golden_finn():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_finn.npz"))


def _run(gt, pred):
    from dvg_amd import ops
    out = ops.eval_frames_finn(torch.from_numpy(np.ascontiguousarray(gt)).to(DEV), torch.from_numpy(np.ascontiguousarray(pred)).to(DEV))
    torch.cuda.synchronize()
    return out


def _close(got, ref, what):
    """got: the op's (ssim, psnr, mse) device tensors; ref: the same three as fp64 arrays."""
    for name, g, r in zip(("ssim", "psnr", "mse"), got, ref):
        g = g.cpu().numpy().astype(np.float64)
        assert g.shape == r.shape, (what, name, g.shape, r.shape)
        fin = np.isfinite(r)
        assert np.array_equal(g[~fin], r[~fin], equal_nan=True), (what, name)
        err = np.abs(g[fin] - r[fin])
        if name == "mse":
            err = err / np.abs(r[fin])
        print(f"{what} {name}: max {'rel' if name == 'mse' else 'abs'} err {err.max() if err.size else 0.0:.3e}")
        if name == "ssim":
            np.testing.assert_allclose(g[fin], r[fin], rtol=0, atol=SSIM_ATOL)
        elif name == "psnr":
            np.testing.assert_allclose(g[fin], r[fin], rtol=0, atol=PSNR_ATOL)
        else:
            np.testing.assert_allclose(g[fin], r[fin], rtol=MSE_RTOL, atol=0)


def _golden(golden_finn, name, sl=slice(None)):
    s, p = finn_ref.assemble(golden_finn[name + "/ssim"][sl], golden_finn[name + "/psnr"][sl])
    return s, p, golden_finn[name + "/mse"][sl]


@pytest.mark.parametrize("name", sorted(finn_ref.CASES))
def test_kernel_matches_the_reference_outputs(name, golden_finn):
    """11x11 (one window position), 12x17 (2 x 7 positions, odd width), 64x64 (three strips), 128x128 (the largest LDS strip),
    C = 1 and 3; uniform noise, a textured block on a flat background (sigma^2 ~ 0 windows), two constants, ground truth in
    [-0.5, 0.5] (PSNR keeps data range 1), 130 frames in one call."""
    gt, pred = finn_ref.case(name)
    _close(_run(gt, pred), _golden(golden_finn, name), name)


def test_frame_counts_1_3_130(golden_finn):
    gt, pred = finn_ref.case("noise_16_x130")
    full = _run(gt, pred)
    for n in (1, 3, 130):
        part = _run(gt[:n], pred[:n])
        _close(part, _golden(golden_finn, "noise_16_x130", slice(0, n)), f"{n} frames")
        for a, b in zip(part, full):
            assert torch.equal(a, b[:n]), n


@pytest.mark.parametrize("shape", [(2, 1, 11, 11), (2, 1, 12, 17), (2, 3, 64, 64), (1, 1, 128, 128)])
def test_identical_images_are_exact(shape):
    gt = np.random.RandomState(9300).uniform(-0.5, 1.0, size=shape).astype(np.float32)
    ssim, psnr, mse = _run(gt, gt.copy())
    assert torch.equal(ssim, torch.ones_like(ssim)), ssim
    assert torch.equal(psnr, torch.full_like(psnr, float("inf"))), psnr
    assert torch.equal(mse, torch.zeros_like(mse)), mse


@pytest.mark.parametrize("in_gt", [False, True])
def test_one_nan_pixel_scores_minus_one_and_touches_no_other_frame(in_gt):
    """utils.py:247-248: a NaN map mean counts as -1 (C = 1: the frame's SSIM IS -1)."""
    gt, pred = (a[:3].copy() for a in finn_ref.case("noise_16_x130"))
    clean = _run(gt, pred)
    (gt if in_gt else pred)[1, 0, 5, 7] = np.nan
    ssim, psnr, mse = _run(gt, pred)
    assert float(ssim[1]) == -1.0 and bool(torch.isnan(psnr[1])) and bool(torch.isnan(mse[1]))
    for a, b in zip((ssim, psnr, mse), clean):
        assert torch.equal(a[[0, 2]], b[[0, 2]])


def test_nan_channel_of_three_enters_the_channel_mean_as_minus_one():
    gt, pred = finn_ref.case("signed_12x17_c3")
    pred = pred.copy()
    pred[0, 2, 3, 4] = np.nan
    ssim, psnr, mse = _run(gt, pred)
    s_ref, _, _ = finn_ref.evaluate(gt, pred)
    assert np.isfinite(s_ref).all()
    np.testing.assert_allclose(ssim.cpu().numpy(), s_ref, rtol=0, atol=SSIM_ATOL)
    assert bool(torch.isnan(psnr[0])) and bool(torch.isnan(mse[0]))


def test_stacked_steps_equal_per_step_calls_bit_for_bit(golden_finn):
    from dvg_amd import ops
    names = ["noise_64_c1", "sparse_64_c1", "signed_64_c1"]              # (2,1,64,64) each -> (3,2,1,64,64)
    gt, pred = (np.stack(a) for a in zip(*(finn_ref.case(n) for n in names)))
    got = _run(gt, pred)
    assert all(tuple(v.shape) == (3, 2) for v in got)
    for t, n in enumerate(names):
        step = _run(gt[t], pred[t])
        for a, b in zip(got, step):
            assert torch.equal(a[t], b), (n, t)
        _close(step, _golden(golden_finn, n), n)
    # three channels: (7,6,3,16,16) out of the 130 16x16 frames; the frame's MSE runs over its three channels
    g3, p3 = (a[:126].reshape(7, 6, 3, 16, 16) for a in finn_ref.case("noise_16_x130"))
    got = _run(g3, p3)
    ref = [finn_ref.evaluate(g3[t], p3[t]) for t in range(7)]
    _close(got, tuple(np.stack([r[k] for r in ref]) for k in range(3)), "stack c3")
    for t in range(7):
        for a, b in zip(got, _run(g3[t], p3[t])):
            assert torch.equal(a[t], b), t
    # a non-contiguous view is packed, not misread
    gt_d = torch.from_numpy(gt).to(DEV)
    pr_d = torch.from_numpy(pred).to(DEV)
    for a, b in zip(ops.eval_frames_finn(gt_d.transpose(0, 1), pr_d.transpose(0, 1)), _run(gt, pred)):
        assert torch.equal(a, b.t())


@pytest.mark.parametrize("name", ["noise_64_c3", "sparse_128_c3", "noise_16_x130"])
def test_two_calls_are_bit_identical(name):
    gt, pred = finn_ref.case(name)
    for a, b in zip(_run(gt, pred), _run(gt, pred)):
        assert torch.equal(a, b)


def test_shape_errors():
    from dvg_amd import ops
    a = torch.zeros(2, 1, 10, 64, device=DEV)
    with pytest.raises(RuntimeError, match="11x11"):
        ops.eval_frames_finn(a, a)
    with pytest.raises(RuntimeError, match="shapes"):
        ops.eval_frames_finn(torch.zeros(2, 1, 16, 16, device=DEV), torch.zeros(2, 1, 16, 17, device=DEV))
    with pytest.raises(RuntimeError, match="shapes"):
        ops.eval_frames_finn(torch.zeros(16, 16, device=DEV), torch.zeros(16, 16, device=DEV))


# ---- end to end ------------------------------------------------------------------------------------------------------------------
B, N_PAST, N_EVAL, S = 2, 2, 17, 3          # one GP trigger step (15) inside the rollout


def _generator(inflight, share):
    import generate_frames
    opt = generate_frames.build_parser().parse_args(["--synthetic_ckpt", "--batch_size", str(B), "--model", "dcgan",
                                                     "--n_past", str(N_PAST), "--n_eval", str(N_EVAL),
                                                     "--inflight", str(inflight)] + ([] if share else ["--no_share_prefix"]))
    torch.manual_seed(4100)
    return generate_frames.Generator(opt, generate_frames.synthetic_checkpoint(opt), torch.device(DEV))


@pytest.mark.parametrize("inflight,share", [(0, True), (0, False), (2, True), (2, False)])
def test_make_gifs_with_finn_metrics(inflight, share):
    """dcgan_64, synthetic checkpoint: the frames do not depend on the metric set; the Finn numbers are those of the
    restatement applied to the RETURNED samples (the rollout's own error does not enter); best = argsort(mean SSIM)[-1] on
    the returned SSIM; the default result is what it was; utils.finn_eval_seq returns the op's numbers as (bs, T) arrays."""
    import utils
    from dvg_amd import ops
    from oracle import dvg_oracle as orc
    from oracle import params
    g = _generator(inflight, share)
    x = [params.frames(4110 + t, B, 1, 64).to(DEV) for t in range(N_EVAL)]
    eps = [{15: params.normal(4140 + s, 90, B).to(DEV)} for s in range(S)]
    assert g.opt.metrics == "skimage"
    plain = g.make_gifs(x, S, eps_by_sample=eps)
    g.opt.metrics = "finn"
    finn = g.make_gifs(x, S, eps_by_sample=eps)
    torch.cuda.synchronize()
    if inflight:
        from dvg_amd import rollout
        assert g._sampler.metrics == "finn" and g._sampler.share == bool(share and rollout.SHARE_PREFIX)
    # the default run: no new key, the same tensors as before (its metrics are the sibling kernel's on its own samples)
    assert sorted(plain) == ["best", "posterior", "psnr", "samples", "ssim"]
    for s in range(S):
        for t in range(N_EVAL - N_PAST):
            a, b = ops.eval_frames(x[N_PAST + t], plain["samples"][s, N_PAST + t])
            assert torch.equal(plain["ssim"][:, s, t], a) and torch.equal(plain["psnr"][:, s, t], b), (s, t)
    assert sorted(finn) == ["best", "metrics", "mse", "posterior", "psnr", "samples", "ssim"] and finn["metrics"] == "finn"
    assert torch.equal(plain["samples"], finn["samples"]) and torch.equal(plain["posterior"], finn["posterior"])
    assert not torch.equal(plain["ssim"], finn["ssim"])
    # the Finn numbers against the restatement on the returned samples
    T = N_EVAL - N_PAST
    gt = torch.stack(x[N_PAST:]).cpu().numpy()                                  # (T,B,1,64,64)
    pred = finn["samples"][:, N_PAST:].cpu().numpy()                            # (S,T,B,1,64,64)
    ref = finn_ref.evaluate(np.broadcast_to(gt, pred.shape).reshape(-1, 1, 64, 64), pred.reshape(-1, 1, 64, 64))
    ref = tuple(r.reshape(S, T, B).transpose(2, 0, 1) for r in ref)             # (B,S,T)
    _close((finn["ssim"], finn["psnr"], finn["mse"]), ref, f"make_gifs inflight {inflight} share {share}")
    mine = finn["ssim"].cpu().numpy()
    assert finn["best"].tolist() == orc.best_ssim(mine)
    assert finn["best"].tolist() == [int(i) for i in np.argsort(mine.astype(np.float64).mean(2), axis=1)[:, -1]]
    # utils.finn_eval_seq: the reference's signature and return order
    for s in (0, S - 1):
        out = utils.finn_eval_seq(x[N_PAST:], [finn["samples"][s, t] for t in range(N_PAST, N_EVAL)])
        assert len(out) == 3
        for arr, key in zip(out, ("mse", "ssim", "psnr")):
            assert isinstance(arr, np.ndarray) and arr.shape == (B, T) and arr.dtype.kind == "f"
            assert np.array_equal(arr, finn[key][:, s].cpu().numpy().astype(arr.dtype)), (key, s)
    # back to the default: the sampler is rebuilt for it and gives the default's numbers again
    g.opt.metrics = "skimage"
    again = g.make_gifs(x, S, eps_by_sample=eps)
    assert sorted(again) == sorted(plain) and all(torch.equal(again[k], plain[k]) for k in plain)


def test_sampler_run_wants_the_mse_output_with_finn_only():
    g = _generator(2, True)
    from oracle import params
    x = [params.frames(4110 + t, B, 1, 64).to(DEV) for t in range(N_EVAL)]
    g.opt.metrics = "finn"
    g.make_gifs(x, 1)
    sm = g._sampler
    buf = lambda: torch.zeros(B, 1, N_EVAL - N_PAST, device=DEV)   # noqa: E731
    samples = torch.empty((1, N_EVAL) + tuple(x[0].shape), device=DEV)
    with pytest.raises(ValueError, match="mse"):
        sm.run(1, samples, buf(), buf())
