"""GPU: the sampler's per-row variance trigger (generate_frames.py --trigger variance; docs/DESIGN_NOTES_trigger_rows.md) -
dvg_gp_trigger_rows as a chain of launches against the literal reference arithmetic (tests/trigger_rows_ref.py), the sampler that
uses it (eager against rollout.GraphedSampler, the device against the host loop), and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import trigger_rows_ref as ref
from tests.common import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-5          # values, thresholds, windows: the bar of the existing trigger tests for this arithmetic


def _kernel_cases():
    for c in ref.CASES:
        for n_past in ref.n_pasts(c):
            for coef in ref.COEFS:
                for gap in ref.GAPS:
                    yield pytest.param(c, n_past, coef, gap, id=f"{'x'.join(map(str, c))}-past{n_past}-coef{coef}-gap{gap}")


@pytest.fixture(scope="module")
def inputs():
    """Per case: the variances on the device, the values, a GP sample and an LSTM output per step (what a row decodes)."""
    out = {}
    for c in ref.CASES:
        D, B, W, T = c
        var, values = ref.case(D, B, W, T, ref.SEEDS[c])
        g = torch.Generator().manual_seed(77)
        out[c] = (torch.from_numpy(var).to(DEV), values, torch.randn(T, D, B, generator=g).to(DEV),
                  torch.randn(T, B, D, generator=g).to(DEV))
    return out


@pytest.mark.parametrize("c,n_past,coef,gap", _kernel_cases())
def test_kernel_chain_against_the_reference_arithmetic(inputs, c, n_past, coef, gap):
    from dvg_amd import rollout
    D, B, W, T = c
    var, values, sample, h_pred = inputs[c]
    trig = rollout.VarianceTrigger(W, coef, gap)
    st = trig.new_state(B, T, DEV)
    assert st["win"].shape == (B, W) and st["last"].dtype == torch.int32 and st["flags"].dtype == torch.int32
    assert bool((st["last"] == -(1 << 30)).all()) and bool(torch.isinf(st["thresholds"]).all())
    first = trig.first_decision(n_past)
    vecs = {}
    for i in range(1, T):
        if i < first:
            trig.record(st, i, var[i])
        else:
            vecs[i] = trig.decide(st, i, var[i], sample[i], h_pred[i])
    torch.cuda.synchronize()
    flags, thr, vals = st["flags"].cpu().numpy(), st["thresholds"].cpu().numpy(), st["values"].cpu().numpy()
    f_ref, t_ref, margins, w_ref = ref.decide(values, n_past, W, coef, gap, device_flags=flags)
    assert not vals[0].any() and np.isinf(thr[:first]).all() and not flags[:first].any()
    np.testing.assert_allclose(vals[1:], values[1:], rtol=RTOL, atol=0)
    np.testing.assert_allclose(thr[first:], t_ref[first:], rtol=RTOL, atol=0)
    np.testing.assert_allclose(st["win"].cpu().numpy(), w_ref, rtol=RTOL, atol=0)
    decisions = (T - first) * B
    if W == 1:           # every decision an exact tie, on both sides: no margin rule, no draw (tests/test_trigger_rows_host.py)
        near = 0
        assert np.array_equal(thr[first:], vals[first:])
    else:
        near = int((margins[first:] <= ref.GUARD).sum())
    assert np.array_equal(flags, f_ref), np.argwhere(flags != f_ref)     # inside the guard f_ref follows the device: counted
    print(f"{c} n_past {n_past} coef {coef} gap {gap}: {decisions} decisions, {int(flags.sum())} draws, {near} inside {ref.GUARD:.0e}")
    assert near <= (0.01 * decisions if c == ref.CASES[3] else 0), near
    if coef == -0.5 and W > 1:
        assert 0 < flags.sum() < decisions
    if W == 1 or coef >= (W - 1) ** 0.5:
        assert not flags.any()
    if gap:
        for b in range(B):
            assert (np.diff(np.nonzero(flags[:, b])[0]) > gap).all()
        last = st["last"].cpu().numpy()
        for b in range(B):
            steps = np.nonzero(flags[:, b])[0]
            assert last[b] == (steps[-1] if len(steps) else -(1 << 30))
    for i, vec in vecs.items():       # bit-equal to the GP sample's column or to the LSTM output, by the device's own flag
        want = torch.where(st["flags"][i].bool().unsqueeze(1), sample[i].t(), h_pred[i])
        assert torch.equal(vec, want), i


def test_a_record_only_launch_touches_no_latent():
    """decide = 0 with NULL sample / h_pred / vec: the window, the logs - and nothing else; a poisoned vec next to them stays."""
    from dvg_amd import _lib, ops, rollout
    D, B, W, T = 130, 3, 5, 8
    var, values = ref.case(D, B, W, T, 0)
    var = torch.from_numpy(var).to(DEV)
    st = rollout.VarianceTrigger(W).new_state(B, T, DEV)
    vec = torch.full((B, D), 12345.0, device=DEV)
    for i in range(1, T):
        rc = _lib.lib().dvg_gp_trigger_rows(var[i].data_ptr(), None, None, None, D, B, st["win"].data_ptr(), W, min(i - 1, W), 0,
                                            2.01, i, 0, st["last"].data_ptr(), st["values"].data_ptr(), st["thresholds"].data_ptr(),
                                            st["flags"].data_ptr(), i, None)
        assert rc == 0
    torch.cuda.synchronize()
    assert bool((vec == 12345.0).all()) and bool((st["last"] == ops.TRIGGER_NEVER).all())
    assert bool(torch.isinf(st["thresholds"]).all()) and not bool(st["flags"].any())
    np.testing.assert_allclose(st["values"].cpu().numpy()[1:], values[1:], rtol=RTOL)
    np.testing.assert_allclose(st["win"].cpu().numpy(), values[T - W:].T, rtol=RTOL)
    with pytest.raises(RuntimeError):        # the wrapper's own checks: a deciding step without its latents, a slot past the logs
        ops.gp_trigger_rows(var[1], st["win"], st["last"], st["values"], st["thresholds"], st["flags"], pos=W, step=6, slot=6, decide=True)
    with pytest.raises(RuntimeError):
        ops.gp_trigger_rows(var[1], st["win"], st["last"], st["values"], st["thresholds"], st["flags"], pos=0, step=1, slot=T)


# ---- the sampler ------------------------------------------------------------------------------------------------------------------
B, N_PAST, N_EVAL, W, COEF, S = 4, 2, 9, 3, -0.5, 3
# SEED: of the synthetic checkpoint and the GP's perturbation (_generator).  The case must have at most one decision inside the
# guard and rows that draw at different steps - conditions on the case, asserted below.  Of the seeds 0 .. 31, eight have NO
# decision inside 1e-4 and rows that differ (0, 7, 15, 18, 19, 20, 22, 31); 15 has the widest smallest margin, 9.6e-4.
SEED = 15
RAW_LENGTHSCALE = -2.0     # soft-plus: 0.127


def _generator(inflight, share=True, extra=(), model="dcgan", b=B, n_eval=N_EVAL, window=W):
    """A Generator on a synthetic checkpoint that behaves like a trained one where the rule looks: BatchNorm statistics of the
    data (benchlib.calibrate_batchnorm: with the N(0, 0.02) initialisation's the decoder ignores its latent and a rollout sits
    on one frame from its second step on, every window a tie) and a GP that has left its prior (the recipe of
    tests/test_gpu_gp_score.py: an untrained GP predicts one variance everywhere)."""
    import generate_frames
    argv = ["--synthetic_ckpt", "--batch_size", str(b), "--model", model, "--n_past", str(N_PAST), "--n_eval", str(n_eval),
            "--inflight", str(inflight), "--trigger", "variance", "--trigger_window", str(window), "--trigger_coef", str(COEF)]
    opt = generate_frames.parse_args(argv + ([] if share else ["--no_share_prefix"]) + list(extra))
    torch.manual_seed(SEED)
    torch.cuda.manual_seed_all(SEED)
    gen = generate_frames.Generator(opt, generate_frames.synthetic_checkpoint(opt), torch.device(DEV))
    from dvg_amd import benchlib
    benchlib.calibrate_batchnorm(gen.encoder, gen.decoder, _clip(b, 1)[0])
    with torch.no_grad():
        gen.gp_layer.covar_module.base_kernel.raw_lengthscale.fill_(RAW_LENGTHSCALE)
        gen.gp_layer.variational_strategy.inducing_points.mul_(2.0).sub_(1.0)
        gen.gp_layer.ensure_initialized()
        vd = gen.gp_layer.variational_strategy.variational_distribution
        vd.variational_mean.add_(0.3 * torch.randn_like(vd.variational_mean))
        vd.chol_variational_covar.mul_(torch.rand_like(vd.variational_mean).mul_(0.95).add_(0.05).unsqueeze(-1))
    return gen


def _clip(b=B, n_eval=N_EVAL, c=1):
    from oracle import params
    return [params.frames(7100 + t, b, c, 64).to(DEV) for t in range(n_eval)]


def _eps(b=B, n_eval=N_EVAL, s=S):
    from oracle import params
    return [{i: params.normal(7200 + 100 * k + i, 90, b).to(DEV) for i in range(1, n_eval)} for k in range(s)]


def _same(a, b, keys=("posterior", "samples", "ssim", "psnr", "best")):
    for k in keys:
        assert torch.equal(a[k], b[k]), k
    for k in ("flags", "values", "thresholds"):
        assert torch.equal(a["trigger"][k], b["trigger"][k]), k


@pytest.fixture(scope="module")
def eager():
    return _generator(0).make_gifs(_clip(), S, eps_by_sample=_eps())


def test_sampler_logs_and_rows_that_draw_at_different_steps(eager):
    tr = eager["trigger"]
    assert (tr["window"], tr["coef"], tr["min_gap"]) == (W, COEF, 0)
    assert tr["flags"].shape == (S, N_EVAL, B) and tr["flags"].dtype == torch.int32
    assert tr["values"].shape == tr["thresholds"].shape == (S, N_EVAL, B)
    first = max(N_PAST, W + 1)
    assert not bool(tr["flags"][:, :first].any()) and bool(torch.isinf(tr["thresholds"][:, :first]).all())
    assert bool(torch.isfinite(tr["thresholds"][:, first:]).all()) and bool((tr["values"][:, 1:] > 0).all())
    assert not bool(tr["values"][:, 0].any())
    # the values before the first decision do not depend on the sample; both branches are taken
    assert all(torch.equal(tr["values"][0, :first + 1], tr["values"][s, :first + 1]) for s in range(S))
    flags = tr["flags"].cpu().numpy()
    assert 0 < flags.sum() < S * (N_EVAL - first) * B
    # the point of the rule: rows of ONE sample draw at different steps
    assert any(not np.array_equal(flags[s, :, a], flags[s, :, b]) for s in range(S) for a in range(B) for b in range(a))
    # and the host rule applied to the logged values gives the logged decisions, outside the guard
    for s in range(S):
        f_ref, t_ref, margins, _ = ref.decide(tr["values"][s].cpu().numpy(), N_PAST, W, COEF, 0, device_flags=flags[s])
        assert np.array_equal(f_ref, flags[s])
        np.testing.assert_allclose(tr["thresholds"][s, first:].cpu().numpy(), t_ref[first:], rtol=RTOL)


@pytest.mark.parametrize("inflight,share", [(1, True), (3, True), (1, False), (3, False)])
def test_graphed_sampler_is_the_eager_loop_bit_for_bit(eager, inflight, share):
    g = _generator(inflight, share)
    got = g.make_gifs(_clip(), S, eps_by_sample=_eps())
    if inflight == 1:      # one chain keeps the latency tiles, as the eager loop does: the same bits
        _same(got, eager)
    again = g.make_gifs(_clip(), S, eps_by_sample=_eps())        # a replay starts from the prefix's state, not the last sample's
    _same(again, got)
    if inflight > 1:       # several chains run the energy tiles (fp32 rounding apart from the eager loop): against one chain of them
        from dvg_amd import ops
        with ops.tile_policy(True):
            _same(got, _generator(0, share).make_gifs(_clip(), S, eps_by_sample=_eps()))


def test_device_rule_against_the_host_loop(eager):
    g = _generator(0)
    flags = eager["trigger"]["flags"].cpu().numpy()
    host = g.make_gifs(_clip(), S, eps_by_sample=_eps(), host_loop=True, follow=flags, guard=ref.GUARD)
    followed = host["trigger"]["followed"]
    print(f"host loop: {len(followed)} decisions inside {ref.GUARD:.0e} followed the device: {followed}")
    assert len(followed) <= 1                      # a condition on the seeded case, not a measurement
    assert torch.equal(host["trigger"]["flags"], eager["trigger"]["flags"])
    for k in ("samples", "posterior", "ssim", "psnr", "best"):      # the same kernels on both sides
        assert torch.equal(host[k], eager[k]), k
    for k in ("values", "thresholds"):
        a, b = host["trigger"][k].cpu().numpy(), eager["trigger"][k].cpu().numpy()
        fin = np.isfinite(a)
        assert np.array_equal(fin, np.isfinite(b))
        np.testing.assert_allclose(a[fin], b[fin], rtol=RTOL)


@pytest.mark.parametrize("inflight", [0, 2])
def test_min_gap_keeps_draws_apart(inflight):
    res = _generator(inflight, extra=["--trigger_min_gap", "2"]).make_gifs(_clip(), S, eps_by_sample=_eps())
    flags = res["trigger"]["flags"].cpu().numpy()
    assert res["trigger"]["min_gap"] == 2 and flags.any()
    for s in range(S):
        for b in range(B):
            assert (np.diff(np.nonzero(flags[s, :, b])[0]) >= 3).all(), (s, b, flags[s, :, b])


@pytest.mark.parametrize("inflight,share", [(0, True), (2, True), (2, False)])
def test_a_window_that_never_fills_in_time_leaves_every_sample_the_prefix(inflight, share):
    res = _generator(inflight, share, window=N_EVAL - 1).make_gifs(_clip(), S, eps_by_sample=_eps())
    assert not bool(res["trigger"]["flags"].any()) and bool(torch.isinf(res["trigger"]["thresholds"]).all())
    assert bool((res["trigger"]["values"][:, 1:] > 0).all())
    for s in range(1, S):
        assert torch.equal(res["samples"][s], res["samples"][0])
        assert torch.equal(res["trigger"]["values"][s], res["trigger"]["values"][0])


@pytest.mark.parametrize("inflight", [0, 2])
def test_the_period_rule_is_untouched(inflight):
    """--trigger period and no flag at all: the same tensors bit for bit, and no `trigger` entry (n_eval 17: one period step)."""
    import generate_frames
    res = []
    for extra in ([], ["--trigger", "period", "--trigger_window", "3", "--trigger_coef", "-0.5"]):
        opt = generate_frames.parse_args(["--synthetic_ckpt", "--batch_size", str(B), "--model", "dcgan", "--n_past", "2", "--n_eval", "17",
                                          "--inflight", str(inflight)] + extra)
        torch.manual_seed(SEED)
        g = generate_frames.Generator(opt, generate_frames.synthetic_checkpoint(opt), torch.device(DEV))
        assert g.trigger is None
        res.append(g.make_gifs(_clip(n_eval=17), 2, eps_by_sample=_eps(n_eval=17, s=2)))
    assert "trigger" not in res[0] and "trigger" not in res[1]
    for k in ("posterior", "samples", "ssim", "psnr", "best"):
        assert torch.equal(res[0][k], res[1][k]), k
    assert not torch.equal(res[0]["samples"][0, 16], res[0]["samples"][1, 16])     # the draw at step 15 happened


def test_vgg_eager_against_graphed():
    kw = dict(model="vgg", b=2, n_eval=7)
    clip, eps = _clip(2, 7), _eps(2, 7, 2)
    a = _generator(0, **kw).make_gifs(clip, 2, eps_by_sample=eps)
    b = _generator(1, **kw).make_gifs(clip, 2, eps_by_sample=eps)
    assert a["trigger"]["flags"].shape == (2, 7, 2)
    _same(a, b)


def test_command_line(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "generate_frames.py"), "--synthetic_ckpt", "--model", "dcgan", "--dataset",
                          "smmnist", "--batch_size", "4", "--n_past", "2", "--n_eval", "8", "--nsample", "2", "--nbatches", "1",
                          "--trigger", "variance", "--trigger_window", "3", "--trigger_coef", "-0.5", "--diversity", "--no_images",
                          "--log_dir", str(tmp_path)], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if "variance trigger" in ln]
    assert len(line) == 1 and "draws per sequence" in line[0] and "never drew" in line[0] and "first draw" in line[0], out.stdout
    assert "between the 2 samples" in out.stdout
    saved = torch.load(os.path.join(str(tmp_path), "gen", "sample_lstm_0.pt"), weights_only=False)
    tr = saved["trigger"]
    assert tr["flags"].shape == (2, 8, 4) and tr["flags"].dtype == torch.int32
    assert tr["values"].shape == tr["thresholds"].shape == (2, 8, 4)
    assert (tr["window"], tr["coef"], tr["min_gap"]) == (3, -0.5, 0) and "diversity" in saved
