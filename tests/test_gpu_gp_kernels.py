"""GPU: the Matern members of the GP trigger's covariance family (--gp_kernel) against the fp64 torch restatement of
tests/gp_kernel_ref.py - forward and backward parity at the bars and on the seeds of the RBF tests (tests/test_gpu_parity.py,
tests/test_gpu_backward.py), step groups, the in-kernel soft-plus, the first-call initialisation, the module glue on both
autograd paths, and the flag's way through training, resume, the checkpoint and generation.  Every test prints the measured
error next to its bar."""
import functools
import io

import pytest
import torch

from oracle import params
from tests import gp_kernel_ref as ref
from tests import train_harness
from tests.common import rel_err
from tests.test_gpu_backward import grads_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MATERN = ("matern12", "matern32", "matern52")
ULP = 2.0 ** -22        # two fp32 ulps: the outputs are rounded to fp32 once

ZK = "variational_strategy.inducing_points"
MK = "variational_strategy.variational_distribution.variational_mean"
LK = "variational_strategy.variational_distribution.chol_variational_covar"


def _args(sd, raw=False):
    """(z, m, L_S, c, s, ell) on the device, soft-plus'ed by torch in fp32 like the layer does - or the raw parameters."""
    s, ell, c = ref.hypers(sd)
    if raw:
        s, ell = sd["covar_module.raw_outputscale"], sd["covar_module.base_kernel.raw_lengthscale"]
    return [t.to(DEV) for t in (sd[ZK], sd[MK], sd[LK], c, s, ell)]


def _absdiff(a, b):
    return float((a.double().cpu() - b.double()).abs().max())


@functools.lru_cache(maxsize=None)
def _forward_case(kernel, B, D, M):
    """Inputs of test_gpu_parity's GP test and the restatement's answers in fp64 and fp32, computed once per case."""
    sd, lik = params.gp_state(90, D=D, M=M)
    h = params.normal(91, B, D, scale=0.7).tanh()
    eps = params.normal(92, D, B)
    noise = ref.noise_of(lik)
    out = {"sd": sd, "h": h, "eps": eps, "noise": noise}
    for name, dt in (("64", torch.float64), ("32", torch.float32)):
        out["ev" + name] = ref.predict(kernel, h, sd, False, noise=noise, dtype=dt)
        out["tr" + name] = ref.predict(kernel, h, sd, True, dtype=dt)
    return out


@pytest.mark.parametrize("B,D,M", [(16, 12, 40), (50, 7, 24), (128, 8, 40), (7, 5, 64)])
@pytest.mark.parametrize("kernel", MATERN)
def test_forward_parity(kernel, B, D, M):
    """Eval (mean, var, cov, sample) and train mode (mean, var, KL) against the fp64 restatement: 1e-5 of max|mean|, 1e-4 of
    max|cov|, the sample also consistent with the kernel's own covariance at 1e-4, KL at 1e-4 relative; and the yardstick - the
    device is no further from fp64 than the restatement's own fp32 arithmetic (or two fp32 ulps of the scale).  B = 128 runs
    the packed-triangle fp64 variant."""
    from dvg_amd import ops
    from dvg_amd._lib import lib
    assert lib().dvg_gp_precision(B, M, 1) == 64 and lib().dvg_gp_precision(B, M, 0) == 64
    case = _forward_case(kernel, B, D, M)
    sd, h, eps, noise = case["sd"], case["h"], case["eps"], case["noise"]
    ev, ev32, tr, tr32 = case["ev64"], case["ev32"], case["tr64"], case["tr32"]
    args = _args(sd)
    r = ops.gp_predict(h.to(DEV), *args, noise=noise.to(DEV), eps=eps.to(DEV), want_cov=True, kernel=kernel)
    scale, mscale = float(ev["cov"].abs().max()), float(ev["mean"].abs().max())
    e_mean, e_cov, e_var = _absdiff(r["mean"], ev["mean"]), _absdiff(r["cov"], ev["cov"]), _absdiff(r["var"], ev["var"])
    smp = ref.rsample(ev["mean"], ev["cov"], eps.double())
    e_smp = _absdiff(r["sample"], smp)
    own = ref.rsample(r["mean"].double().cpu(), r["cov"].double().cpu(), eps.double())
    e_own = _absdiff(r["sample"], own)
    y_mean, y_cov = _absdiff(ev32["mean"], ev["mean"]), _absdiff(ev32["cov"], ev["cov"])
    print(f"\n{kernel} ({B},{D},{M}) eval: mean {e_mean / mscale:.2e} (bar 1e-5, fp32 {y_mean / mscale:.2e})  cov {e_cov / scale:.2e} "
          f"var {e_var / scale:.2e} (bar 1e-4, fp32 {y_cov / scale:.2e})  sample {e_smp / float(smp.abs().max()):.2e} (bar 1e-4)  "
          f"sample vs own cov {e_own:.2e} (bar 1e-4)")
    assert e_mean < 1e-5 * mscale and e_cov < 1e-4 * scale and e_var < 1e-4 * scale, (e_mean, e_cov, e_var)
    assert e_smp < 1e-4 * float(smp.abs().max()), e_smp
    assert e_own < 1e-4, e_own
    assert e_mean <= max(y_mean, ULP * mscale), (e_mean, y_mean)
    assert e_cov <= max(y_cov, ULP * scale), (e_cov, y_cov)

    t = ops.gp_predict(h.to(DEV), *args, want_kl=True, train_mode=True, kernel=kernel)
    e_mean, e_var = _absdiff(t["mean"], tr["mean"]), _absdiff(t["var"], tr["var"])
    e_kl = float(((t["kl"].double().cpu() - tr["kl"]).abs() / tr["kl"].abs()).max())
    y_var = _absdiff(tr32["var"], tr["var"])
    y_kl = float(((tr32["kl"].double() - tr["kl"]).abs() / tr["kl"].abs()).max())
    print(f"{kernel} ({B},{D},{M}) train: mean {e_mean / mscale:.2e} (bar 1e-5)  var {e_var / scale:.2e} (bar 1e-4, fp32 "
          f"{y_var / scale:.2e})  kl {e_kl:.2e} (bar 1e-4, fp32 {y_kl:.2e})")
    assert e_mean < 1e-5 * mscale and e_var < 1e-4 * scale and e_kl < 1e-4, (e_mean, e_var, e_kl)
    assert e_var <= max(y_var, ULP * scale) and e_kl <= max(y_kl, ULP), (e_var, y_var, e_kl, y_kl)


def _restated_grads(kernel, sd, lik, loss_of):
    """fp64 autograd through the restatement: loss_of(state dict, likelihood dict) -> scalar; gradients by parameter name,
    tril(chol) only (the kernels read the lower triangle)."""
    rs = {k: v.double().clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    rl = {k: v.double().clone().requires_grad_(True) for k, v in lik.items()}
    full = dict(sd)
    full.update(rs)
    loss = loss_of(full, rl)
    loss.backward()
    g = {k: v.grad for k, v in rs.items()}
    g["noise"] = rl["noise_covar.raw_noise"].grad
    g[LK] = torch.tril(g[LK])
    return float(loss.detach()), g


def _layer(kernel, sd, lik, D, M, num_data):
    from dvg_amd.models.gp_models import GaussianLikelihood, GPRegressionLayer1, VariationalELBO
    gp, like = GPRegressionLayer1(D, M, kernel=kernel), GaussianLikelihood(batch_size=D)
    gp.load_state_dict(sd)
    like.load_state_dict(lik)
    gp.to(DEV).train(), like.to(DEV).train()
    return gp, like, VariationalELBO(like, gp, num_data=num_data)


def _worst(ours, want):
    return max((rel_err(ours[k], g), k) for k, g in want.items() if g is not None)


@pytest.mark.parametrize("B,D,M", [(16, 12, 40), (50, 7, 24), (101, 5, 40)])
@pytest.mark.parametrize("kernel", MATERN)
def test_backward_parity(kernel, B, D, M):
    """dvg_gp_train_bwd_cov through the autograd glue against fp64 autograd of the restatement: inputs and loss of
    test_gp_train_backward (seeds 500-503, -ELBO + <mean, gmean>), every gradient at 1e-4.  B = 101: two ragged chunks of 51 + 50.
    Conditions on the inputs, asserted first from the restatement: no point within 1e-6 s of the variance clamp (the mask's
    derivative is a step) and no data point on an inducing point (the Matern kernels have a kink there)."""
    from dvg_amd import _lib
    assert _lib.lib().dvg_gp_bwd_precision(B, M) == 64 and (_lib.lib().dvg_gp_bwd_chunk(B, M) < B) == (B > 71)
    sd, lik = params.gp_state(500, D=D, M=M)
    h = params.normal(501, B, D, scale=0.7).tanh()
    tgt = params.normal(502, D, B, scale=0.5)
    gmean = params.normal(503, D, B)
    pr = ref.predict(kernel, h, sd, True)
    s = ref.hypers(sd)[0].double().view(-1, 1)
    clamp_gap, zx_gap = float((pr["gap"].abs() / s).min()), ref.min_gap_to_inducing(h, sd)
    print(f"\n{kernel} ({B},{D},{M}): smallest |s - q| / s {clamp_gap:.2e}, smallest |z - x| {zx_gap:.2e}")
    assert clamp_gap > 1e-6 and zx_gap > 0.0

    hr = h.double().clone().requires_grad_(True)

    def loss_of(full, rl):
        p = ref.predict(kernel, hr, full, True)
        return -(ref.elbo(p, tgt.double(), ref.noise_of(rl), num_data=B).sum()) + (p["mean"] * gmean.double()).sum()
    loss_r, want = _restated_grads(kernel, sd, lik, loss_of)
    want["h"] = hr.grad

    gp, like, mll = _layer(kernel, sd, lik, D, M, B)
    ho = h.to(DEV).requires_grad_(True)
    pred = gp(ho.transpose(0, 1).view(D, B, 1))
    loss_o = -(mll(pred, tgt.to(DEV)).sum()) + (pred.mean * gmean.to(DEV)).sum()
    loss_o.backward()
    ours = {k: p.grad for k, p in gp.named_parameters()}
    ours["h"], ours["noise"] = ho.grad, like.noise_covar.raw_noise.grad
    print(f"{kernel} ({B},{D},{M}) backward: loss {abs(float(loss_o) - loss_r) / abs(loss_r):.2e} (bar 1e-5), worst gradient "
          f"{_worst(ours, want)} (bar 1e-4)")
    assert abs(float(loss_o) - loss_r) < 1e-5 * abs(loss_r) + 1e-5
    grads_close(ours, want, tol=1e-4)


@pytest.mark.parametrize("S,B,k", [(7, 16, 4), (3, 40, 2)])
@pytest.mark.parametrize("kernel", ["matern32", "matern52"])
def test_step_groups_equal_one_workgroup_per_step(kernel, S, B, k):
    """step_group = k against one workgroup per (step, dim), as test_gp_step_groups_equal_one_workgroup_per_step: mean and
    variance bit-identical, KL within 1e-6, every gradient within 1e-5."""
    from dvg_amd import ops
    D, M = 90, 40
    sd, _ = params.gp_state(560, D=D, M=M)
    par = _args(sd)
    par[0] = par[0].squeeze(-1)
    h = params.normal(561, B, S * D, scale=0.7).tanh().to(DEV)
    gmean, gvar = params.normal(562, S * D, B).to(DEV), params.normal(563, S * D, B).abs().to(DEV)
    gkl = params.normal(564, S * D).to(DEV)
    out = {}
    for kk in (1, k):
        r = ops.gp_predict(h, *par, want_var=True, want_kl=True, train_mode=True, param_period=D, step_group=kk, kernel=kernel)
        g = ops.gp_train_bwd(h, *par, gmean, gvar, gkl, param_period=D, step_group=kk, kernel=kernel)
        assert g["groups"] == -(-S // kk) and g["dz"].shape[0] == g["groups"] * D
        names = ("dz", "dm", "dls", "dc", "ds", "dell")
        summed = ops.sum_steps([g[n] for n in names], g["groups"]) if g["groups"] > 1 else [g[n].reshape(-1) for n in names]
        out[kk] = (r, g["dh"], dict(zip(names, summed)))
    (ra, dha, ga), (rb, dhb, gb) = out[1], out[k]
    worst = max([(rel_err(gb[n], ga[n]), n) for n in ga] + [(rel_err(dhb, dha), "dh")])
    print(f"\n{kernel} S={S} B={B} k={k}: kl {rel_err(rb['kl'], ra['kl']):.2e} (bar 1e-6), worst gradient {worst} (bar 1e-5)")
    assert torch.equal(ra["mean"], rb["mean"]) and torch.equal(ra["var"], rb["var"])
    assert rel_err(rb["kl"], ra["kl"]) < 1e-6
    assert worst[0] < 1e-5, worst


def test_raw_hyper_parameters_in_kernel():
    """matern52, (50, 90, 40): soft-plus and the noise floor applied in the kernel against the soft-plus'ed call, 1e-5 of scale
    (as test_gp_raw_hyper_parameters_in_kernel)."""
    from dvg_amd import ops
    B, D, M = 50, 90, 40
    sd, lik = params.gp_state(93, D=D, M=M)
    h = params.normal(94, B, D, scale=0.7).tanh().to(DEV)
    eps = params.normal(95, D, B).to(DEV)
    a = ops.gp_predict(h, *_args(sd), noise=ref.noise_of(lik).to(DEV), eps=eps, want_cov=True, kernel="matern52")
    b = ops.gp_predict(h, *_args(sd, raw=True), noise=lik["noise_covar.raw_noise"].to(DEV), eps=eps, want_cov=True,
                       raw_hypers=True, kernel="matern52")
    errs = {k: float((a[k] - b[k]).abs().max()) / float(a[k].abs().max()) for k in ("mean", "cov", "sample")}
    print(f"\nmatern52 raw hypers against soft-plus'ed: {errs} (bar 1e-5)")
    assert all(e < 1e-5 for e in errs.values()), errs


def test_the_kind_reaches_the_kernel():
    """kernel="rbf" is the call without the argument, bit for bit, forward and backward; every Matern member moves the
    covariance by more than 1e-3 of its scale, and its gradients too."""
    from dvg_amd import ops
    B, D, M = 16, 12, 40
    case = _forward_case("matern12", B, D, M)
    sd, h, eps, noise = case["sd"], case["h"].to(DEV), case["eps"].to(DEV), case["noise"].to(DEV)
    args = _args(sd)
    plain = ops.gp_predict(h, *args, noise=noise, eps=eps, want_cov=True)
    rbf = ops.gp_predict(h, *args, noise=noise, eps=eps, want_cov=True, kernel="rbf")
    assert all(torch.equal(plain[k], rbf[k]) for k in ("mean", "var", "cov", "sample"))
    up = [params.normal(570 + i, *shape).to(DEV) for i, shape in enumerate(((D, B), (D, B), (D,)))]
    up[1] = up[1].abs()
    g_plain, g_rbf = ops.gp_train_bwd(h, *args, *up), ops.gp_train_bwd(h, *args, *up, kernel="rbf")
    names = ("dh", "dz", "dm", "dls", "dc", "ds", "dell")
    assert all(torch.equal(g_plain[n], g_rbf[n]) for n in names)
    scale = float(plain["cov"].abs().max())
    for kernel in MATERN:
        r = ops.gp_predict(h, *args, noise=noise, eps=eps, want_cov=True, kernel=kernel)
        g = ops.gp_train_bwd(h, *args, *up, kernel=kernel)
        moved = float((r["cov"] - plain["cov"]).abs().max()) / scale
        print(f"\n{kernel} against rbf: cov moves by {moved:.2e} of its scale, dz by {rel_err(g['dz'], g_plain['dz']):.2e}")
        assert moved > 1e-3 and rel_err(g["dz"], g_plain["dz"]) > 1e-3 and rel_err(g["dell"], g_plain["dell"]) > 1e-3
    with pytest.raises(RuntimeError, match="matern72"):
        ops.gp_predict(h, *args, kernel="matern72")


@pytest.mark.parametrize("kernel", MATERN)
def test_prior_init(kernel):
    """An untrained layer's first train-mode call: chol_variational_covar = chol((K_ZZ + 1e-3 I)^-1) of ITS kernel - the same fp64
    host computation as the restatement, rounded once: 1e-6 relative - and the GP starts at its prior, |KL| < 2e-3 (zero up to
    the fp32 storage of L_S, the RBF test's bar)."""
    from dvg_amd.models import gp_models as gm
    D, M, B = 12, 40, 16
    assert gm.INIT_JITTER_TERMS == 1
    sd, _ = params.gp_state(96, D=D, M=M, trained=False)
    h = params.normal(97, B, D, scale=0.7).tanh()
    layer = gm.GPRegressionLayer1(D, M, kernel=kernel)
    layer.load_state_dict(sd)
    layer.to(DEV).train()
    with torch.no_grad():
        kl = layer(h.to(DEV)).kl.double().cpu()
    _, ls = ref.prior_init(kernel, sd, 1)
    got = layer.variational_strategy.variational_distribution.chol_variational_covar.detach().cpu()
    e = rel_err(got, ls.to(torch.float32))
    print(f"\n{kernel} prior init: L_S {e:.2e} (bar 1e-6), |KL| {float(kl.abs().max()):.2e} (bar 2e-3)")
    assert int(layer.variational_strategy.variational_params_initialized) == 1
    assert e < 1e-6 and float(kl.abs().max()) < 2e-3


def test_module_level_on_both_autograd_paths():
    """GPRegressionLayer1(D, M, kernel="matern52") from a seeded state through layer(h), likelihood and VariationalELBO in
    train mode - the single step, and gp_elbo_steps with S = 3, B = 16 - against the restatement: ELBO and posterior mean at
    1e-5 / 1e-4, every gradient at 1e-4.  The glue passes the kind on both paths."""
    from dvg_amd.gp_autograd import gp_elbo_steps
    kernel, S, B, D, M = "matern52", 3, 16, 12, 40
    sd, lik = params.gp_state(540, D=D, M=M)
    hin = params.normal(541, S, B, D, scale=0.7).tanh()
    htgt = params.normal(542, S, B, D, scale=0.5)
    w_elbo, w_mean = params.normal(543, S, D), params.normal(544, S, B, D)
    for steps in (1, S):
        hr = hin[:steps].double().clone().requires_grad_(True)
        vals = {}

        def loss_of(full, rl):
            loss = 0.0
            for i in range(steps):
                p = ref.predict(kernel, hr[i], full, True)
                e = ref.elbo(p, htgt[i].double().t(), ref.noise_of(rl), num_data=37)
                vals[i] = (e.detach(), p["mean"].detach().t())
                loss = loss + (e * w_elbo[i].double()).sum() + (p["mean"].t() * w_mean[i].double()).sum()
            return loss
        _, want = _restated_grads(kernel, sd, lik, loss_of)
        want["h"] = hr.grad
        gp, like, mll = _layer(kernel, sd, lik, D, M, 37)
        assert gp.kernel == kernel
        hi = hin[:steps].to(DEV).requires_grad_(True)
        if steps == 1:
            pred = gp(hi[0].transpose(0, 1).view(D, B, 1))
            elbo, mean = mll(pred, htgt[0].to(DEV).transpose(0, 1)).view(1, D), pred.mean.transpose(0, 1)[None]
            noisy = ref.predict(kernel, hin[0], sd, True, noise=ref.noise_of(lik))["var"]          # likelihood(gp_layer(h))
            e_noisy = rel_err(like(gp(hi[0].detach().transpose(0, 1).view(D, B, 1))).variance, noisy)
            print(f"\nmatern52 module: likelihood(layer(h)).variance {e_noisy:.2e} (bar 1e-4)")
            assert e_noisy < 1e-4
        else:
            elbo, mean = gp_elbo_steps(gp, mll, hi, htgt.to(DEV))
            elbo = elbo.view(S, D)
        ((elbo * w_elbo[:steps].to(DEV)).sum() + (mean * w_mean[:steps].to(DEV)).sum()).backward()
        ours = {k: p.grad for k, p in gp.named_parameters()}
        ours["h"], ours["noise"] = hi.grad, like.noise_covar.raw_noise.grad
        e_elbo = rel_err(elbo, torch.stack([vals[i][0] for i in range(steps)]))
        e_mean = rel_err(mean, torch.stack([vals[i][1] for i in range(steps)]))
        print(f"\nmatern52 module, {steps} step(s): elbo {e_elbo:.2e} (bar 1e-4)  mean {e_mean:.2e} (bar 1e-5)  worst gradient "
              f"{_worst(ours, want)} (bar 1e-4)")
        assert e_elbo < 1e-4 and e_mean < 1e-5
        grads_close(ours, want, tol=1e-4)


# ---- training, resume, checkpoint, generation ------------------------------------------------------------------------------------
M52 = ["--gp_kernel", "matern52"]


def _train(extra, n, graphed=False, resume_after=None, seed=3):
    """n iterations of the harness' Trainer on the same batches; resume_after = k: after k iterations the state goes through a
    file image into a fresh Trainer with another seed."""
    import train
    tr = train_harness.trainer(extra, seed=seed)
    xs = train_harness.make_batches(n)
    step = train.GraphedIteration(tr, warmup=1) if graphed else tr.iteration
    torch.manual_seed(77)
    losses = []
    for i, x in enumerate(xs):
        if resume_after is not None and i == resume_after:
            f = io.BytesIO()
            torch.save(tr.state_dict(epoch=0), f)
            f.seek(0)
            del tr, step
            tr = train_harness.trainer(extra, seed=99)
            tr.load_state_dict(torch.load(f, weights_only=False))
            step = tr.iteration
        losses.append(tuple(step(x)) + (tr.last_loss,))
    torch.cuda.synchronize()
    if graphed:
        assert not step.failed and step.graph is not None
    return tr, losses


@pytest.fixture(scope="module")
def matern_eager():
    """Two eager iterations with --gp_kernel matern52, shared by the tests below: (trainer, parameters, losses)."""
    a, la = _train(M52, 2)
    assert a.gp_layer.kernel == "matern52" and a.state_dict(epoch=0)["fingerprint"]["gp_kernel"] == "matern52"
    line = a.gp_report.epoch_line()
    assert "matern52" in line and "lengthscale" in line and "outputscale" in line
    return a, a.arena.p.clone(), la


def test_training_eager_against_graphed(matern_eager):
    """dcgan_64, B = 4, 2-in / 2-out, --gp_kernel matern52: two iterations eager against GraphedIteration at the bars of
    test_training_with_a_gru_eager_against_graphed (losses 2e-4 relative, parameters rtol 2e-3 / atol 2e-5)."""
    _, pa, la = matern_eager
    g, lg = _train(M52, 2, graphed=True)
    worst = max(abs(s - t) / max(1.0, abs(s)) for u, v in zip(la, lg) for s, t in zip(u, v))
    print(f"\nmatern52 training: losses {la}; eager against graphed: losses {worst:.2e} (bar 2e-4), parameters "
          f"{float((g.arena.p - pa).abs().max()):.2e}")
    assert worst <= 2e-4
    assert torch.allclose(g.arena.p, pa, rtol=2e-3, atol=2e-5)


def test_training_resumes_exactly_and_refuses_another_kernel(matern_eager):
    _, pa, la = matern_eager
    a2, _ = _train(M52, 2)
    noise = float((a2.arena.p - pa).abs().max())
    del a2
    r, lr_ = _train(M52, 2, resume_after=1)
    got = float((r.arena.p - pa).abs().max())
    print(f"\nmatern52 resume: A vs A {noise:.3e}, resumed vs A {got:.3e}")
    if noise == 0.0:
        assert torch.equal(r.arena.p, pa) and lr_ == la
    else:
        assert got <= 2 * noise
    other = train_harness.trainer([], seed=5)
    assert other.gp_layer.kernel == "rbf" and other.gp_report is None
    with pytest.raises(SystemExit, match="gp_kernel is 'matern52' in the file and 'rbf' in this run"):
        other.load_state_dict(r.state_dict(epoch=0))


def test_gp_kernel_rbf_is_the_run_without_the_flag():
    a, la = _train([], 2)
    assert a.gp_layer.kernel == "rbf" and "gp_kernel" not in a.state_dict(epoch=0)["fingerprint"]
    pa = a.arena.p.clone()
    del a
    a2, _ = _train([], 2)
    noise = float((a2.arena.p - pa).abs().max())
    del a2
    b, lb = _train(["--gp_kernel", "rbf"], 2)
    assert b.gp_layer.kernel == "rbf" and "gp_kernel" not in b.state_dict(epoch=0)["fingerprint"] and b.gp_report is None
    got = float((b.arena.p - pa).abs().max())
    print(f"\n--gp_kernel rbf vs no flag: A vs A {noise:.3e}, flag vs A {got:.3e}")
    if noise == 0.0:
        assert torch.equal(b.arena.p, pa) and lb == la
    else:
        assert got <= 2 * noise


def test_checkpoint_to_generation(matern_eager):
    """train_state.checkpoint of the matern52 trainer through generate_frames.Generator with no kernel flag: the layer is built
    with the checkpoint's kernel, one eval-mode sample rollout (n_past 2, n_eval 4, a GP draw at step 3) eager equals its graph
    bit for bit (the existing rollout tests' bar), and the draw is not the one an rbf layer makes from the same state dict."""
    import generate_frames
    from dvg_amd import train_state
    from dvg_amd.models.gp_models import GPRegressionLayer1
    from dvg_amd.rollout import GraphedRollout, sample_rollout
    tr, _, _ = matern_eager
    ckpt = train_state.checkpoint(tr)
    assert ckpt["opt"].gp_kernel == "matern52"
    B, n_past, n_eval = 4, 2, 4
    opt = generate_frames.build_parser().parse_args(["--batch_size", str(B), "--model", "dcgan", "--n_past", str(n_past), "--n_eval",
                                                     str(n_eval)])
    assert opt.gp_kernel == "rbf"          # the command line says nothing: the checkpoint decides
    g = generate_frames.Generator(opt, ckpt, torch.device(DEV))
    assert g.gp_layer.kernel == "matern52"
    mods = [g.encoder, g.decoder, g.frame_predictor, g.gp_layer, g.likelihood]
    xs = [params.frames(2310 + t, B, 1, 64).to(DEV) for t in range(n_eval)]
    eps = {3: params.normal(2320, 90, B).to(DEV)}
    with torch.no_grad():
        eager = [f.clone() for f in sample_rollout(*mods, xs, n_past, n_eval, period=3, eps_by_step=eps)]
        got = GraphedRollout(*mods, xs, n_past, n_eval, period=3)(xs, eps)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, eager))
        rbf = GPRegressionLayer1(90)
        rbf.load_state_dict(ckpt["gp_layer"])
        rbf.to(DEV).eval()
        h = params.normal(2330, B, 90, scale=0.7).tanh().to(DEV)
        draw = {layer.kernel: g.likelihood(layer(h)).rsample(eps[3]) for layer in (g.gp_layer, rbf)}
        other = sample_rollout(mods[0], mods[1], mods[2], rbf, mods[4], xs, n_past, n_eval, period=3, eps_by_step=eps)
    moved = float((draw["matern52"] - draw["rbf"]).abs().max())
    print(f"\ncheckpoint to generation: the GP draw moves by {moved:.2e} against an rbf layer on the same state dict")
    assert moved > 1e-3 and not torch.equal(other[3], eager[3])
    assert all(torch.equal(other[t], eager[t]) for t in range(3))       # no GP draw before step 3
