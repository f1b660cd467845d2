"""GPU: the held-out scores of the GP trigger - dvg_gp_score (gp_score.hip) against tests/gp_score_ref.py, dvg_amd.gp_score.GPScorer
against a torch-fp64 recomputation from the modules' public calls, and the two command lines: train.py --val_every 1 --val_gp
(training does not notice, the line, the log, a resume) and generate_frames.py --gp_report.

Bars.  Counts are integers decided by two IEEE products on either side: equal, for input sets that keep 1e-9 away from every edge
(gp_score_ref.case asserts it on the CPU).  Sums: 1e-13 sum|terms| per slot (gp_score_ref.bar says where that comes from).  The
scorer: the same fp32 moments enter both sides, only the summation differs: 1e-12 relative on every pooled number, equal counts.
Everything that compares two runs of the same code on the same inputs is bit for bit.

Shapes: (R, B, noise period) of gp_score_ref.SHAPES for the kernel; dcgan_64 with the default latent size at batch 4, n_past 2,
n_eval 5, two batches for the scorer; tests/test_gpu_validate.py's sizes for train.py."""
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch

from tests import gp_score_ref as ref, train_harness

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VAL = ["--val_every", "1", "--val_batches", "2", "--val_nsample", "2"]
RUN = ["--epoch_size", "2", "--save_every", "1", "--no_images", "--print_param_checksum"]
IDS = ["x".join(map(str, s)) for s in ref.SHAPES]


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
_REF = {}


def _case(shape, noise):
    """(inputs on the host, reference (acc, cnt, sum |terms|)) of an input set: computed once, shared, never written."""
    key = tuple(shape) + (noise,)
    if key not in _REF:
        x = ref.case(*shape, noise=noise)
        _REF[key] = (x, ref.accumulate(*x))
    return _REF[key]


def _dev(x, layout="contiguous", cols=slice(None)):
    """The input set on the device (columns `cols` of it); layout "view": the target is a transposed view of a (B, R) tensor."""
    mean, var, nz, period, target = x
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    target = t(target[:, cols].T).t() if layout == "view" else t(target[:, cols])
    assert target.is_contiguous() == (layout == "contiguous" or min(target.shape) == 1)
    return t(mean[:, cols]), t(var[:, cols]), target, None if nz is None else t(nz), period


def _launch(d, acc=None, cnt=None):
    from dvg_amd import ops
    mean, var, target, nz, period = d
    if acc is None:
        acc, cnt = ops.gp_score_accumulators(mean.shape[0], DEV)
    ops.gp_score(mean, var, target, acc, cnt, noise=nz, noise_period=period)
    return acc, cnt


def _within(acc, want, absum, what):
    """Prints the largest |error| / sum|terms| per slot, then holds every slot of every row to the bar."""
    err = np.abs(acc.cpu().numpy() - want)
    ratio = np.where(absum > 0, err / np.where(absum > 0, absum, 1.0), np.where(err > 0, np.inf, 0.0))
    print(what, "max |err| / sum|terms| per slot:", " ".join("%.1e" % v for v in ratio.max(0)))
    assert np.all(err <= ref.bar(absum)), float(ratio.max())


@pytest.mark.parametrize("layout", ["contiguous", "view"])
@pytest.mark.parametrize("noise", [True, False], ids=["noise", "latent"])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_kernel_matches_the_reference(shape, noise, layout):
    x, (acc_r, cnt_r, absum) = _case(shape, noise)
    d = _dev(x, layout)
    acc, cnt = _launch(d)
    assert np.array_equal(cnt.cpu().numpy(), cnt_r)
    _within(acc, acc_r, absum, f"shape {shape} noise {noise} {layout}")
    assert bool(torch.isfinite(acc).all())
    # the same launch again: the same bits; into the same accumulators: twice the counts
    acc2, cnt2 = _launch(d)
    assert torch.equal(acc2.view(torch.int64), acc.view(torch.int64)) and torch.equal(cnt2, cnt)
    _launch(d, acc2, cnt2)
    assert torch.equal(cnt2, 2 * cnt) and torch.equal(acc2, 2 * acc)          # (x + x is exact)


@pytest.mark.parametrize("shape", [s for s in ref.SHAPES if s[1] >= 2], ids=[i for i, s in zip(IDS, ref.SHAPES) if s[1] >= 2])
def test_two_launches_over_two_halves_equal_one_reference_pass(shape):
    x, (acc_r, cnt_r, absum) = _case(shape, True)
    h = shape[1] // 2
    acc, cnt = _launch(_dev(x, "view", slice(0, h)))
    _launch(_dev(x, "contiguous", slice(h, None)), acc, cnt)
    assert np.array_equal(cnt.cpu().numpy(), cnt_r)
    _within(acc, acc_r, absum, f"shape {shape} in two halves")


@pytest.mark.parametrize("shape", [(3, 65, 0), (15, 33, 5)], ids=["3x65x0", "15x33x5"])
def test_a_captured_launch_replayed_twice_equals_two_eager_launches(shape):
    from dvg_amd import graphs, ops
    d = _dev(_case(shape, True)[0], "view")
    acc_e, cnt_e = _launch(d)
    _launch(d, acc_e, cnt_e)
    acc, cnt = ops.gp_score_accumulators(shape[0], DEV)
    graphs.warm_up(lambda: _launch(d, acc, cnt))
    acc.zero_()
    cnt.zero_()
    graph, _, _keep = graphs.capture(lambda: _launch(d, acc, cnt))
    torch.cuda.synchronize()
    assert int(cnt.abs().sum()) == 0                 # a capture executes nothing
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(acc.view(torch.int64), acc_e.view(torch.int64)) and torch.equal(cnt, cnt_e)


def test_wrapper_refuses_what_the_kernel_cannot_take():
    from dvg_amd import ops
    z, nz = torch.zeros(6, 4, device=DEV), torch.ones(3, device=DEV)
    acc, cnt = ops.gp_score_accumulators(6, DEV)
    assert ops.GP_SCORE_SLOTS == (14, 14) and tuple(acc.shape) == tuple(cnt.shape) == (6, 14)
    with pytest.raises(RuntimeError, match="float32"):
        ops.gp_score(z.double(), z, z, acc, cnt)
    with pytest.raises(RuntimeError, match="float32"):
        ops.gp_score(z, z, z, acc, cnt, noise=nz.double(), noise_period=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gp_score(z, z, z.cpu(), acc, cnt)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.gp_score(z.t().contiguous().t(), z, z, acc, cnt)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.gp_score(z, z[:, :2], z[:, :2], acc, cnt)
    with pytest.raises(RuntimeError, match="target"):
        ops.gp_score(z, z, z[:3], acc, cnt)
    with pytest.raises(RuntimeError, match="noise period"):
        ops.gp_score(z, z, z, acc, cnt, noise=torch.ones(4, device=DEV), noise_period=4)
    with pytest.raises(RuntimeError, match="noise period"):
        ops.gp_score(z, z, z, acc, cnt, noise=nz, noise_period=-3)
    with pytest.raises(RuntimeError, match="noise period"):
        ops.gp_score(z, z, z, acc, cnt, noise_period=5)                       # (refused with or without noise)
    with pytest.raises(RuntimeError, match="variances"):
        ops.gp_score(z, z, z, acc, cnt, noise=nz, noise_period=2)
    with pytest.raises(RuntimeError, match="variances"):
        ops.gp_score(z, z, z, acc, cnt, noise=nz)
    with pytest.raises(RuntimeError, match="fp64"):
        ops.gp_score(z, z, z, acc.float(), cnt)
    with pytest.raises(RuntimeError, match="fp64"):
        ops.gp_score(z, z, z, *ops.gp_score_accumulators(5, DEV))
    with pytest.raises(RuntimeError, match="int64"):
        ops.gp_score(z, z, z, acc, cnt.int())
    assert float(acc.abs().sum()) == 0.0 and int(cnt.abs().sum()) == 0
    ops.gp_score(z, z + 1, z, acc, cnt, noise=nz, noise_period=3)             # and what it can
    assert cnt[:, 0].tolist() == [4] * 6 and acc[:, 3].tolist() == [8.0] * 6


# ---- the scorer -------------------------------------------------------------------------------------------------------------------
GEN = ["--synthetic_ckpt", "--model", "dcgan", "--dataset", "smmnist", "--synthetic_data", "--batch_size", "4", "--n_past", "2",
       "--n_eval", "5", "--n_future", "3", "--nsample", "2", "--nbatches", "2", "--no_images"]


def _generator(kernel):
    """A Generator on a synthetic checkpoint whose GP has left its prior: an untrained GP predicts ONE variance everywhere (its
    prior's, up to fp32 rounding), which leaves the variance ~ error correlation undefined (and any number put there is decided
    by rounding: a Pearson coefficient from pooled moments loses mean^2 / variance of its digits).  A short length scale and a
    variational distribution that is tight along some whitened directions and loose along others make the variance depend on
    the input by a large factor, as a trained GP's does: the coefficient is then as well conditioned as the other numbers."""
    import generate_frames
    opt = generate_frames.build_parser().parse_args(GEN + ["--gp_kernel", kernel])
    torch.manual_seed(5)
    torch.cuda.manual_seed_all(5)
    gen = generate_frames.Generator(opt, generate_frames.synthetic_checkpoint(opt), torch.device(DEV))
    with torch.no_grad():
        gen.gp_layer.covar_module.base_kernel.raw_lengthscale.fill_(-2.0)          # soft-plus: 0.127
        gen.gp_layer.variational_strategy.inducing_points.mul_(2.0).sub_(1.0)      # over the encoder's tanh range
        gen.gp_layer.ensure_initialized()
        vd = gen.gp_layer.variational_strategy.variational_distribution
        vd.variational_mean.add_(0.3 * torch.randn_like(vd.variational_mean))
        vd.chol_variational_covar.mul_(torch.rand_like(vd.variational_mean).mul_(0.95).add_(0.05).unsqueeze(-1))
    return gen


def _clips(opt, n=2):
    import utils
    from dvg_amd.data import SyntheticMovingMNIST
    ds = SyntheticMovingMNIST(seq_len=opt.n_eval, image_size=opt.image_width, seed=opt.seed + 7919)
    return [utils.normalize_data(opt, torch.cuda.FloatTensor, ds.batch(opt.batch_size))[0] for _ in range(n)]


def _posterior(gen, x):
    from dvg_amd import rollout
    o = gen.opt
    gen.frame_predictor.batch_size = x[0].shape[0]
    state = rollout.condition(gen.encoder, gen.frame_predictor, x, o.n_past, o.last_frame_skip, decoder=gen.decoder)
    return rollout.posterior_from(state, gen.encoder, gen.decoder, gen.frame_predictor, gen.gp_layer, gen.likelihood, o.n_past,
                                  o.n_eval, o.last_frame_skip)


def _pooled_by_hand(entries):
    """The pooled scores from the entries themselves in fp64 on the host: entries = [(mean, v, y), ...], each (D, B) fp64."""
    m, v, y = (torch.cat([e[k].flatten() for e in entries]).cpu() for k in range(3))
    assert bool(torch.isfinite(m).all() and torch.isfinite(y).all() and (v > 0).all())
    e = y - m
    e2, z = e * e, e / v.sqrt()
    se = e * e.abs()
    decile = sum((se > c * v).long() for c in ref.EDGES)
    corr = np.corrcoef(v.numpy(), e2.numpy())[0, 1]
    return {"nlpd": float((0.5 * (ref.LN_2PI + v.log() + e2 / v)).mean()), "rmse": math.sqrt(float(e2.mean())), "mae": float(e.abs().mean()),
            "mean_var": float(v.mean()), "z_mean": float(z.mean()), "z_std": float(z.std(unbiased=False)),
            "cover68": float((e2 <= v).double().mean()), "cover95": float((e2 <= ref.CHI2_95 * v).double().mean()),
            "pit": [float((decile == k).double().mean()) for k in range(10)], "var_err_corr": float(corr),
            "smse": float(e2.sum() / ((y - y.mean()) ** 2).sum()), "taken": e.numel(), "skipped": 0}


def _by_hand(gen, batches, with_likelihood=False):
    """Both tracks' pooled numbers from the modules' public calls: encoder(x)[0], gp_layer(...).mean / .variance and the
    likelihood's noise, added in fp64 - or, with_likelihood, likelihood(gp_layer(...)).variance, which carries the noise in fp32."""
    from dvg_amd import rollout
    o, out = gen.opt, {"forced": [], "rollout": []}
    B, D = o.batch_size, o.g_dim
    with torch.no_grad():
        noise = gen.likelihood.noise.double().view(-1, 1)
        for x in batches:
            post = _posterior(gen, x)
            h = gen.encoder(torch.cat(list(x[:o.n_eval])))[0].view(o.n_eval, B, D)
            h_fed = gen.encoder(torch.cat(list(post[o.n_past - 1:o.n_eval - 1])))[0].view(o.n_eval - o.n_past, B, D)
            for track, h_in, first in (("forced", h[:o.n_eval - 1], 1), ("rollout", h_fed, o.n_past)):
                for s in range(h_in.shape[0]):
                    pred = gen.gp_layer(rollout.gp_input(gen.gp_layer, h_in[s]))
                    if with_likelihood:
                        v = gen.likelihood(pred).variance.double()
                    else:
                        v = pred.variance.double() + noise
                    out[track].append((pred.mean.double(), v, h[first + s].t().double()))
    return {t: _pooled_by_hand(e) for t, e in out.items()}


@pytest.mark.parametrize("kernel", ["rbf", "matern52"])
def test_scorer_reports_what_the_modules_public_calls_give(kernel):
    from dvg_amd import gp_score
    gen = _generator(kernel)
    o = gen.opt
    assert o.g_dim == 90 and gen.gp_layer.kernel == kernel
    batches = _clips(o)
    scorer = gen.gp_scorer()
    assert scorer.steps == {"forced": 4, "rollout": 3} and scorer.acc["forced"].shape == (4 * 90, 14)
    for x in batches:
        gen.score_gp(scorer, x, _posterior(gen, x))
    got = scorer.read()
    want = _by_hand(gen, batches)
    for track in gp_score.TRACKS:
        rep, w = got[track], want[track]
        assert rep["pooled"]["taken"] == w["taken"] == 2 * 4 * 90 * scorer.steps[track] and rep["pooled"]["skipped"] == 0
        assert len(rep["per_step"]) == scorer.steps[track] and len(rep["per_dim"]) == 90 and len(rep["worst_dims"]) == 5
        for k in ("cover68", "cover95", "pit"):
            assert rep["pooled"][k] == w[k], (track, k)                         # counts over the same n
        for k in ("nlpd", "rmse", "mae", "mean_var", "z_mean", "z_std", "var_err_corr", "smse"):
            assert rep["pooled"][k] is not None, (track, k)
            rel = abs(rep["pooled"][k] - w[k]) / abs(w[k])
            print(kernel, track, k, "%.12g" % rep["pooled"][k], "rel err %.1e" % rel)
            assert rel <= 1e-12, (track, k, rep["pooled"][k], w[k])
        print(kernel, track, "pooled:", json.dumps(rep["pooled"]))
        assert [s["taken"] for s in rep["per_step"]] == [2 * 4 * 90] * scorer.steps[track]
    # the first rollout step is fed a ground-truth frame: the forced track's step n_past - 1 (the encoder saw it in a batch of
    # another size: the same numbers to fp32 rounding, not bit for bit)
    assert got["rollout"]["per_step"][0]["nlpd"] == pytest.approx(got["forced"]["per_step"][o.n_past - 1]["nlpd"], rel=1e-4)
    assert got["rollout"]["per_step"][1] != got["forced"]["per_step"][o.n_past]
    # likelihood(gp_layer(h)).variance is the same predictive with var + noise rounded to fp32: each v within 3 x 2^-24 (the
    # kernel's soft-plus, its sum and the rounding of the result), so the pooled mean within 2^-22
    lik = _by_hand(gen, batches, with_likelihood=True)
    for track in gp_score.TRACKS:
        rel = abs(got[track]["pooled"]["mean_var"] - lik[track]["mean_var"]) / lik[track]["mean_var"]
        print(kernel, track, "mean var against likelihood(...).variance: rel %.1e" % rel)
        assert rel <= 2.0 ** -22
    # a second pass over the same batches: the same bits; zero() starts over
    first = {t: scorer.acc[t].clone() for t in gp_score.TRACKS}
    scorer.zero()
    for x in batches:
        gen.score_gp(scorer, x, _posterior(gen, x))
    assert all(torch.equal(scorer.acc[t].view(torch.int64), first[t].view(torch.int64)) for t in gp_score.TRACKS)
    assert scorer.read() == got
    with pytest.raises(ValueError, match="steps"):
        scorer.score(gen.encoder, gen.gp_layer, gen.likelihood, batches[0], _posterior(gen, batches[0]), 3, 5)


# ---- train.py ---------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _main(tmp_path_factory, capsys, name, extra):
    """train.main(train_harness.ARGS + RUN + extra) into a directory of its own, once per `name`: {"out", "text", "tr"}."""
    import train
    if name not in _RUNS:
        out = str(tmp_path_factory.mktemp("valgp") / name)
        capsys.readouterr()
        tr = train.main(train_harness.ARGS + RUN + ["--output_path", out] + list(extra))
        _RUNS[name] = {"out": out, "text": capsys.readouterr().out, "tr": tr}
    return _RUNS[name]


def _checksums(text):
    return [ln for ln in text.splitlines() if " param checksum " in ln]


def _log(run):
    return [json.loads(ln) for ln in open(os.path.join(run["out"], "val_log.jsonl"))]


@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_training_does_not_notice_and_the_record_carries_gp(tmp_path_factory, capsys, mode):
    flags = ["--niter", "2"] + (["--no_hip_graph"] if mode == "eager" else [])
    val = _main(tmp_path_factory, capsys, f"{mode}-val", flags + VAL)
    gp = _main(tmp_path_factory, capsys, f"{mode}-gp", flags + VAL + ["--val_gp"])
    assert "capture failed" not in val["text"] + gp["text"]
    assert _checksums(val["text"]) == _checksums(gp["text"]) and len(_checksums(gp["text"])) == 1
    assert "val gp:" not in val["text"] and gp["text"].count("     val gp: nlpd ") == 2 and gp["text"].count("     val: ssim ") == 2
    line = [ln for ln in gp["text"].splitlines() if ln.startswith("     val gp: ")][0]
    for word in ("rmse", "mean var", "z std", "cover 68/95", "pit err", "var~err corr", "| rollout: nlpd", "cover 95"):
        assert word in line, word
    assert "nan" not in line.replace("var~err corr nan", "")
    a, b = _log(val), _log(gp)
    assert len(a) == len(b) == 2 and all("gp" not in r for r in a) and all(sorted(r["gp"]) == ["forced", "rollout"] for r in b)
    for ra, rb in zip(a, b):                              # everything else in the record is what it was
        assert {k: v for k, v in rb.items() if k != "gp"} == ra
    rec = b[0]["gp"]
    assert rec["forced"]["pooled"]["taken"] == 8 * 90 * 3 and rec["rollout"]["pooled"]["taken"] == 8 * 90 * 2
    assert len(rec["forced"]["per_step"]) == 3 and len(rec["rollout"]["per_dim"]) == 90
    sa, sb = (torch.load(os.path.join(r["out"], "train_state.pth"), weights_only=False) for r in (val, gp))
    assert all("gp" not in r for r in sa["validation"]["history"]) and all("gp" in r for r in sb["validation"]["history"])
    assert val["tr"].validation.validator.gp is None and gp["tr"].validation.validator.gp is not None


def test_without_the_flag_no_launch_and_with_it_one_per_batch_and_track():
    from dvg_amd import ops
    counts = {}
    for name, extra in (("plain", VAL), ("gp", VAL + ["--val_gp"])):
        tr = train_harness.trainer(extra)
        x = train_harness.make_batches(1)[0]
        tr.iteration(x)                                   # the GP's first call initialises its variational parameters
        timer = ops.KernelTimer()
        ops.set_timer(timer)
        try:
            res = tr.validation.validator.run(tr.modules, tr)
        finally:
            ops.set_timer(None)
        counts[name] = sum(1 for r in timer.records if r[0] == "gp_score")
        assert ("gp" in res) == (name == "gp") and ("gp" in tr.state_dict(epoch=0)["validation"]) is False
        tr.train_mode()
    assert counts == {"plain": 0, "gp": 2 * 2}            # two batches x two tracks


def test_resume_continues_the_history(tmp_path_factory, capsys):
    import train
    eager = ["--no_hip_graph"]
    two = _main(tmp_path_factory, capsys, "eager-gp", eager + ["--niter", "2"] + VAL + ["--val_gp"])
    whole = _main(tmp_path_factory, capsys, "eager-gp-3", eager + ["--niter", "3"] + VAL + ["--val_gp"])
    out = str(tmp_path_factory.mktemp("valgp") / "resumed")
    shutil.copytree(two["out"], out)
    capsys.readouterr()
    tr = train.main(train_harness.ARGS + RUN + eager + ["--niter", "3", "--output_path", out, "--resume", out] + VAL + ["--val_gp"])
    text = capsys.readouterr().out
    assert "resumed from" in text and text.count("     val gp: nlpd ") == 1
    a, b = (open(os.path.join(d, "val_log.jsonl"), "rb").read() for d in (whole["out"], out))
    assert a == b and a.count(b"\n") == 3 and a.count(b'"gp"') == 3
    assert [r["epoch"] for r in tr.validation.history] == [0, 1, 2] and all("gp" in r for r in tr.validation.history)
    assert _checksums(text) == _checksums(whole["text"])
    # the flag is not part of the fingerprint: the same state resumes without it, and its later records have no gp
    out2 = str(tmp_path_factory.mktemp("valgp") / "dropped")
    shutil.copytree(two["out"], out2)
    tr2 = train.main(train_harness.ARGS + RUN + eager + ["--niter", "3", "--output_path", out2, "--resume", out2] + VAL)
    assert ["gp" in r for r in tr2.validation.history] == [True, True, False]


def test_ema_line(tmp_path_factory, capsys):
    run = _main(tmp_path_factory, capsys, "ema", ["--niter", "1", "--no_hip_graph", "--ema_decay", "0.9"] + VAL + ["--val_gp"])
    lines = [ln.split(":")[0].strip() for ln in run["text"].splitlines() if ln.startswith("     val")]
    assert lines == ["val", "val gp", "val(ema)", "val(ema) gp"]
    rec = run["tr"].validation.history[0]
    assert sorted(rec["ema"]["gp"]) == ["forced", "rollout"] and rec["ema"]["gp"] != rec["gp"]


# ---- generate_frames.py -----------------------------------------------------------------------------------------------------------
def test_generate_frames_gp_report(tmp_path, capsys):
    import generate_frames
    from dvg_amd import gp_score

    def run(name, extra):
        torch.manual_seed(11)
        torch.cuda.manual_seed_all(11)
        capsys.readouterr()
        gen = generate_frames.main(GEN + ["--gp_kernel", "matern32", "--log_dir", str(tmp_path / name)] + extra)
        return gen, capsys.readouterr().out
    gen, text = run("with", ["--gp_report"])
    path = tmp_path / "with" / "gen" / "gp_report.json"
    rep = json.load(open(path))
    assert rep == json.loads(json.dumps(gen.gp_report)) and sorted(rep) == ["forced", "rollout"]
    assert sorted(os.listdir(tmp_path / "with" / "gen")) == ["gp_report.json", "sample_lstm_0.pt", "sample_lstm_1.pt"]
    assert rep["forced"]["pooled"]["taken"] == 2 * 4 * 90 * 4 and rep["rollout"]["pooled"]["taken"] == 2 * 4 * 90 * 3
    for tag in gp_score.TRACKS:
        assert text.count("gp %s (" % tag) == 1 and "%s nlpd by step: " % tag in text and "%s cover 95 by step: " % tag in text
    # the scorer called directly on the same clips with the same generator: the same numbers
    scorer = gen.gp_scorer()
    for x in _clips(gen.opt):
        gen.score_gp(scorer, x, gen.make_gifs(x, 2)["posterior"])
    assert scorer.read() == gen.gp_report
    # without the flag: no file, no key, and the saved tensors are what the run with it saved beside the report
    plain, text0 = run("without", [])
    assert not hasattr(plain, "gp_report") and "gp forced" not in text0
    assert sorted(os.listdir(tmp_path / "without" / "gen")) == ["sample_lstm_0.pt", "sample_lstm_1.pt"]
    for i in range(2):
        a = torch.load(tmp_path / "with" / "gen" / f"sample_lstm_{i}.pt", weights_only=False)
        b = torch.load(tmp_path / "without" / "gen" / f"sample_lstm_{i}.pt", weights_only=False)
        assert a.pop("gp_report") == gen.gp_report and "gp_report" not in b and sorted(a) == sorted(b)
        assert all(torch.equal(a[k], b[k]) for k in a)
