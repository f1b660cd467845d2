"""GPU: train.py --val_every - dvg_val_accumulate (validate.hip) against tests/val_ref.py, dvg_amd.validate.Validator against the
rollouts it is made of, and the command line: training that does not notice, the EMA line, a resume, model_best.pth,
generate_frames.py --best and two ranks.

Bars (derived, not measured).  `best` and `cnt` are integers: exact.  A sum of n terms in fp64 is within (n - 1) 2^-53 sum|terms| of
the exact sum whatever the order, so two orders differ by at most (n - 1) 2^-52 sum|terms|; the inner mean over S samples is formed
alike on both sides.  The kernel tests hold every sum and sum of squares to (B + S) 2^-52 sum|terms| (val_ref.bar), n = B rows; the
Validator test to the same bar with n = all rows of the K batches.  Everything that compares two runs of the same code on the same
inputs is bit for bit.

Shapes: (B, S, T) of val_ref.SHAPES for the kernel - one row, one sample, one step, B below / at / above a wave and no multiple of
64, S above 64; dcgan_64 at batch 4, n_past 2, n_future 2 for the trainer, two batches of two samples per validation."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests import val_ref as ref, train_harness

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VAL = ["--val_every", "1", "--val_batches", "2", "--val_nsample", "2"]
RUN = ["--epoch_size", "2", "--save_every", "1", "--no_images", "--print_param_checksum"]


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
_REF = {}


def _case(shape):
    """(inputs on the host, reference acc / cnt / best, sum |terms|) of a shape: computed once, shared, never written."""
    if shape not in _REF:
        x = ref.inputs(*shape)
        _REF[shape] = (x, ref.accumulate(*x), ref.absum(*x))
    return _REF[shape]


def _dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _launch(arrays, acc=None, cnt=None, best=True):
    from dvg_amd import ops
    s, p, m = arrays
    if acc is None:
        acc, cnt = ops.val_accumulators(s.shape[2], DEV)
    b = torch.full((s.shape[0],), -7, dtype=torch.int32, device=DEV) if best else None
    ops.val_accumulate(s, p, m, acc, cnt, b)
    return acc, cnt, b


def _within(acc, want, shape, total_abs):
    err = np.abs(acc.cpu().numpy() - want)
    lim = ref.bar(shape[0], shape[1], total_abs)
    print("shape", shape, "max err / bar", float((err / np.maximum(lim, 1e-300)).max()))
    assert np.all(err <= lim), float((err / np.maximum(lim, 1e-300)).max())


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_the_reference(shape):
    x, (acc_r, cnt_r, best_r), total = _case(shape)
    d = _dev(x)
    acc, cnt, best = _launch(d)
    assert best.cpu().numpy().tolist() == best_r.tolist()
    assert np.array_equal(cnt.cpu().numpy(), cnt_r)
    if shape[0] > 2:
        assert int(cnt[:, 1, 0].abs().sum()) == 0 and float(acc[:, 1, 0].abs().sum()) == 0.0     # step 0: every psnr is +inf
    _within(acc, acc_r, shape, total)
    assert bool(torch.isfinite(acc).all())
    # the same launch again: the same bits; without `best`: the same sums
    acc2, cnt2, best2 = _launch(d)
    assert torch.equal(acc2.view(torch.int64), acc.view(torch.int64)) and torch.equal(cnt2, cnt) and torch.equal(best2, best)
    acc3, cnt3, _ = _launch(d, best=False)
    assert torch.equal(acc3.view(torch.int64), acc.view(torch.int64)) and torch.equal(cnt3, cnt)


@pytest.mark.parametrize("shape", [s for s in ref.SHAPES if s[0] >= 2], ids=lambda s: "x".join(map(str, s)))
def test_two_launches_over_two_halves_equal_one_reference_pass(shape):
    x, (acc_r, cnt_r, best_r), total = _case(shape)
    h = shape[0] // 2
    acc, cnt, b0 = _launch(_dev([a[:h] for a in x]))
    acc, cnt, b1 = _launch(_dev([a[h:] for a in x]), acc, cnt)
    assert torch.cat([b0, b1]).cpu().numpy().tolist() == best_r.tolist()
    assert np.array_equal(cnt.cpu().numpy(), cnt_r)
    _within(acc, acc_r, shape, total)


@pytest.mark.parametrize("shape", [(5, 7, 3), (130, 2, 33)], ids=lambda s: "x".join(map(str, s)))
def test_a_captured_launch_replayed_twice_equals_two_eager_launches(shape):
    from dvg_amd import graphs, ops
    d = _dev(_case(shape)[0])
    acc_e, cnt_e, best_e = _launch(d)
    _launch(d, acc_e, cnt_e)
    acc, cnt = ops.val_accumulators(shape[2], DEV)
    best = torch.zeros(shape[0], dtype=torch.int32, device=DEV)
    graphs.warm_up(lambda: ops.val_accumulate(*d, acc, cnt, best))
    acc.zero_()
    cnt.zero_()
    graph, _, _keep = graphs.capture(lambda: ops.val_accumulate(*d, acc, cnt, best))
    torch.cuda.synchronize()
    assert int(cnt.abs().sum()) == 0                 # a capture executes nothing
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(acc.view(torch.int64), acc_e.view(torch.int64)) and torch.equal(cnt, cnt_e) and torch.equal(best, best_e)


def test_wrapper_refuses_what_the_kernel_cannot_take():
    from dvg_amd import ops
    z = torch.zeros(2, 3, 4, device=DEV)
    acc, cnt = ops.val_accumulators(4, DEV)
    with pytest.raises(RuntimeError, match="float32"):
        ops.val_accumulate(z.double(), z, z, acc, cnt)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.val_accumulate(z, z.transpose(0, 1).contiguous().transpose(0, 1), z, acc, cnt)
    with pytest.raises(RuntimeError, match="like ssim"):
        ops.val_accumulate(z, z, z[:1], acc, cnt)
    with pytest.raises(RuntimeError, match="fp64"):
        ops.val_accumulate(z, z, z, acc.float(), cnt)
    with pytest.raises(RuntimeError, match="fp64"):
        ops.val_accumulate(z, z, z, *ops.val_accumulators(5, DEV))
    with pytest.raises(RuntimeError, match="int32"):
        ops.val_accumulate(z, z, z, acc, cnt, torch.zeros(2, dtype=torch.int64, device=DEV))
    assert float(acc.abs().sum()) == 0.0 and int(cnt.abs().sum()) == 0


# ---- the Validator ----------------------------------------------------------------------------------------------------------------
def _train_batch(seed=9):
    return train_harness.make_batches(1, seed=seed)[0]


def test_validator_reports_the_rollouts_numbers_and_leaves_no_trace():
    """n_eval 17: step 15 draws from the GP, so the samples differ from there on.  The Validator's clips and base samples through
    posterior_from / sample_from and utils.finn_eval_seq by hand, reduced by val_ref: the same sums within the bar, the same best
    samples; two runs give the same bits; modes, recurrent state, batch size, the fine-tuning cache and the caches are put back."""
    from dvg_amd import _derived, rollout, validate
    from dvg_amd import utils as dutils
    tr = train_harness.trainer(["--n_eval", "17"] + VAL)
    assert tr.validation is not None and tr.validation.every == 1
    x = _train_batch()
    tr.iteration(x)                                   # the GP's first call initialises its variational parameters
    tr.iteration(x)
    val = tr.validation.validator
    K, S, T, B = 2, 2, 15, 4
    assert (val.batches, val.nsample, val.steps) == (K, S, T)
    tr.train_mode()
    tr.likelihood.eval()                              # mixed flags must come back as they are
    hidden = [(torch.ones(1, device=DEV), torch.ones(1, device=DEV))]
    tr.frame_predictor.hidden, tr.frame_predictor.batch_size, tr._ft_cache = hidden, 4, ("sentinel",)
    flags = [sm.training for m in tr.modules for sm in m.modules()]
    skips, store = _derived.skip_mark(), {k: sorted(map(str, slot)) for k, (_, slot) in _derived.derived_mark().items()}
    rng = torch.cuda.get_rng_state(DEV).clone(), torch.get_rng_state().clone()
    p0 = tr.arena.p.clone()
    buffers = [b.clone() for m in tr.modules for b in m.buffers()]

    res = val.run(tr.modules, tr)
    acc1, cnt1, best1 = val.acc.clone(), val.cnt.clone(), val.best.clone()
    assert [sm.training for m in tr.modules for sm in m.modules()] == flags
    assert tr.frame_predictor.hidden is hidden and tr.frame_predictor.batch_size == 4 and tr._ft_cache == ("sentinel",)
    assert _derived.skip_mark() == skips
    assert {k: sorted(map(str, slot)) for k, (_, slot) in _derived.derived_mark().items()} == store
    assert torch.equal(torch.cuda.get_rng_state(DEV), rng[0]) and torch.equal(torch.get_rng_state(), rng[1])
    assert torch.equal(tr.arena.p, p0) and all(torch.equal(a, b) for a, b in zip(buffers, (b for m in tr.modules for b in m.buffers())))

    res2 = val.run(tr.modules, tr)
    assert res2 == res and torch.equal(val.acc.view(torch.int64), acc1.view(torch.int64)) and torch.equal(val.cnt, cnt1)

    # by hand
    for m in tr.modules:
        m.eval()
    mods = (tr.encoder, tr.decoder, tr.frame_predictor, tr.gp_layer, tr.likelihood)
    post_ref, samp_ref, post_abs, samp_abs = [None, None], [None, None], [None, None], [None, None]
    differ = 0
    with torch.no_grad():
        for x, eps in val.draws():
            assert len(x) == 17 and len(eps) == S and sorted(eps[0]) == [15] and not torch.equal(eps[0][15], eps[1][15])
            tr.frame_predictor.batch_size = B
            state = rollout.condition(tr.encoder, tr.frame_predictor, x, 2, False, decoder=tr.decoder)
            post = rollout.posterior_from(state, *mods, 2, 17)
            mse, ssim, psnr = (a.astype(np.float32)[:, None, :] for a in dutils.finn_eval_seq(x[2:17], post[2:17]))
            post_ref[0], post_ref[1], _ = ref.accumulate(ssim, psnr, mse, *post_ref)
            post_abs[0], post_abs[1], _ = ref.accumulate(ssim, psnr, mse, *post_abs, absolute=True)
            per = []
            for s in range(S):
                frames = rollout.sample_from(state, *mods, 2, 17, eps_by_step=eps[s])
                per.append([a.astype(np.float32) for a in dutils.finn_eval_seq(x[2:17], frames[2:17])])
            mse, ssim, psnr = (np.stack([per[s][k] for s in range(S)], 1) for k in range(3))
            differ += int((ssim[:, 0] != ssim[:, 1]).any(1).sum())
            samp_ref[0], samp_ref[1], best = ref.accumulate(ssim, psnr, mse, *samp_ref)
            samp_abs[0], samp_abs[1], _ = ref.accumulate(ssim, psnr, mse, *samp_abs, absolute=True)
    tr.train_mode()
    assert differ >= 1                                # at least one row's samples differ
    assert best1.cpu().numpy().tolist() == best.tolist()          # the last batch's best samples
    got_acc, got_cnt = acc1.cpu().numpy(), cnt1.cpu().numpy()
    for k, (want, total) in enumerate(((post_ref, post_abs), (samp_ref, samp_abs))):
        assert np.array_equal(got_cnt[k], want[1])
        err, lim = np.abs(got_acc[k] - want[0]), ref.bar(K * B, S, total[0])
        print("track set", k, "max err / bar", float((err / np.maximum(lim, 1e-300)).max()))
        assert np.all(err <= lim)
    assert np.array_equal(got_acc[0][0], got_acc[0][1])           # one "sample": the best and the mean are that sample
    t = res["tracks"]
    assert t["mean"]["ssim"]["curve"] != t["best"]["ssim"]["curve"] and t["mean"]["ssim"]["curve"][:13] == t["best"]["ssim"]["curve"][:13]
    assert res["clips"] == K * B and res["steps"] == T and res["nsample"] == S and res["score"] == t["best"]["ssim"]["mean"]
    want = validate.summarise(got_acc[1][0].tolist(), got_cnt[1][0].tolist())
    assert t["best"] == want and t["posterior"] == validate.summarise(got_acc[0][0].tolist(), got_cnt[0][0].tolist())
    n = got_cnt[1][0][0][14]
    assert n == K * B and t["best"]["ssim"]["curve"][14] == got_acc[1][0][0][14][0] / n


def test_without_the_flag_nothing_exists():
    tr = train_harness.trainer()
    assert tr.validation is None and "validation" not in tr.state_dict(epoch=0)
    with_val = train_harness.trainer(VAL)
    sd = with_val.state_dict(epoch=0)
    assert sd["validation"] == {"history": [], "best": {"score": None, "epoch": None}, "ema_best": {"score": None, "epoch": None}}
    o = train_harness.opt(VAL)
    o.rank = 1
    from dvg_amd import validate
    assert validate.make(o, torch.device(DEV)) is None            # rank 0 alone validates


# ---- the command line -------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _main(tmp_path_factory, capsys, name, extra):
    """train.main(train_harness.ARGS + RUN + extra) into a directory of its own, once per `name`: {"out", "text", "tr"}."""
    import train
    if name not in _RUNS:
        out = str(tmp_path_factory.mktemp("val") / name)
        capsys.readouterr()
        tr = train.main(train_harness.ARGS + RUN + ["--output_path", out] + list(extra))
        _RUNS[name] = {"out": out, "text": capsys.readouterr().out, "tr": tr}
    return _RUNS[name]


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and np.array_equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def _tensors(ck):
    """Every tensor of a model.pth container, by name."""
    out = {}
    for name in ("encoder", "decoder", "frame_predictor"):
        out.update({f"{name}.{k}": v for k, v in ck[name].state_dict().items()})
    for name in ("likelihood", "gp_layer"):
        out.update({f"{name}.{k}": v for k, v in ck[name].items()})
    return out


def _checksums(text):
    return [ln for ln in text.splitlines() if " param checksum " in ln]


@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_training_does_not_notice(tmp_path_factory, capsys, mode):
    flags = ["--niter", "2"] + (["--no_hip_graph"] if mode == "eager" else [])
    plain = _main(tmp_path_factory, capsys, f"{mode}-plain", flags)
    val = _main(tmp_path_factory, capsys, f"{mode}-val", flags + VAL)
    assert "capture failed" not in plain["text"] + val["text"]
    assert "     val: " not in plain["text"] and val["text"].count("     val: ssim ") == 2 and "val(ema)" not in val["text"]
    assert _checksums(plain["text"]) == _checksums(val["text"]) and len(_checksums(val["text"])) == 1
    a, b = (torch.load(os.path.join(r["out"], "model.pth"), weights_only=False) for r in (plain, val))
    ta, tb = _tensors(a), _tensors(b)
    assert set(ta) == set(tb) and any("running_mean" in k for k in ta)
    for k in ta:
        assert _same(ta[k], tb[k]), k
    sa, sb = (torch.load(os.path.join(r["out"], "train_state.pth"), weights_only=False) for r in (plain, val))
    assert _same(sa["rank_state"]["rng"], sb["rank_state"]["rng"]) and _same(sa["rank_state"]["data"], sb["rank_state"]["data"])
    assert _same(sa["rank_state"]["buffers"], sb["rank_state"]["buffers"]) and _same(sa["arena"], sb["arena"])
    assert "validation" not in sa and len(sb["validation"]["history"]) == 2
    assert not os.path.exists(os.path.join(plain["out"], "val_log.jsonl"))
    assert not os.path.exists(os.path.join(plain["out"], "model_best.pth"))
    log = [json.loads(ln) for ln in open(os.path.join(val["out"], "val_log.jsonl"))]
    assert [r["epoch"] for r in log] == [0, 1] and [r["global_step"] for r in log] == [2, 4]
    assert log[0]["clips"] == 8 and log[0]["steps"] == 2 and log[0]["nsample"] == 2
    assert os.path.exists(os.path.join(val["out"], "model_best.pth"))


def test_ema_line_scores_the_average(tmp_path_factory, capsys):
    """When the average IS the live weights the two lines carry the same numbers, bit for bit in the record; --ema_decay 0.9: both
    lines, different numbers, and model_ema_best.pth beside model_best.pth.
    --ema_decay 0 alone does not make the average the live weights: dvg_ema_update stores fmaf(1, p - e, e), which is p only where
    p - e is exact in fp32 (measured after 4 iterations of this run: 7 502 of 10 991 876 elements differ, all by rounding).  So
    the run is made with --ema_decay 0, both lines are checked to be there, and the comparison is made on that trainer after the
    remaining elements of the average have been set to the live weights - the bar stays bit for bit."""
    zero = _main(tmp_path_factory, capsys, "ema-0", ["--niter", "2", "--no_hip_graph", "--ema_decay", "0"] + VAL)
    lines = [ln for ln in zero["text"].splitlines() if ln.startswith("     val")]
    assert len(lines) == 4 and [ln.split(":")[0].strip() for ln in lines] == ["val", "val(ema)"] * 2
    tr = zero["tr"]
    off = int((tr.ema.e != tr.arena.p).sum())
    print("elements of the average that are not the live weight:", off, "of", tr.arena.p.numel())
    assert off < tr.arena.p.numel() // 100
    with torch.no_grad():
        tr.ema.e.copy_(tr.arena.p)
    capsys.readouterr()
    rec = tr.validation.validate(tr, 2)
    live = {k: rec[k] for k in ("tracks", "score", "clips", "steps", "nsample")}
    assert rec["ema"] == live
    a, b = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("     val")]
    assert a.replace("val:", "val(ema):").split("best so far")[0] == b.split("best so far")[0]
    nine = _main(tmp_path_factory, capsys, "ema-9", ["--niter", "2", "--no_hip_graph", "--ema_decay", "0.9"] + VAL)
    lines = [ln for ln in nine["text"].splitlines() if ln.startswith("     val")]
    assert len(lines) == 4
    for rec in nine["tr"].validation.history:
        assert rec["ema"]["tracks"] != rec["tracks"]
    assert sorted(f for f in os.listdir(nine["out"]) if "best" in f) == ["model_best.pth", "model_ema_best.pth"]
    sd = torch.load(os.path.join(nine["out"], "train_state.pth"), weights_only=False)
    assert sd["validation"]["ema_best"]["epoch"] in (0, 1) and sd["validation"]["ema_best"]["score"] is not None


def test_resume_continues_the_history_and_the_best_checkpoint(tmp_path_factory, capsys):
    """Four epochs in one go, and two + a resume for two more (eager iterations: a fresh process starts with eager warm-up
    iterations where the uninterrupted run replays): the same val_log.jsonl byte for byte, the same best epoch, the same
    model_best.pth.  A state without validations starts an empty history; one with them, resumed without the flag, says so."""
    eager = ["--no_hip_graph"]
    whole = _main(tmp_path_factory, capsys, "eager-whole", eager + ["--niter", "4"] + VAL)
    two = _main(tmp_path_factory, capsys, "eager-val", eager + ["--niter", "2"] + VAL)
    out = str(tmp_path_factory.mktemp("val") / "resumed")
    shutil.copytree(two["out"], out)
    import train
    capsys.readouterr()
    tr = train.main(train_harness.ARGS + RUN + eager + ["--niter", "4", "--output_path", out, "--resume", out] + VAL)
    text = capsys.readouterr().out
    assert "resumed from" in text and text.count("     val: ssim ") == 2
    a, b = (open(os.path.join(d, "val_log.jsonl"), "rb").read() for d in (whole["out"], out))
    assert a == b and a.count(b"\n") == 4
    assert tr.validation.best_live == whole["tr"].validation.best_live and tr.validation.best_live["epoch"] in (0, 1, 2, 3)
    ta, tb = (_tensors(torch.load(os.path.join(d, "model_best.pth"), weights_only=False)) for d in (whole["out"], out))
    assert set(ta) == set(tb) and all(_same(ta[k], tb[k]) for k in ta)
    assert _checksums(text) == _checksums(whole["text"])
    # a state without validations + the flag: an empty history, filled from here on
    plain = _main(tmp_path_factory, capsys, "eager-plain", eager + ["--niter", "2"])
    out2 = str(tmp_path_factory.mktemp("val") / "late")
    shutil.copytree(plain["out"], out2)
    capsys.readouterr()
    tr2 = train.main(train_harness.ARGS + RUN + eager + ["--niter", "3", "--output_path", out2, "--resume", out2] + VAL)
    assert [r["epoch"] for r in tr2.validation.history] == [2]
    assert open(os.path.join(out2, "val_log.jsonl")).read().count("\n") == 1
    # a state with validations, resumed without the flag: one line, no object, no new key
    out3 = str(tmp_path_factory.mktemp("val") / "dropped")
    shutil.copytree(two["out"], out3)
    capsys.readouterr()
    tr3 = train.main(train_harness.ARGS + RUN + eager + ["--niter", "3", "--output_path", out3, "--resume", out3])
    text3 = capsys.readouterr().out
    assert text3.count("the validation history in the file is ignored: this run has no --val_every") == 1
    assert tr3.validation is None and "     val: " not in text3
    assert "validation" not in torch.load(os.path.join(out3, "train_state.pth"), weights_only=False)


def test_best_checkpoint_is_the_checkpoint_of_the_best_epoch(tmp_path_factory, capsys):
    import generate_frames
    import train
    eager = ["--no_hip_graph"]
    whole = _main(tmp_path_factory, capsys, "eager-whole", eager + ["--niter", "4"] + VAL)
    hist = whole["tr"].validation.history
    scores = [r["score"] for r in hist]
    best = whole["tr"].validation.best_live
    assert best["score"] == max(scores) and best["epoch"] == scores.index(max(scores))     # strictly greater: the first of equals
    last = [ln for ln in whole["text"].splitlines() if ln.startswith("     val: ")][-1]
    assert last.endswith("best so far: epoch %d" % best["epoch"])
    # the same run stopped after the best epoch: what tr.save writes there
    again = _main(tmp_path_factory, capsys, "eager-to-best-%d" % best["epoch"], eager + ["--niter", str(best["epoch"] + 1)] + VAL) \
        if best["epoch"] != 3 else whole
    want = _tensors(train.train_state.checkpoint(again["tr"]))
    got = _tensors(torch.load(os.path.join(whole["out"], "model_best.pth"), weights_only=False))
    assert set(want) == set(got) and all(_same(want[k], got[k]) for k in want)
    gen_args = ["--model_dir", whole["out"], "--dataset", "smmnist", "--synthetic_data", "--batch_size", "4", "--n_eval", "6",
                "--n_future", "4", "--nsample", "2", "--nbatches", "1", "--no_images", "--log_dir", whole["out"] + "/logs"]
    gen = generate_frames.main(gen_args + ["--best"])
    w = dict(gen.encoder.state_dict())
    assert all(_same(v, got["encoder." + k]) for k, v in w.items())
    with pytest.raises(SystemExit) as exc:
        generate_frames.main(gen_args + ["--best", "--ema"])
    assert "model_ema_best.pth" in str(exc.value) and "\n" not in str(exc.value)
    os.remove(os.path.join(whole["out"], "model_best.pth"))
    with pytest.raises(SystemExit) as exc:
        generate_frames.main(gen_args + ["--best"])
    assert "model_best.pth" in str(exc.value)
    del _RUNS["eager-whole"]            # its directory is no longer what the run left


def test_two_ranks_rank_zero_validates_and_nobody_notices(tmp_path):
    """Two ranks on one GPU over gloo (the rehearsal switches and fresh child processes of tests/test_gpu_ema.py's two-rank
    test): with and without --val_every both ranks end with the same parameters as each other and as the other run, and every
    validation prints exactly one line."""
    args = ["--model", "dcgan", "--dataset", "smmnist", "--n_past", "2", "--n_future", "2", "--n_eval", "4", "--batch_size", "8",
            "--save_every", "1", "--no_images", "--print_param_checksum", "--niter", "2", "--epoch_size", "2"]

    def run(extra):
        r = train_harness.run_train_py(args + extra, ranks=2, env=dict(train_harness.REHEARSAL, DVG_FORCE_ALLREDUCE="1"))
        assert r.returncode == 0, r.stderr[-2000:]
        assert "capture failed" not in r.stderr
        pars = {ln.split()[1]: ln.split()[-2:] for ln in r.stdout.splitlines() if " param checksum " in ln}
        assert set(pars) == {"0", "1"} and pars["0"] == pars["1"], pars
        return r, pars["0"]

    r0, plain = run(["--output_path", str(tmp_path / "plain")])
    r1, val = run(["--output_path", str(tmp_path / "val")] + VAL)
    assert plain == val
    assert "     val: " not in r0.stdout and r1.stdout.count("     val: ssim ") == 2
    log = [json.loads(ln) for ln in open(tmp_path / "val" / "val_log.jsonl")]
    assert [r["epoch"] for r in log] == [0, 1] and log[0]["clips"] == 8          # rank 0's half of the batch, two batches
    sd = torch.load(tmp_path / "val" / "train_state.pth", weights_only=False)
    assert len(sd["validation"]["history"]) == 2 and os.path.exists(tmp_path / "val" / "model_best.pth")
