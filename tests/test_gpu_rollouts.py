"""GPU parity of the orchestration rows S and K of SURVEY.md §8: the step closures' values, the qualitative rollout of
train.py (`plot`), the posterior rollout and the variance-trigger generation of generate_frames.py, best-of-N selection -
HIP path vs the oracle's restatements (oracle/dvg_oracle.py), base samples eps passed in.  Integer results (trigger-step
lists, argmin / argsort indices) must be EXACT; frames hold the 1e-4 bar, GP-sampled steps included (the GP kernels
compute in fp64 since ABI 6); the one looser bar left is train-mode BatchNorm at B = 4 in `plot`, which amplifies fp32
rounding of the conv kernels step by step (2e-3) and has nothing to do with the GP."""
import numpy as np
import pytest
import torch

from oracle import dvg_oracle as orc
from oracle import params
from tests.common import rel_err, to64, yardstick
from tests.test_gpu_configs import _build, _oracle_fns

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLOT_BAR = 1e-5        # frames of train.py's `plot` rollout after n_past (train-mode BatchNorm at B = 4): measured r05 worst
#                        HIP vs fp64 1.2e-6, worst fp32 oracle vs fp64 2.0e-6 over the 10 predicted steps (r04's bar: 2e-3)
CLOSURE_BAR = 1e-6     # LSTM fine-tuning closure VALUE against the oracle: measured r05 <= 1.8e-7
GP_CLOSURE_BAR = 5e-5  # GP fine-tuning closure VALUE (-ELBO): measured r05 1.3e-5 at B = 4 (the oracle's GP is fp64 in both runs)


def _cpu_state(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def _trainer(model, batch, n_past, n_future, n_eval, nc=1, width=64, seed=3):
    import train
    torch.manual_seed(seed)
    o = train.options(["--model", model, "--batch_size", str(batch), "--n_past", str(n_past), "--n_future", str(n_future),
                       "--n_eval", str(n_eval), "--channels", str(nc), "--image_width", str(width), "--dataset", "smmnist", "--no_save"])
    tr = train.Trainer(o, torch.device(DEV))
    tr.train_mode()
    tr.gp_layer(torch.zeros(batch, 90, device=DEV))   # prior initialisation of the variational distribution
    return tr, o


def _train_mode_fns(model, width, esd, dsd):
    if model == "vgg":
        return (lambda t: orc.vgg_encoder(t, esd, True)), (lambda v, s: orc.vgg_decoder(v, s, dsd, True))
    act = "tanh" if width == 64 else "sigmoid"
    return (lambda t: orc.dcgan_encoder(t, esd, True)), (lambda v, s: orc.dcgan_decoder(v, s, dsd, True, act))


@pytest.mark.parametrize("model", ["dcgan", "vgg"])
def test_finetuning_closure_values_match_oracle(model):
    """train_frame_predictor (train.py:175-198) and train_GP_Frame_predictor (:146-172): the returned VALUES against the
    oracle composition (train-mode BatchNorm; the GP closure reuses the LSTM closure's encodings on our side)."""
    tr, o = _trainer(model, 4, 2, 2, 4)
    x = [params.frames(1200 + t, 4, 1, 64) for t in range(4)]
    esd, lsd, gsd, lik = (_cpu_state(m) for m in (tr.encoder, tr.frame_predictor, tr.gp_layer, tr.likelihood))
    e64, l64, g64, k64 = (to64(sd) for sd in (esd, lsd, gsd, lik))
    enc, _ = _train_mode_fns(model, 64, esd, None)
    enc64, _ = _train_mode_fns(model, 64, e64, None)
    x64 = [t.double() for t in x]
    T = o.n_past + o.n_future
    with torch.no_grad():
        ref_fp = float(orc.train_frame_predictor_loss(x, enc, lsd, o.n_past, o.n_future)) / T
        ref_gp = float(orc.train_gp_loss(x, enc, gsd, lik, o.n_past, o.n_future, num_data=o.batch_size)) / T
        r64_fp = float(orc.train_frame_predictor_loss(x64, enc64, l64, o.n_past, o.n_future)) / T
        r64_gp = float(orc.train_gp_loss(x64, enc64, g64, k64, o.n_past, o.n_future, num_data=o.batch_size)) / T
    xd = [t.to(DEV) for t in x]
    got_fp = tr.train_frame_predictor(xd)
    got_gp = tr.train_GP_Frame_predictor(xd)
    yardstick(f"train_frame_predictor value {model}", got_fp, ref_fp, r64_fp, ratio=1.5, slack=CLOSURE_BAR)
    yardstick(f"train_GP_Frame_predictor value {model}", got_gp, ref_gp, r64_gp, ratio=1.5, slack=GP_CLOSURE_BAR)
    assert abs(got_fp - ref_fp) < CLOSURE_BAR * abs(ref_fp), (got_fp, ref_fp)
    assert abs(got_gp - ref_gp) < GP_CLOSURE_BAR * abs(ref_gp), (got_gp, ref_gp)


@pytest.mark.slow
def test_plot_rollout_and_best_of_n_match_oracle():
    """train.py:256-310: encoder / decoder stay in TRAIN mode, LSTM / GP / likelihood in eval (train.py:372-374); the one
    GP-sampled step is i == 10; best-of-N by summed squared error must pick the same sample per row."""
    n_past, n_eval, B, S = 3, 13, 4, 3
    tr, o = _trainer("dcgan", B, n_past, 10, n_eval)
    tr.frame_predictor.eval(), tr.gp_layer.eval(), tr.likelihood.eval()
    x = [params.frames(1300 + t, B, 1, 64) for t in range(n_eval)]
    eps = [params.normal(1320 + s, 90, B) for s in range(S)]
    esd, dsd, lsd, gsd, lik = (_cpu_state(m) for m in (tr.encoder, tr.decoder, tr.frame_predictor, tr.gp_layer,
                                                       tr.likelihood))
    e64, d64, l64, g64, k64 = (to64(sd) for sd in (esd, dsd, lsd, gsd, lik))
    enc, dec = _train_mode_fns("dcgan", 64, esd, dsd)
    enc64, dec64 = _train_mode_fns("dcgan", 64, e64, d64)
    with torch.no_grad():
        ref = orc.plot_rollout(x, enc, dec, lsd, gsd, lik, n_past, n_eval, eps)
        ref64 = orc.plot_rollout([t.double() for t in x], enc64, dec64, l64, g64, k64, n_past, n_eval, [e.double() for e in eps])
    ref_best = orc.best_of_n_sse(x, ref, B)
    gen, best = tr.plot([t.to(DEV) for t in x], 0, nsample=S, eps_by_sample=[e.to(DEV) for e in eps])
    assert gen.shape == (S, n_eval, B, 1, 64, 64)
    # A 10-step autoregressive rollout through TRAIN-mode BatchNorm at B = 4: every step divides by batch statistics of four
    # images, so fp32 rounding is amplified step by step - in the oracle's own fp32 run as much as in ours.  Measured, per
    # step: truth = the oracle in fp64, yardstick = the oracle in fp32; HIP stays within 1.5 x that (+ 1e-5), and the bar
    # against the fp32 oracle is 3 x the largest HIP deviation measured (r05).
    worst = [0.0, 0.0]
    for s in range(S):
        for t in range(n_eval):
            e_hip, e_32 = rel_err(gen[s, t], ref64[s][t]), rel_err(ref[s][t], ref64[s][t])
            worst = [max(worst[0], e_hip), max(worst[1], e_32)]
            assert e_hip <= 1.5 * e_32 + 1e-5, (s, t, e_hip, e_32)
            tol = 1e-4 if t < n_past else PLOT_BAR
            assert rel_err(gen[s, t], ref[s][t]) < tol, (s, t, rel_err(gen[s, t], ref[s][t]))
    print(f"yardstick plot rollout (train-mode BN, B=4, {n_eval - n_past} steps): worst HIP vs fp64 {worst[0]:.2e} | worst fp32 "
          f"oracle vs fp64 {worst[1]:.2e}")
    assert best.tolist() == ref_best, (best.tolist(), ref_best)
    # the frames after i == 10 differ between samples (distinct eps), the frames before do not
    assert torch.equal(gen[0, 9], gen[1, 9]) and not torch.equal(gen[0, 10], gen[1, 10])
    # BatchNorm side effects of plot(): the discarded encoder(x[i]) calls of train.py:273-274 count as well
    got = tr.encoder.state_dict()
    for k in ("c1.main.1.running_mean", "c1.main.1.running_var", "c5.1.running_mean"):
        print(f"plot rollout BatchNorm buffer {k}: rel err {rel_err(got[k], esd[k]):.2e}")
        assert rel_err(got[k], esd[k]) < 1e-4, k
    # per sample: 2 encoder calls per conditioning step (train.py:267,273), 1 per predicted step
    assert int(got["c1.main.1.num_batches_tracked"]) == S * (2 * (n_past - 1) + (n_eval - n_past))


@pytest.mark.parametrize("family", ["dcgan", "vgg"])
def test_posterior_rollout_matches_oracle(family):
    """generate_frames.py:110-134: the GP is fed the LSTM output and its predictive MEAN is decoded at every step.  Both forms:
    `posterior_rollout` (the reference's loop) and `posterior_from(condition())` (what make_gifs runs: the conditioning phase
    shared with the samples, its frames encoded as one batch)."""
    from dvg_amd.rollout import condition, posterior_from, posterior_rollout
    B, n_past, n_eval = 4, 3, 8
    mods, (esd, dsd, lsd, gsd, lik) = _build(family, 64, 1, B, 1400)
    xs = [params.frames(1410 + t, B, 1, 64) for t in range(n_eval)]
    enc_o, dec_o = _oracle_fns(family, 64, esd, dsd)
    with torch.no_grad():
        ref = orc.posterior_rollout(xs, enc_o, dec_o, lsd, gsd, lik, n_past, n_eval)
    for m in mods:
        m.to(DEV).eval()
    ours = posterior_rollout(*mods, [t.to(DEV) for t in xs], n_past, n_eval)
    assert len(ours) == len(ref) == n_eval
    for t in range(n_eval):
        assert rel_err(ours[t], ref[t]) < 1e-4, (t, rel_err(ours[t], ref[t]))
    xd = [t.to(DEV) for t in xs]
    with torch.no_grad():
        st = condition(mods[0], mods[2], xd, n_past, decoder=mods[1])
        shared = posterior_from(st, *mods, n_past, n_eval)
    assert len(shared) == n_eval
    for t in range(n_eval):
        assert rel_err(shared[t], ref[t]) < 1e-4, (t, rel_err(shared[t], ref[t]))
        assert rel_err(shared[t], ours[t]) < 2e-5       # same arithmetic per image; tile choices may differ with the batch


@pytest.mark.parametrize("family,B", [("dcgan", 1), ("dcgan", 3), ("dcgan", 7), ("vgg", 1), ("vgg", 5)])
def test_posterior_rollout_at_ragged_batches(family, B):
    """The rollout at batch sizes that divide none of the kernels' tiles (the 4-image 4 x 4 tiles, the 8-row waves of the LSTM /
    GEMV kernels, the GP's point chunks, Winograd tile groups): B = 1, 3, 5, 7 against the oracle at the inference bar, plain
    and as a captured hipGraph (the reference runs whatever batch the data loader's last slice has: generate_frames.py:300-318
    drops nothing)."""
    from dvg_amd.rollout import GraphedRollout, posterior_rollout, sample_rollout
    n_past, n_eval = 2, 5
    mods, (esd, dsd, lsd, gsd, lik) = _build(family, 64, 1, B, 1500 + B)
    xs = [params.frames(1520 + t, B, 1, 64) for t in range(n_eval)]
    enc_o, dec_o = _oracle_fns(family, 64, esd, dsd)
    with torch.no_grad():
        ref = orc.posterior_rollout(xs, enc_o, dec_o, lsd, gsd, lik, n_past, n_eval)
    for m in mods:
        m.to(DEV).eval()
    xd = [t.to(DEV) for t in xs]
    ours = posterior_rollout(*mods, xd, n_past, n_eval)
    for t in range(n_eval):
        assert ours[t].shape == ref[t].shape and rel_err(ours[t], ref[t]) < 1e-4, (t, rel_err(ours[t], ref[t]))
    with torch.no_grad():
        eager = [f.clone() for f in sample_rollout(*mods, xd, n_past=n_past, n_eval=n_eval)]      # (no trigger step inside 2 + 3)
        graphed = GraphedRollout(*mods, xd, n_past, n_eval)(xd)
    assert len(graphed) == len(eager) == n_eval
    for t in range(n_eval):
        assert torch.equal(graphed[t], eager[t]), t


@pytest.mark.parametrize("depth,index", [(1, 0), (1, 2), (-250, 1)])
def test_gp_trigger_generation_matches_oracle(depth, index):
    """generate_frames.py:249-298 per batch index: variance norms (float32, host-side like the reference), thresholds, the
    LIST OF TRIGGER STEPS (exact) and the frames.  depth = 1 is the reference's value; depth = -250 turns the threshold into
    mean - 0.5 std so that both branches (GP sample without LSTM step / LSTM generation) are exercised densely.  The warm-up
    reads sample `index`, the main loop sample [3] (the reference's asymmetry)."""
    import generate_frames
    B, total = 4, 20   # untrained networks roll out towards a fixed point: later steps sit within fp32 noise of the threshold
    opt = generate_frames.build_parser().parse_args(["--synthetic_ckpt", "--batch_size", str(B), "--model", "dcgan"])
    mods, (esd, dsd, lsd, gsd, lik) = _build("dcgan", 64, 1, B, 1500)
    ckpt = {"encoder": mods[0], "decoder": mods[1], "frame_predictor": mods[2], "likelihood": lik, "gp_layer": gsd}
    g = generate_frames.Generator(opt, ckpt, torch.device(DEV))
    xs = [params.frames(1510, B, 1, 64)]
    eps = {i: params.normal(1520 + i, 90, B) for i in range(12, total)}
    enc_o, dec_o = _oracle_fns("dcgan", 64, esd, dsd)
    with torch.no_grad():
        ref = orc.gp_trigger_gen(xs, enc_o, dec_o, lsd, gsd, lik, index, eps, total=total, depth=depth)
    margin = min(abs(v - th) / abs(th) for v, th in zip(ref["values"][12:], ref["thresholds"]))
    assert margin > 5e-4, f"case too close to the threshold to be a meaningful exact-match test ({margin:.1e})"
    res = g.gp_trigger_gen([xs[0].to(DEV)], n_index=index + 1, total=total, depth=depth,
                           eps_by_step={k: v.to(DEV) for k, v in eps.items()}, keep_batch=True)[index]
    assert res["index"] == index
    assert res["triggers"] == ref["triggers"], (res["triggers"], ref["triggers"])
    if depth != 1:
        assert 0 < len(ref["triggers"]) < total - 12, "both branches must have been taken"
    np.testing.assert_allclose(res["values"], ref["values"], rtol=margin / 4)      # far inside every decision margin
    np.testing.assert_allclose(res["thresholds"], ref["thresholds"], rtol=margin / 4)
    for t in range(total):
        tol = 1e-4       # before AND after the first GP-sampled step
        assert rel_err(res["batch_frames"][t], ref["frames"][t]) < tol, (t, rel_err(res["batch_frames"][t], ref["frames"][t]))
    # the eager form of the device schedule: the same kernels on the same operands -> the same frames, bit for bit; the
    # reference's own schedule (a host round trip and 2-3 encoder calls per step, the warm-up per index): the same decisions
    # and frames up to the summation order of the decoder's concat convs (the device schedule declares the skip frozen at step
    # 4 and adds the hoisted skip half from then on, the host loop's decoder hoists from the second sighting)
    epd = {k: v.to(DEV) for k, v in eps.items()}
    for kw in ({"graph": False}, {"host_loop": True}):
        alt = g.gp_trigger_gen([xs[0].to(DEV)], indices=[index], total=total, depth=depth, eps_by_step=epd, keep_batch=True, **kw)[0]
        assert alt["triggers"] == res["triggers"], kw
        np.testing.assert_allclose(alt["values"], res["values"], rtol=1e-5)
        for t in range(total):
            if "graph" in kw:
                assert torch.equal(alt["batch_frames"][t], res["batch_frames"][t]), (kw, t)
            else:
                assert rel_err(alt["batch_frames"][t], res["batch_frames"][t]) < 1e-5, (kw, t)
    with pytest.raises(IndexError):
        g.frame_predictor.batch_size = 2
        g.gp_trigger_gen([xs[0][:2].to(DEV)], n_index=1, total=14)


@pytest.mark.slow
@pytest.mark.parametrize("family,depth", [("dcgan", -250), ("dcgan", 1), ("vgg", -250)])
def test_gp_trigger_generation_at_the_reference_batch(family, depth):
    """GPtrigger_gen as generate_frames.py:47-49,249-298 configures it: B = 50, the batch indices {0, 3, 49} (the warm-up reads
    sample `index`, the main loop sample [3]), 40 steps after the warm-up, both backbone families, the whole batch's frames at
    1e-4.  `value > threshold` is a discontinuity and untrained networks roll out towards a fixed point where the margin
    falls to fp32 noise, so the oracle runs SECOND with the decision-margin guard of `orc.gp_trigger_gen`: a step whose oracle
    margin is below 1e-4 follows the HIP run's branch (reported, counted), every other step decides for itself and must
    agree with the HIP run EXACTLY; values and thresholds are compared at every step.  depth = -250 (threshold = mean - 0.5
    std) exercises both branches densely; depth = 1 is the reference's value."""
    import generate_frames
    B, total, guard = 50, 52, 1e-4
    opt = generate_frames.build_parser().parse_args(["--synthetic_ckpt", "--batch_size", str(B), "--model", family])
    mods, (esd, dsd, lsd, gsd, lik) = _build(family, 64, 1, B, 3100)
    ckpt = {"encoder": mods[0], "decoder": mods[1], "frame_predictor": mods[2], "likelihood": lik, "gp_layer": gsd}
    g = generate_frames.Generator(opt, ckpt, torch.device(DEV))
    xs = [params.frames(3110, B, 1, 64)]
    eps = {i: params.normal(3120 + i, 90, B) for i in range(12, total)}
    enc_o, dec_o = _oracle_fns(family, 64, esd, dsd)
    idx = [0, 3, 49]
    got = g.gp_trigger_gen([xs[0].to(DEV)], indices=idx, total=total, depth=depth,
                           eps_by_step={k: v.to(DEV) for k, v in eps.items()}, keep_batch=True)
    unforced, both, memo = 0, [0, 0], {}      # memo: the oracle computes a (step, decisions so far) pair once for all indices
    for res in got:
        index = res["index"]
        dec = {i: (i in res["triggers"]) for i in range(12, total)}
        with torch.no_grad():
            ref = orc.gp_trigger_gen(xs, enc_o, dec_o, lsd, gsd, lik, index, eps, total=total, depth=depth, decisions=dec,
                                     guard=guard, memo=memo)
        # every decision the oracle took on its own is the HIP run's decision; forced ones are by construction
        assert ref["triggers"] == res["triggers"], (index, ref["triggers"], res["triggers"], ref["forced"])
        np.testing.assert_allclose(res["values"], ref["values"], rtol=2e-5)
        np.testing.assert_allclose(res["thresholds"], ref["thresholds"], rtol=2e-5)
        worst = max(rel_err(res["batch_frames"][t], ref["frames"][t]) for t in range(total))
        free = [i for i in range(12, total) if i not in ref["forced"]]
        unforced += len(free)
        both[0] += sum(1 for i in free if dec[i])
        both[1] += sum(1 for i in free if not dec[i])
        print(f"gp_trigger {family} depth {depth} index {index}: {len(res['triggers'])} triggers, {len(ref['forced'])} of "
              f"{total - 12} decisions inside the {guard:.0e} guard, frames rel err {worst:.2e}")
        assert worst < 1e-4, (index, worst)
    if depth != 1:
        assert unforced >= 0.5 * len(idx) * (total - 12) and min(both) >= 5, (unforced, both)
    # indices whose decisions on an already computed trigger-free rollout are that rollout's decisions reused it (their
    # frames / values / thresholds went through the same oracle comparison above)
    assert 1 <= g.trigger_rollouts_run <= len(idx)
    if all(not r["triggers"] for r in got):
        assert g.trigger_rollouts_run == 1


@pytest.mark.parametrize("inflight,share", [(0, True), (2, True), (2, False)])
def test_make_gifs_best_ssim_matches_oracle(inflight, share):
    """generate_frames.py:143-189,207: nsample rollouts with GP samples at i % 15 == 0, SSIM / PSNR per frame
    (utils.eval_seq), best sample per row = np.argsort(mean SSIM)[-1] - exact index match.  inflight = 0: the eager sample
    loop; 2: the sample body replayed as hipGraphs, two samples at a time (rollout.GraphedSampler) - with the prediction steps
    before the first trigger step run once per batch (share, the default) or once per sample."""
    import generate_frames
    B, n_past, n_eval, S = 3, 3, 20, 3
    opt = generate_frames.build_parser().parse_args(["--synthetic_ckpt", "--batch_size", str(B), "--model", "dcgan",
                                                     "--n_past", str(n_past), "--n_eval", str(n_eval),
                                                     "--inflight", str(inflight)] + ([] if share else ["--no_share_prefix"]))
    mods, (esd, dsd, lsd, gsd, lik) = _build("dcgan", 64, 1, B, 1800)
    ckpt = {"encoder": mods[0], "decoder": mods[1], "frame_predictor": mods[2], "likelihood": lik, "gp_layer": gsd}
    g = generate_frames.Generator(opt, ckpt, torch.device(DEV))
    xs = [params.frames(1810 + t, B, 1, 64) for t in range(n_eval)]
    eps = [{15: params.normal(1840 + s, 90, B)} for s in range(S)]
    enc_o, dec_o = _oracle_fns("dcgan", 64, esd, dsd)
    ssim = np.zeros((B, S, n_eval - n_past))
    psnr = np.zeros_like(ssim)
    with torch.no_grad():
        for s in range(S):
            fr = orc.rollout(xs, enc_o, dec_o, lsd, gsd, lik, n_past, n_eval, eps[s])
            ssim[:, s], psnr[:, s] = orc.eval_seq(xs[n_past:], fr[n_past:])
    ref_best = orc.best_ssim(ssim)
    res = g.make_gifs([t.to(DEV) for t in xs], S, eps_by_sample=[{15: e[15].to(DEV)} for e in eps])
    mine = res["ssim"].cpu().numpy()
    np.testing.assert_allclose(mine[:, :, :15 - n_past], ssim[:, :, :15 - n_past], atol=2e-6)   # before the GP sample
    np.testing.assert_allclose(mine, ssim, atol=1e-4)          # after it: fp32 GP solves (cond ~1e4) chained through the rollout
    np.testing.assert_allclose(res["psnr"].cpu().numpy(), psnr, atol=2e-2)
    # index bookkeeping proper: argsort(mean SSIM)[-1] on the SAME numbers must give the same index, bit for bit ...
    assert res["best"].tolist() == orc.best_ssim(mine)
    # ... and end to end wherever best and runner-up are further apart than the observed SSIM deviation
    dev_ = float(np.abs(mine.mean(2) - ssim.mean(2)).max())
    gaps = np.sort(ssim.mean(2), axis=1)
    decidable = [i for i in range(B) if gaps[i, -1] - gaps[i, -2] > 4 * dev_]
    assert len(decidable) >= 2, (gaps[:, -1] - gaps[:, -2], dev_)
    for i in decidable:
        assert int(res["best"][i]) == ref_best[i], (i, res["best"].tolist(), ref_best)
    if inflight:
        # the replayed sample body is the eager loop's arithmetic: same kernels on the same inputs, a second batch included
        xs2 = [params.frames(1870 + t, B, 1, 64).to(DEV) for t in range(n_eval)]
        eps_d = [{15: e[15].to(DEV)} for e in eps]
        for batch in ([t.to(DEV) for t in xs], xs2):
            a = g.make_gifs(batch, S, eps_by_sample=eps_d)
            g.opt.inflight = 0
            b = g.make_gifs(batch, S, eps_by_sample=eps_d)
            g.opt.inflight = inflight
            for k in ("samples", "ssim", "psnr", "best", "posterior"):
                assert torch.equal(a[k], b[k]), k
        # without base samples handed in every sample draws its own (torch's generator, per chain, outside the graphs):
        # all four samples of a batch differ from the trigger step on and agree before it
        r = g.make_gifs(xs2, 4)["samples"]
        for i in range(4):
            for j in range(i + 1, 4):
                assert torch.equal(r[i, :15], r[j, :15]) and not torch.equal(r[i, 15], r[j, 15]), (i, j)
        from dvg_amd import rollout
        share = share and rollout.SHARE_PREFIX           # (the module attribute turns the default off)
        assert g._sampler.share == share and g._sampler.t0 == (15 if share else n_past)


@pytest.mark.parametrize("family", ["vgg", "dcgan"])
def test_rollout_without_the_discarded_skip_stores_is_bit_identical(family):
    """rollout.ELIDE_SKIPS (default on): the skip tensors a rollout never reads - those of the conditioning frames before the
    last one, and of every predicted frame once the skip is frozen (generate_frames.py:154-157) - are not stored.  Frames of
    sample_rollout and posterior_rollout equal the run that stores everything, bit for bit, B = 32 (Winograd shapes)."""
    from dvg_amd import fused, ops, rollout
    mods, _ = _build(family, 64, 1, 32, 2900)
    for m in mods:
        m.to(DEV).eval()
    n_past, n_eval = 4, 9
    xs = [params.frames(2910 + t, 32, 1, 64).to(DEV) for t in range(n_eval)]
    eps = {i: params.normal(2920 + i, 90, 32).to(DEV) for i in range(n_past, n_eval)}
    out = {}
    for elide in (True, False):
        old = rollout.ELIDE_SKIPS
        rollout.ELIDE_SKIPS = elide
        fused.clear_skip_hoist_cache()
        ops.clear_skip_proj_cache()
        try:
            a = rollout.sample_rollout(*mods, xs, n_past, n_eval, period=3, eps_by_step=eps)
            b = rollout.posterior_rollout(*mods, xs, n_past, n_eval)
        finally:
            rollout.ELIDE_SKIPS = old
        out[elide] = (torch.stack(a), torch.stack(b))
    fused.clear_skip_hoist_cache()
    ops.clear_skip_proj_cache()
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])


@pytest.mark.parametrize("family", ["vgg", "dcgan"])
def test_make_gifs_shared_prefix_equals_the_per_sample_loop(family):
    """GraphedSampler's shared prefix (the prediction steps before the first GP trigger step once per batch) against the eager
    per-sample loop AND the per-sample graphs, bit for bit: frames, SSIM, PSNR, best index - at the bench's own step layout
    (10-in / 10-out: trigger at 15), for two batches through one sampler, and for a rollout that ends before the first
    trigger step (n_eval = 14: every sample is the prefix)."""
    import generate_frames
    from dvg_amd import ops, rollout
    B, S = 8, 4
    old, rollout.SHARE_PREFIX = rollout.SHARE_PREFIX, True     # (the flag is read per sampler)
    mods, (esd, dsd, lsd, gsd, lik) = _build(family, 64, 1, B, 1900)
    ckpt = {"encoder": mods[0], "decoder": mods[1], "frame_predictor": mods[2], "likelihood": lik, "gp_layer": gsd}
    for n_past, n_eval in ((10, 20), (10, 14)):
        eps = [{i: params.normal(1940 + 7 * s + i, 90, B).to(DEV) for i in range(n_past, n_eval) if i % 15 == 0} for s in range(S)]
        out = {}
        for name, extra in (("shared", ["--inflight", "3"]), ("per_sample", ["--inflight", "3", "--no_share_prefix"]),
                            ("eager", ["--inflight", "0"])):
            opt = generate_frames.build_parser().parse_args(["--synthetic_ckpt", "--batch_size", str(B), "--model", family,
                                                             "--n_past", str(n_past), "--n_eval", str(n_eval)] + extra)
            g = generate_frames.Generator(opt, ckpt, torch.device(DEV))
            # the samplers with chains in flight capture under the energy tile policy; the eager loop (one chain, latency tiles by
            # default) is run under the same policy here - across policies the frames agree to fp32 summation order only
            with ops.tile_policy(True):
                out[name] = [g.make_gifs([params.frames(1910 + 40 * b + t, B, 1, 64).to(DEV) for t in range(n_eval)], S,
                                         eps_by_sample=eps) for b in range(2)]
            if name == "shared":
                assert g._sampler.share and g._sampler.t0 == min(15, n_eval)
        for name in ("per_sample", "eager"):
            for a, b in zip(out["shared"], out[name]):
                for k in ("samples", "ssim", "psnr", "best", "posterior"):
                    assert torch.equal(a[k], b[k]), (family, n_past, n_eval, name, k)
    rollout.SHARE_PREFIX = old


def test_many_graph_holders_in_one_process_share_their_streams():
    """bench.py builds ~10 graph holders in one process (two families x (three chains + make_gifs) + C1).  torch hands streams out of
    a pool of 32 per device, round-robin: with one fresh torch.cuda.Stream() per chain and warm-up (r06 until the last day) the
    pool wrapped around, a chain landed on a stream torch also used elsewhere and hipGraphLaunch died with a segmentation
    fault (hip::Graph::UpdateStreams).  graphs.pooled_stream makes each stream once per process: 14 holders x (3 chains + 3 warm-ups)
    would have taken 84 streams; they must all replay, and give the eager rollout's frames."""
    from dvg_amd import graphs, ops
    from dvg_amd.rollout import ConcurrentRollouts, sample_rollout
    B, n_past, n_eval = 2, 2, 5
    mods, _ = _build("dcgan", 64, 1, B, 4100)
    for m in mods:
        m.to(DEV).eval()
    xs = [params.frames(4110 + t, B, 1, 64).to(DEV) for t in range(n_eval)]
    with ops.tile_policy(True):
        ref = sample_rollout(*mods, xs, n_past, n_eval, period=0)
    assert graphs.pooled_stream("chain", 1) is graphs.pooled_stream("chain", 1)
    assert graphs.pooled_stream("chain", 1) is not graphs.pooled_stream("chain", 2)
    holders = []
    for _ in range(14):
        cr = ConcurrentRollouts(*mods, xs, n_past, n_eval, inflight=3, period=0)
        holders.append(cr)
        assert all(a is b for a, b in zip(cr.streams, holders[0].streams))
    for cr in holders:
        for frames in cr.run(6):
            torch.cuda.synchronize()
            assert all(torch.equal(frames[t], ref[t]) for t in range(n_eval))
    assert len(graphs._streams) <= 8


def test_gaussian_encoder_matches_reference_golden(golden):
    """vgg_64.gaussian_encoder (vgg_64.py:108-159) on the HIP path against the outputs of the reference's own module."""
    import dvg_amd.models.vgg_64 as ours
    from tests.common import summarize
    net = ours.gaussian_encoder(90, 24, 1)
    net.load_state_dict(params.fill_state_dict(net.state_dict(), 180))
    net.to(DEV).eval()
    gz = golden["gaussian_encoder/zmle"]            # [z, mu, logvar, eps]
    eps = torch.from_numpy(gz[3]).to(DEV)
    net.reparameterize = lambda mu, logvar: eps * torch.exp(0.5 * logvar) + mu    # the reference's draw, replayed
    with torch.no_grad():
        z, mu, logvar, skips = net(params.frames(182, 3, 1, 64).to(DEV))
    assert rel_err(mu, torch.from_numpy(gz[1])) < 1e-4 and rel_err(logvar, torch.from_numpy(gz[2])) < 1e-4
    assert rel_err(z, torch.from_numpy(gz[0])) < 1e-4
    assert len(skips) == 4
    for i, sk in enumerate(skips):
        np.testing.assert_allclose(summarize(sk), golden[f"gaussian_encoder/skip{i}"], rtol=2e-4, atol=2e-3)
    # and with its own RNG draw: z = eps' * exp(logvar / 2) + mu for SOME standard-normal eps'
    del net.reparameterize
    torch.manual_seed(0)
    with torch.no_grad():
        z2, mu2, logvar2, _ = net(params.frames(182, 3, 1, 64).to(DEV))
    e2 = (z2 - mu2) / torch.exp(0.5 * logvar2)
    assert torch.equal(mu2, mu) and abs(float(e2.mean())) < 0.5 and 0.5 < float(e2.std()) < 1.5
