"""GPU: the GRU / RNN frame predictors (--predictor gru|rnn) - dvg_gru_cell, dvg_gru_cell_pre, dvg_rnn_cell and dvg_gru_gates_bwd
against the fp64 restatement tests/gru_ref.py, the modules against the reference's own outputs (tests/golden/reference_gru.npz),
step-by-step and sequence-form BPTT against fp64 autograd, the rollouts (eager against their hipGraph forms, the trigger's state
hand-over), training eager / graphed / resumed, and run-to-run determinism of the new kernels.

Bars: the project's own for the LSTM against fp64 - 1e-5 for a cell's forward, 2e-5 for gradients (about 30 x torch's fp32 error on
these shapes: tests/test_gru_host.py shows torch's fp32 cells inside them and every planted defect of gru_ref outside)."""
import io
import os

import numpy as np
import pytest
import torch

from oracle import params
from tests import gru_ref, train_harness
from tests.common import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_BAR, GRAD_BAR = 1e-5, 2e-5
CELL_SHAPES = [(5, 64), (33, 64), (9, 128), (64, 256), (5, 256)]
HERE = os.path.dirname(os.path.abspath(__file__))


def cell_case(B, H, gates, seed=600):
    x, h = (params.normal(seed + i, B, H, scale=0.6) for i in range(2))
    w_ih, w_hh = (params.normal(seed + 2 + i, gates * H, H, scale=1.0 / H ** 0.5) for i in range(2))
    b_ih, b_hh = (params.normal(seed + 4 + i, gates * H, scale=0.3) for i in range(2))
    return x, h, w_ih, w_hh, b_ih, b_hh


def dev(ts):
    return [t.to(DEV) for t in ts]


@pytest.mark.parametrize("B,H", CELL_SHAPES)
def test_gru_and_rnn_cells_against_fp64(B, H):
    """dvg_gru_cell (h' and the saved r, z, n, hn, slice by slice), dvg_gru_cell_pre against it, dvg_rnn_cell; two calls on the same
    inputs are bit-equal."""
    from dvg_amd import ops
    args = cell_case(B, H, 3)
    h_ref, acts_ref = gru_ref.gru_cell(*[a.double() for a in args])
    x, h, w_ih, w_hh, b_ih, b_hh = dev(args)
    h2, acts = ops.gru_cell(x, h, w_ih, w_hh, b_ih, b_hh, want_acts=True)
    errs = {"h": rel_err(h2, h_ref)}
    for k, name in enumerate(("r", "z", "n", "hn")):
        errs[name] = rel_err(acts[:, k * H:(k + 1) * H], acts_ref[:, k * H:(k + 1) * H])
    print(f"\ngru_cell B={B} H={H}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < FWD_BAR, errs
    assert torch.equal(ops.gru_cell(x, h, w_ih, w_hh, b_ih, b_hh), h2)            # no acts requested: the same h'
    again = ops.gru_cell(x, h, w_ih, w_hh, b_ih, b_hh, want_acts=True)
    assert torch.equal(again[0], h2) and torch.equal(again[1], acts)
    # the teacher-forced form: the input half handed over, b_hr and b_hz added by the caller, b_hn with the kernel
    bias = b_ih.clone()
    bias[:2 * H] += b_hh[:2 * H]
    pre = ops.gemm_nt(x, w_ih, None, bias)
    h3, acts3 = torch.empty_like(h2), torch.empty_like(acts)
    ops.gru_cell_pre(pre, h, w_hh, b_hh[2 * H:], h3, acts3)
    e_pre = max(rel_err(h3, h2), rel_err(acts3, acts))
    print(f"gru_cell_pre vs gru_cell: {e_pre:.2e}; vs fp64 {rel_err(h3, h_ref):.2e}")
    assert e_pre < 2e-6 and rel_err(h3, h_ref) < FWD_BAR
    h4, acts4 = torch.empty_like(h2), torch.empty_like(acts)
    ops.gru_cell_pre(pre, h, w_hh, b_hh[2 * H:], h4, acts4)
    assert torch.equal(h4, h3) and torch.equal(acts4, acts3)
    # nn.RNNCell
    rargs = cell_case(B, H, 1, seed=620)
    r_ref = gru_ref.rnn_cell(*[a.double() for a in rargs])
    rd = dev(rargs)
    r2 = ops.rnn_cell(*rd)
    print(f"rnn_cell: {rel_err(r2, r_ref):.2e}")
    assert rel_err(r2, r_ref) < FWD_BAR
    assert torch.equal(ops.rnn_cell(*rd), r2)


@pytest.mark.parametrize("B,H", [(21, 256), (5, 64)])
def test_gru_gates_bwd_against_fp64(B, H):
    """dGi, dGh, dh_prev with both, one and the other of dh_a / dh_b, h_prev NULL bit-equal to explicit zeros, no dh_prev
    requested, caller-owned output buffers; bit-equal across two calls."""
    from dvg_amd import ops
    args = cell_case(B, H, 3, seed=640)
    _, acts_ref = gru_ref.gru_cell(*[a.double() for a in args])
    da, db = params.normal(650, B, H), params.normal(651, B, H)
    h_prev = args[1]
    acts = acts_ref.float().to(DEV)
    acts_ref = acts.double().cpu()             # the fp32 values the kernel reads
    for a, b in ((da, db), (da, None), (None, db)):
        d = (0 if a is None else a.double()) + (0 if b is None else b.double())
        ref = gru_ref.gates_bwd(d, acts_ref, h_prev.double())
        got = ops.gru_gates_bwd(None if a is None else a.to(DEV), None if b is None else b.to(DEV), acts, h_prev.to(DEV))
        errs = [rel_err(g, r) for g, r in zip(got, ref)]
        print(f"\ngru_gates_bwd B={B} H={H} a={a is not None} b={b is not None}: dGi {errs[0]:.2e} dGh {errs[1]:.2e} dh_prev {errs[2]:.2e}")
        assert max(errs) < GRAD_BAR, errs
        again = ops.gru_gates_bwd(None if a is None else a.to(DEV), None if b is None else b.to(DEV), acts, h_prev.to(DEV))
        assert all(torch.equal(u, v) for u, v in zip(got, again))
    # the zero initial state: NULL h_prev == explicit zeros, bit for bit; and against fp64
    z0 = ops.gru_gates_bwd(da.to(DEV), db.to(DEV), acts, None)
    z1 = ops.gru_gates_bwd(da.to(DEV), db.to(DEV), acts, torch.zeros(B, H, device=DEV))
    assert all(torch.equal(u, v) for u, v in zip(z0, z1))
    ref0 = gru_ref.gates_bwd(da.double() + db.double(), acts_ref, None)
    assert max(rel_err(g, r) for g, r in zip(z0, ref0)) < GRAD_BAR
    # no dh_prev requested; outputs into the caller's buffers (slices of a sequence's buffers)
    full = ops.gru_gates_bwd(da.to(DEV), db.to(DEV), acts, h_prev.to(DEV))
    gi, gh, none = ops.gru_gates_bwd(da.to(DEV), db.to(DEV), acts, h_prev.to(DEV), want_dh_prev=False)
    assert none is None and torch.equal(gi, full[0]) and torch.equal(gh, full[1])
    big_i = torch.full((3 * B, 3 * H), 7.0, device=DEV)
    big_h = torch.full((3 * B, 3 * H), 7.0, device=DEV)
    dhp = torch.full((B, H), 7.0, device=DEV)
    ops.gru_gates_bwd(da.to(DEV), db.to(DEV), acts, h_prev.to(DEV), big_i[B:2 * B], big_h[B:2 * B], dhp)
    assert torch.equal(big_i[B:2 * B], full[0]) and torch.equal(big_h[B:2 * B], full[1]) and torch.equal(dhp, full[2])
    assert bool((big_i[:B] == 7).all()) and bool((big_i[2 * B:] == 7).all()) and bool((big_h[:B] == 7).all()) \
        and bool((big_h[2 * B:] == 7).all())


@pytest.mark.parametrize("kind", ["gru", "rnn"])
def test_modules_match_the_reference_golden(kind):
    """3 steps of the reference's gru / rnn (tests/golden/make_golden_gru.py) on the GPU: outputs and final states; and
    step_state_only advances the state exactly as a full call."""
    import dvg_amd.models.lstm as ours
    golden = np.load(os.path.join(HERE, "golden", "reference_gru.npz"))
    seed = {"gru": 500, "rnn": 520}[kind]
    net = getattr(ours, kind)(90, 90, 64, 2, 5)
    sd = params.fill_state_dict(net.state_dict(), seed)
    net.load_state_dict(sd)
    net.to(DEV)
    xs = [params.normal(seed + 10 + t, 5, 90, scale=0.5).to(DEV) for t in range(3)]
    sd64 = {k: v.double() for k, v in sd.items()}
    hid64 = gru_ref.init_hidden(5, 64, 2)
    with torch.no_grad():
        net.hidden = net.init_hidden()
        for t in range(3):
            y = net(xs[t])
            y64 = gru_ref.module_step(xs[t].double().cpu(), sd64, hid64, kind)
            assert rel_err(y, torch.from_numpy(golden[f"{kind}/y"][t])) < FWD_BAR, t
            assert rel_err(y, y64) < FWD_BAR, t
        final = [h.clone() for h in net.hidden]
        for i in range(2):
            assert rel_err(final[i], torch.from_numpy(golden[f"{kind}/h{i}"])) < FWD_BAR
        net.hidden = net.init_hidden()
        for t in range(3):
            net.step_state_only(xs[t])
        assert all(torch.equal(a, b) for a, b in zip(net.hidden, final))
        assert all(a is b for a, b in zip(net.state_tensors(), net.hidden))


def _module_bptt(kind, B, S, seq, seed=700):
    import dvg_amd.models.lstm as ours
    net = getattr(ours, kind)(90, 90, 256, 2, B)
    sd = params.fill_state_dict(net.state_dict(), seed)
    net.load_state_dict(sd)
    net.to(DEV)
    xs = torch.stack([params.normal(seed + 10 + t, B, 90, scale=0.5) for t in range(S)])
    ws = torch.stack([params.normal(seed + 40 + t, B, 90) for t in range(S)])
    xd = xs.to(DEV).requires_grad_(True)
    net.hidden = net.init_hidden()
    if seq:
        assert ours.sequence_applies(net)
        y = ours.forward_sequence(net, xd)
        assert net.hidden is None
    else:
        y = torch.stack([net(xd[t]) for t in range(S)])
    (y * ws.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    g = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    g["x"] = xd.grad.detach().clone()
    return sd, xs, ws, y.detach().clone(), g


@pytest.mark.parametrize("kind,B,S", [("gru", 6, 3), ("gru", 16, 4), ("rnn", 6, 3)])
def test_bptt_against_fp64_autograd(kind, B, S):
    """A 2-layer predictor (90, 90, 256) step by step against fp64 autograd of gru_ref: outputs, all parameter gradients and the
    input gradient; for the gru also the sequence form (autograd._GRUSequence) against step-by-step: 2e-6 outputs, 2e-5
    gradients, as for the LSTM."""
    import dvg_amd.models.lstm as ours
    sd, xs, ws, y, g = _module_bptt(kind, B, S, False)
    y64, g64 = gru_ref.bptt(sd, xs, ws, kind, 2)
    errs = {k: rel_err(g[k], g64[k]) for k in g64}
    print(f"\n{kind} BPTT B={B} S={S} vs fp64: y {rel_err(y, y64):.2e} worst grad {max(errs, key=errs.get)} {max(errs.values()):.2e}")
    assert set(g) == set(g64) and len(g) == 13
    assert rel_err(y, y64) < FWD_BAR
    for k, e in errs.items():
        assert e < GRAD_BAR, (k, e)
    if kind == "rnn":
        assert not ours.sequence_applies(getattr(ours, kind)(90, 90, 256, 2, B))
        return
    _, _, _, ys, gs = _module_bptt(kind, B, S, True)
    errs = {k: rel_err(gs[k], g[k]) for k in g}
    print(f"{kind} sequence vs step-by-step: y {rel_err(ys, y):.2e} worst grad {max(errs, key=errs.get)} {max(errs.values()):.2e}")
    assert ys.shape == (S, B, 90) and rel_err(ys, y) < 2e-6
    for k, e in errs.items():
        assert e < GRAD_BAR, (k, e)
    for k in g64:
        assert rel_err(gs[k], g64[k]) < GRAD_BAR, k


@pytest.mark.parametrize("kind,seq", [("gru", False), ("gru", True), ("rnn", False)])
def test_in_place_gradients_equal_the_ones_returned_to_autograd(kind, seq):
    """Parameter gradients written into `.grad` by the kernels (one batched dW GEMM per backward pass, per use, in batches of
    two) against the same gradients returned to autograd (autograd.DIRECT_PARAM_GRADS = False), accumulated over two backward
    passes: 2e-5, as for the LSTM."""
    from dvg_amd import autograd as ag
    import dvg_amd.models.lstm as ours
    res = {}
    old_dense = ag.DENSE_BATCH
    xs = torch.stack([params.normal(2310 + t, 6, 90, scale=0.5) for t in range(3)]).to(DEV)
    for direct in (True, False, "per_use", "batch2"):
        ag.DIRECT_PARAM_GRADS = direct is not False
        ag.DENSE_BATCH = {"per_use": 1, "batch2": 2}.get(direct, old_dense)
        try:
            net = getattr(ours, kind)(90, 90, 128, 2, 6)
            net.load_state_dict(params.fill_state_dict(net.state_dict(), 2300))
            net.to(DEV)
            for rep in range(2):
                net.hidden = net.init_hidden()
                y = ours.forward_sequence(net, xs) if seq else torch.stack([net(xs[t]) for t in range(3)])
                (y ** 2).sum().backward()
            res[direct] = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
            assert not ag._dense_queues
        finally:
            ag.DIRECT_PARAM_GRADS, ag.DENSE_BATCH = True, old_dense
    for k, g in res[False].items():
        for mode in (True, "per_use", "batch2"):
            assert float((res[mode][k] - g).abs().max()) <= 2e-5 * max(float(g.abs().max()), 1e-20) + 1e-9, (k, mode)


def test_gru_sequence_refuses_a_parameter_changed_between_forward_and_backward():
    import dvg_amd.models.lstm as ours
    net = ours.gru(90, 90, 64, 1, 4).to(DEV)
    y = ours.forward_sequence(net, torch.zeros(2, 4, 90, device=DEV))
    with torch.no_grad():
        net.gru[0].weight_hh.mul_(0.5)
    with pytest.raises(RuntimeError, match="modified in place"):
        y.sum().backward()


def _rollout_modules(B, seed, kind="gru"):
    import dvg_amd.models.lstm as ours
    from tests.test_gpu_configs import _build
    mods, (esd, dsd, lsd, gsd, lik) = _build("dcgan", 64, 1, B, seed)
    fp = getattr(ours, kind)(90, 90, 256, 2, B)
    fp.load_state_dict(params.fill_state_dict(fp.state_dict(), seed + 2))
    return [mods[0], mods[1], fp, mods[3], mods[4]], gsd, lik


def test_rollouts_with_a_gru_eager_against_their_graphs():
    """dcgan_64, B = 4, n_past 2, n_eval 5: sample_rollout with a gru predictor against GraphedRollout (a GP draw at step 3) and
    make_gifs' eager loop against its GraphedSampler: bit-equal."""
    import generate_frames
    from dvg_amd.rollout import GraphedRollout, sample_rollout
    B, n_past, n_eval = 4, 2, 5
    mods, gsd, lik = _rollout_modules(B, 2100)
    for m in mods:
        m.to(DEV).eval()
    xs = [params.frames(2110 + t, B, 1, 64).to(DEV) for t in range(n_eval)]
    eps = {3: params.normal(2120, 90, B).to(DEV)}
    ref = sample_rollout(*mods, xs, n_past, n_eval, period=3, eps_by_step=eps)
    assert len(mods[2].hidden) == 2 and all(torch.is_tensor(h) for h in mods[2].hidden)
    gr = GraphedRollout(*mods, xs, n_past, n_eval, period=3)
    got = gr(xs, eps)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    assert not torch.equal(ref[3], ref[4])
    out = {}
    ckpt = {"encoder": mods[0], "decoder": mods[1], "frame_predictor": mods[2], "likelihood": lik, "gp_layer": gsd}
    for name, inflight in (("graph", "2"), ("eager", "0")):
        opt = generate_frames.build_parser().parse_args(["--synthetic_ckpt", "--batch_size", str(B), "--model", "dcgan", "--n_past",
                                                         str(n_past), "--n_eval", str(n_eval), "--inflight", inflight])
        g = generate_frames.Generator(opt, ckpt, torch.device(DEV))
        from dvg_amd import ops
        with ops.tile_policy(True):        # the sampler's chains capture under the energy tiles: compare like with like
            out[name] = g.make_gifs(xs, 2)
    for k in ("samples", "ssim", "psnr", "best", "posterior"):
        assert torch.equal(out["graph"][k], out["eager"][k]), k


@pytest.mark.parametrize("depth,expect", [(-1e6, "all"), (1e6, "none")])
def test_trigger_hands_a_gru_state_over(depth, expect):
    """GraphedTrigger with B = 4 (above the probe index 3) and total = warm-up + 3 against the eager trigger_body: a threshold far
    below every value forces a trigger at every step (the GP sample is decoded and the OLD state survives gp_trigger_select), one
    far above forces none (the predictor's output and the NEW state)."""
    import generate_frames
    from dvg_amd.rollout import trigger_body, trigger_log, trigger_warmup
    B, warmup, total = 4, 12, 15
    mods, gsd, lik = _rollout_modules(B, 2200)
    ckpt = {"encoder": mods[0], "decoder": mods[1], "frame_predictor": mods[2], "likelihood": lik, "gp_layer": gsd}
    opt = generate_frames.build_parser().parse_args(["--synthetic_ckpt", "--batch_size", str(B), "--model", "dcgan"])
    g = generate_frames.Generator(opt, ckpt, torch.device(DEV))
    x0 = params.frames(2210, B, 1, 64).to(DEV)
    eps = {i: params.normal(2220 + i, 90, B).to(DEV) for i in range(warmup, total)}
    res = {}
    for graph in (True, False):
        res[graph] = g.gp_trigger_gen([x0], indices=[1], total=total, depth=depth, eps_by_step=eps, keep_batch=True,
                                      graph=graph)[0]
    want = list(range(warmup, total)) if expect == "all" else []
    assert res[True]["triggers"] == res[False]["triggers"] == want
    np.testing.assert_allclose(res[True]["values"], res[False]["values"], rtol=1e-5)
    for t in range(total):
        assert torch.equal(res[True]["batch_frames"][t], res[False]["batch_frames"][t]), t
    # the state after the body, on the eager path: the warm-up's when every step triggered, three steps further otherwise
    mods = (g.encoder, g.decoder, g.frame_predictor, g.gp_layer, g.likelihood)
    with torch.no_grad():
        state = trigger_warmup(*mods, x0, warmup)
        before = [t.clone() for t in state["hidden"]]
        assert len(before) == 2 and all(torch.is_tensor(t) for t in before)
        e = torch.stack([eps[i] for i in range(warmup, total)])
        trigger_body(state, *mods, state["norms"][:, 1].clone(), 2 + 0.01 * depth, e, trigger_log(total, x0.device), warmup, total)
    after = g.frame_predictor.state_tensors()
    same = [torch.equal(a, b) for a, b in zip(after, before)]
    assert all(same) if expect == "all" else not any(same)


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
def gru_eager():
    """Two eager iterations with --predictor gru, shared by the tests below: (parameters, losses)."""
    import dvg_amd.models.lstm as ours
    a, la = _train(["--predictor", "gru"], 2)
    assert isinstance(a.frame_predictor, ours.gru) and a._lstm_seq_applies()          # the sequence form runs
    assert a.state_dict(epoch=0)["fingerprint"]["predictor"] == "gru"
    return a.arena.p.clone(), la


def test_training_with_a_gru_eager_against_graphed(gru_eager):
    """dcgan_64, B = 4, 2-in / 2-out, --predictor gru: two iterations eager against GraphedIteration - losses and parameters at the
    bars of test_graphed_iteration_matches_eager, the parameter checksums (--print_param_checksum's figures) printed."""
    pa, la = gru_eager
    g, lg = _train(["--predictor", "gru"], 2, graphed=True)
    for u, v in zip(la, lg):
        for s, t in zip(u, v):
            assert abs(s - t) <= 2e-4 * max(1.0, abs(s)), (la, lg)
    assert torch.allclose(g.arena.p, pa, rtol=2e-3, atol=2e-5)
    cs = lambda p: (float(p.double().sum()), float(p.double().abs().sum()))        # noqa: E731
    print(f"\ngru training: losses {la}; checksum eager {cs(pa)} graphed {cs(g.arena.p)}")
    assert abs(cs(g.arena.p)[1] - cs(pa)[1]) <= 2e-3 * cs(pa)[1]


def test_training_with_a_gru_resumes_exactly(gru_eager):
    """A --resume round trip through a file image into a fresh Trainer continues bit for bit where two identical runs are
    bit-identical (measured here), within twice their difference otherwise; a state of another predictor is refused naming the
    field."""
    pa, la = gru_eager
    extra = ["--predictor", "gru"]
    a2, _ = _train(extra, 2)
    noise = float((a2.arena.p - pa).abs().max())
    del a2
    r, lr_ = _train(extra, 2, resume_after=1)
    got = float((r.arena.p - pa).abs().max())
    print(f"\nresume: A vs A {noise:.3e}, resumed vs A {got:.3e}")
    if noise == 0.0:
        assert torch.equal(r.arena.p, pa) and lr_ == la
    else:
        assert got <= 2 * noise
    other = train_harness.trainer(["--predictor", "rnn"], seed=5)
    with pytest.raises(SystemExit, match="predictor is 'gru' in the file and 'rnn' in this run"):
        other.load_state_dict(r.state_dict(epoch=0))


def test_predictor_lstm_is_the_run_without_the_flag():
    """--predictor lstm against no flag: the same class, the same fingerprint, the same parameters after two iterations (bit for
    bit where two identical runs are; measured)."""
    import dvg_amd.models.lstm as ours
    a, la = _train([], 2)
    assert type(a.frame_predictor) is ours.lstm and "predictor" not in a.state_dict(epoch=0)["fingerprint"]
    pa = a.arena.p.clone()
    del a
    a2, _ = _train([], 2)
    noise = float((a2.arena.p - pa).abs().max())
    del a2
    b, lb = _train(["--predictor", "lstm"], 2)
    assert type(b.frame_predictor) is ours.lstm and "predictor" not in b.state_dict(epoch=0)["fingerprint"]
    got = float((b.arena.p - pa).abs().max())
    print(f"\n--predictor lstm vs no flag: A vs A {noise:.3e}, flag vs A {got:.3e}")
    if noise == 0.0:
        assert torch.equal(b.arena.p, pa) and lb == la
    else:
        assert got <= 2 * noise


def test_rnn_trains_step_by_step():
    """--predictor rnn: no sequence form; one iteration eager moves every parameter of the predictor and leaves finite losses."""
    import dvg_amd.models.lstm as ours
    tr = train_harness.trainer(["--predictor", "rnn"], seed=3)
    assert isinstance(tr.frame_predictor, ours.rnn) and not tr._lstm_seq_applies()
    before = {k: p.detach().clone() for k, p in tr.frame_predictor.named_parameters()}
    x = train_harness.make_batches(1)[0]
    torch.manual_seed(77)
    out = tr.iteration(x)
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in out)
    for k, p in tr.frame_predictor.named_parameters():
        assert bool(torch.isfinite(p).all()) and not torch.equal(p, before[k]), k
