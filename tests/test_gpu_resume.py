"""GPU: `train.py --resume` - Trainer.state_dict / load_state_dict restore a training state exactly and through the existing
arena views, warm caches do not survive a load, the GP gradients that leak from one iteration into the next are part of the
state, a resumed run continues like the uninterrupted one (eager and as a hipGraph, Adam's device-side step counts included),
and the script resumes end to end with one rank and with two.

Shapes (the smallest at which the time-batched closures, forward_sequence and the fused losses all run): dcgan_64, batch 4,
n_past 2, n_future 2, g_dim 90, rnn_size 256, the in-repo synthetic smmnist.

Run-to-run stability is MEASURED here, not assumed (`_rel`, `test_continuation`): where two identical runs end bit-identical a
resumed run must be bit-identical to the uninterrupted one; where they do not, it may differ by at most twice what they do."""
import os

import pytest
import torch

from dvg_amd import train_state
from tests import train_harness

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DATA_SEED = 5


def _stream():
    import train
    from dvg_amd.data import make_batch_generator
    return train.BatchPrefetcher(make_batch_generator(train_harness.opt(), 4, DATA_SEED, torch.device(DEV)))


def _rel(a, b):
    """Largest parameter difference relative to the largest parameter magnitude, over the whole arena."""
    return float((a - b).abs().max()) / float(b.abs().max())


def _abs(a, b):
    return float((a - b).abs().max())


def _steps(tr):
    return {n: o.host_state()["steps"] for n, o in train_state.named_optimizers(tr)}


def _live(tr):
    """Clones of everything load_state_dict must reproduce, read from the LIVE Trainer (not from its state_dict)."""
    lo, hi = tr.rng_gp
    return {"p": tr.arena.p.clone(), "m": tr.arena.m.clone(), "v": tr.arena.v.clone(), "g_gp": tr.arena.g[lo:hi].clone(),
            "buffers": {k: b.clone() for k, b in train_state.named_buffers(tr)}, "steps": _steps(tr),
            "lrs": [g["lr"] for o in tr.optimizers() for g in o.param_groups], "scheduler": tr.scheduler.state_dict(),
            "torch_cpu": torch.get_rng_state().clone(), "torch_cuda": torch.cuda.get_rng_state(torch.device(DEV)).clone()}


@pytest.fixture(scope="module")
def source():
    """Trainer A after 3 eager iterations (the second scheduler step has moved the learning rate of the GP groups): its state
    dict, clones of its live state, the batches, and the arena after the 4th iteration of the UNINTERRUPTED run."""
    tr = train_harness.trainer(seed=3)
    gen = _stream()
    xs = [next(gen)() for _ in range(3)]
    tr.scheduler.step()
    for i, x in enumerate(xs):
        tr.iteration(x)
        if i == 0:
            tr.scheduler.step()
            tr.scheduler.step()
            tr.scheduler.step()          # milestone 3: lr of the GP groups x 0.1
    torch.rand(3)                        # both torch streams away from their seeds
    torch.rand(3, device=DEV)
    sd = tr.state_dict(epoch=1, train_gen=gen)
    live = _live(tr)
    x4 = next(gen)()
    tr.iteration(x4)
    torch.cuda.synchronize()
    return {"sd": sd, "live": live, "xs": xs, "x4": x4, "p_after": tr.arena.p.clone()}


def test_state_dict_owns_its_storage_and_names_what_it_holds(source):
    sd = source["sd"]
    assert sd["epoch"] == 1 and sd["global_step"] == 3 and sd["fingerprint"]["world"] == 1
    assert [e[0] for e in sd["fingerprint"]["layout"]] == ["gp", "gp", "frame_predictor", "decoder", "encoder"]

    def walk(o):
        if torch.is_tensor(o):
            yield o
        elif isinstance(o, dict):
            for v in o.values():
                yield from walk(v)
        elif isinstance(o, (list, tuple)):
            for v in o:
                yield from walk(v)
    tensors = list(walk(sd))
    assert len(tensors) > 20
    for t in tensors:
        assert t.untyped_storage().nbytes() == t.numel() * t.element_size()
    assert float(sd["arena"]["g_gp"].abs().max()) > 0          # the GP closure's gradients are there to be leaked


def test_round_trip_is_bit_exact_through_the_existing_views(source):
    sd, live = source["sd"], source["live"]
    tr = train_harness.trainer(seed=41)
    ptrs = [tr.arena.p.data_ptr(), tr.arena.g.data_ptr(), tr.arena.m.data_ptr(), tr.arena.v.data_ptr()]
    params = [p for m in tr.modules for p in m.parameters()]
    pp = [(p.data_ptr(), p.grad.data_ptr(), p._version) for p in params]
    bp = [(b.data_ptr(), b._version) for _, b in train_state.named_buffers(tr)]
    moments = [(o.state[p]["exp_avg"].data_ptr(), o.state[p]["exp_avg_sq"].data_ptr()) for o in tr.optimizers()
               for g in o.param_groups for p in g["params"]]
    assert not torch.equal(tr.arena.p, live["p"])
    assert tr.load_state_dict(sd) == 1
    got = _live(tr)
    for k in ("p", "m", "v", "g_gp", "torch_cpu", "torch_cuda"):
        assert torch.equal(got[k], live[k]), k
    assert set(got["buffers"]) == set(live["buffers"]) and len(got["buffers"]) > 10
    for k, b in live["buffers"].items():
        assert torch.equal(got["buffers"][k], b), k
    assert got["steps"] == live["steps"] and got["steps"]["encoder"][0][0] == 3 and got["steps"]["gp"][0][0] == 6
    assert got["lrs"] == live["lrs"] and got["lrs"][0] == 0.002 and got["lrs"][-1] == pytest.approx(0.0002)
    assert got["scheduler"] == live["scheduler"] and train_state.global_step(tr) == 3
    # the same views as before: nothing was re-pointed
    assert ptrs == [tr.arena.p.data_ptr(), tr.arena.g.data_ptr(), tr.arena.m.data_ptr(), tr.arena.v.data_ptr()]
    for p, (dp, gp, ver) in zip(params, pp):
        assert p.data_ptr() == dp and p.grad.data_ptr() == gp and p._version > ver
    for (_, b), (dp, ver) in zip(train_state.named_buffers(tr), bp):
        assert b.data_ptr() == dp and b._version > ver
    assert moments == [(o.state[p]["exp_avg"].data_ptr(), o.state[p]["exp_avg_sq"].data_ptr()) for o in tr.optimizers()
                       for g in o.param_groups for p in g["params"]]


def test_round_trip_through_a_file_and_refusal_of_another_layout(source, tmp_path):
    f = train_state.write(source["sd"], str(tmp_path), 0, 1)
    assert f.endswith("train_state.pth") and os.listdir(str(tmp_path)) == ["train_state.pth"]
    sd = train_state.read(f)
    tr = train_harness.trainer(seed=43)
    tr.load_state_dict(sd, path=f)
    assert torch.equal(tr.arena.p, source["live"]["p"]) and torch.equal(tr.arena.v, source["live"]["v"])
    other = dict(sd, fingerprint=dict(sd["fingerprint"], layout=sd["fingerprint"]["layout"][:-1]))
    with pytest.raises(SystemExit, match="train_state.pth: layout is .* in the file and .* in this run"):
        tr.load_state_dict(other, path=f)


def test_warm_caches_do_not_serve_the_old_weights(source):
    """Trainer B has trained and predicted - packed weights, Winograd-domain weights and BatchNorm folds of ITS parameters
    exist, keyed by parameter version - before A's state is loaded into it.  Its encoder and decoder must then compute
    exactly what a fresh Trainer computes after the same load, in training mode and in eval mode (the folds)."""
    sd, x = source["sd"], source["xs"][0]
    b = train_harness.trainer(seed=7)

    def forward(tr):
        out = []
        with torch.no_grad():
            for mode in (True, False):
                tr.encoder.train(mode)
                tr.decoder.train(mode)
                h, skips = tr.encoder(x[0])
                out += [h.clone(), tr.decoder([h, skips]).clone()] + [s.clone() for s in skips]
        tr.train_mode()
        return out
    b.iteration(x)
    stale = forward(b)
    b.load_state_dict(sd)
    fresh = train_harness.trainer(seed=8)
    fresh.load_state_dict(sd)
    got, want = forward(b), forward(fresh)
    assert len(got) == len(want) > 4
    for i, (u, v) in enumerate(zip(got, want)):
        assert torch.equal(u, v), i
    assert not torch.equal(stale[0], want[0])       # the control: B's own weights gave something else


def test_the_leaked_gp_gradients_are_state(source):
    """reference_gp_grad_leak (the default): train_model does not zero the GP optimiser's gradients, so what the last GP closure
    left in `.grad` enters the next optimizer.step().  Resumed Trainers that keep the saved range match each other and the
    uninterrupted run; one whose range is zeroed after the load gets other GP parameters.  Without the leak the range is
    zeroed by train_model anyway: both agree."""
    sd, x4 = source["sd"], source["x4"]

    def gp_after(seed, zero, leak=True):
        tr = train_harness.trainer(seed=seed)
        tr.reference_gp_grad_leak = leak
        tr.load_state_dict(sd)
        lo, hi = tr.rng_gp
        if zero:
            tr.arena.g[lo:hi].zero_()
        tr.train_model(x4)
        torch.cuda.synchronize()
        return tr.arena.p[lo:hi].clone()
    # the uninterrupted run: A's three iterations again, then the same train_model
    u = train_harness.trainer(seed=3)
    u.scheduler.step()
    for i, x in enumerate(source["xs"]):
        u.iteration(x)
        if i == 0:
            for _ in range(3):
                u.scheduler.step()
    lo, hi = u.rng_gp
    noise_state = _abs(u.arena.p[lo:hi], source["live"]["p"][lo:hi])     # the same three iterations, run twice
    u.train_model(x4)
    torch.cuda.synchronize()
    unint = u.arena.p[lo:hi].clone()
    kept, kept2, zeroed = gp_after(11, False), gp_after(12, False), gp_after(13, True)
    noise = max(_abs(kept2, kept), noise_state)
    print(f"\nGP parameters after one train_model from the saved state, largest absolute differences: resumed vs resumed "
          f"{_abs(kept2, kept):.3e}, resumed vs uninterrupted {_abs(kept, unint):.3e} (the two runs' states before it: "
          f"{noise_state:.3e}), zeroed vs resumed {_abs(zeroed, kept):.3e}")
    assert _abs(kept, unint) <= 2 * noise                        # == 0 where runs are bit-stable
    # one Adam step moves an entry by up to lr = 2e-4 here; fp32 rounding of parameters of magnitude ~1 is 1e-7
    assert _abs(zeroed, kept) > max(100 * noise, 1e-6)           # the saved gradients decide the next GP step
    a, b = gp_after(14, False, leak=False), gp_after(15, True, leak=False)
    assert _abs(a, b) <= 2 * noise
    assert _abs(a, kept) > max(100 * noise, 1e-6)


def _run(mode, n, seed=3, resume_after=None, load_seed=99):
    """n iterations from seed, eager or as GraphedIteration; resume_after = k: after k iterations the state goes through a file
    image into a FRESH Trainer with another seed, in front of a fresh data stream, which does the rest.  Both graph forms
    capture at the 4th iteration."""
    import io
    import train
    tr, gen = train_harness.trainer(seed=seed), _stream()
    step = tr.iteration if mode == "eager" else train.GraphedIteration(tr, warmup=3)
    tr.scheduler.step()
    for i in range(n):
        if resume_after is not None and i == resume_after:
            f = io.BytesIO()
            torch.save(tr.state_dict(epoch=0, train_gen=gen), f)
            f.seek(0)
            del tr, step
            tr, gen = train_harness.trainer(seed=load_seed), _stream()
            tr.load_state_dict(torch.load(f, weights_only=False), train_gen=gen)
            step = tr.iteration if mode == "eager" else train.GraphedIteration(tr, warmup=3 - resume_after)
        step(next(gen)())
    torch.cuda.synchronize()
    return tr, step


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_continuation(mode):
    """4 iterations in one go against 2 + (save, fresh Trainer, load) + 2 on the continued data stream.  A-versus-A is measured
    first: bit-identical runs demand a bit-identical continuation, otherwise twice their difference is allowed (one extra
    capture boundary).  Under the graph, Adam's bias correction after the resume: the device step counts read back after the
    first replay equal the host counts."""
    a1, _ = _run(mode, 4)
    p1, m1, v1 = a1.arena.p.clone(), a1.arena.m.clone(), a1.arena.v.clone()
    buf1 = {k: b.clone() for k, b in train_state.named_buffers(a1)}
    del a1
    a2, _ = _run(mode, 4)
    noise = _rel(a2.arena.p, p1)
    del a2
    b, step = _run(mode, 4, resume_after=2)
    got = _rel(b.arena.p, p1)
    print(f"\ncontinuation {mode}: A vs A {noise:.3e} ({'bit-identical' if noise == 0 else 'not bit-identical'}), "
          f"resumed vs A {got:.3e}")
    if noise == 0.0:
        assert torch.equal(b.arena.p, p1) and torch.equal(b.arena.m, m1) and torch.equal(b.arena.v, v1)
        for k, t in train_state.named_buffers(b):
            assert torch.equal(t, buf1[k]), k
    else:
        assert got <= 2 * noise
    assert _steps(b)["encoder"][0][0] == 4 and _steps(b)["decoder"][0][0] == 4
    assert _steps(b)["frame_predictor"][0][0] == 8 and _steps(b)["gp"] == [[8] * len(s) for s in _steps(b)["gp"]]
    if mode == "graph":
        assert not step.failed and step.graph is not None and step.calls == 2     # one eager warm-up, one capture + replay
        for name, o in train_state.named_optimizers(b):
            for gi, f in o._flat.items():
                assert int(f["tdev"]) == int(o.state[f["params"][0]]["step"]) == (4 if name in ("encoder", "decoder") else 8), name


def test_a_load_makes_a_captured_iteration_capture_again(source):
    """A Trainer that holds a captured graph: after load_state_dict the next call must not replay it (device step counts and
    packs of the old state) - it captures again, seeded from the restored host counts - and does what the uninterrupted run's
    4th iteration did."""
    import train
    tr = train_harness.trainer(seed=21)
    step = train.GraphedIteration(tr, warmup=1)
    tr.scheduler.step()
    step(source["xs"][0])
    step(source["xs"][1])
    old = step.graph
    assert old is not None and not step.failed
    tr.load_state_dict(source["sd"])
    step(source["x4"])
    torch.cuda.synchronize()
    assert not step.failed and step.graph is not None and step.graph is not old
    for name, o in train_state.named_optimizers(tr):
        for gi, f in o._flat.items():
            assert int(f["tdev"]) == int(o.state[f["params"][0]]["step"]) == (4 if name in ("encoder", "decoder") else 8), name
    # eager (the source) against a replay: the tolerance of test_graphed_iteration_matches_eager, not bit-identity
    assert torch.allclose(tr.arena.p, source["p_after"], rtol=2e-3, atol=2e-5)
    assert not torch.allclose(tr.arena.p, source["live"]["p"], rtol=2e-3, atol=2e-5)     # (an iteration moves them by more)


def test_end_to_end_resume_runs_exactly_the_missing_epoch(tmp_path, capsys):
    import train
    out = str(tmp_path)
    common = train_harness.ARGS + ["--epoch_size", "2", "--save_every", "1", "--output_path", out]
    train.main(common + ["--niter", "2"])
    first = capsys.readouterr().out
    assert "[00] mse loss" in first and "[01] mse loss" in first and "resumed from" not in first
    state = os.path.join(out, "train_state.pth")
    assert os.path.exists(state) and os.path.exists(os.path.join(out, "model.pth"))
    assert not os.path.exists(os.path.join(out, "sample_2.pt"))
    assert not [n for n in os.listdir(out) if ".tmp." in n]
    sd = train_state.read(state)
    assert sd["epoch"] == 2 and sd["global_step"] == 4 and sd[train_state.RANK_KEY]["plot_writer"] is not None
    model_before = open(os.path.join(out, "model.pth"), "rb").read()
    tr = train.main(common + ["--niter", "3", "--resume", out])
    second = capsys.readouterr().out
    assert f"resumed from {state}: epoch 2, global step 4\n" in second
    assert second.count("mse loss") == 1 and "[02] mse loss" in second
    assert os.path.exists(os.path.join(out, "sample_2.pt")) and os.path.exists(os.path.join(out, "sample_2.png"))
    assert train_state.global_step(tr) == 6 and tr.scheduler.last_epoch == 3
    sd = train_state.read(state)
    assert sd["epoch"] == 3 and sd["global_step"] == 6
    assert open(os.path.join(out, "model.pth"), "rb").read() != model_before      # model.pth is still written, beside it
    # nothing left to do: the loop does not run, nothing is trained or written
    train.main(common + ["--niter", "3", "--resume", state])
    third = capsys.readouterr().out
    assert "resumed from" in third and "mse loss" not in third


def test_two_ranks_save_and_resume_and_one_rank_is_refused(tmp_path):
    """Two ranks on one GPU over gloo (the rehearsal switches of tests/test_gpu_multirank.py; fresh child processes): the shared
    part is written once, what differs per rank beside it; the resumed run ends with identical parameters on both ranks; the
    same state is refused by a single process."""
    out = str(tmp_path)
    args = ["--model", "dcgan", "--dataset", "smmnist", "--n_past", "2", "--n_future", "2", "--n_eval", "4", "--batch_size", "8",
            "--epoch_size", "2", "--save_every", "1", "--no_images", "--output_path", out, "--print_param_checksum"]

    def run(ranks, extra):
        return train_harness.run_train_py(args + extra, ranks=ranks, env=train_harness.REHEARSAL)

    def checksums(r):
        return {ln.split()[1]: ln.split()[-2:] for ln in r.stdout.splitlines() if "param checksum" in ln}
    r = run(2, ["--niter", "2"])
    assert r.returncode == 0, r.stderr[-2000:]
    saved = checksums(r)
    assert sorted(n for n in os.listdir(out) if n.startswith("train_state")) == \
        ["train_state.pth", "train_state.rank0.pth", "train_state.rank1.pth"]
    r = run(2, ["--niter", "3", "--resume", out])
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("resumed from") == 1 and "epoch 2, global step 4" in r.stdout
    assert r.stdout.count("mse loss") == 1 and "[02] mse loss" in r.stdout
    two = checksums(r)
    assert set(two) == {"0", "1"} and two["0"] == two["1"], two
    assert two["0"] != saved["0"]                                 # an epoch was trained on top of the saved parameters
    r = run(1, ["--niter", "3", "--resume", out])
    assert r.returncode != 0 and "world is 2 in the file and 1 in this run" in r.stderr and "mse loss" not in r.stdout
