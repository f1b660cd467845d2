"""GPU: the weight average - dvg_ema_update (ema.hip), dvg_amd.ema.WeightAverage, and train.py --ema_decay through the Trainer, a
hipGraph, a resume, model_ema.pth, generate_frames.py --ema and two ranks.  fp64 restatement: tests/ema_ref.py.

Bars (derived, not measured).  The average after K updates: K 2^-23 max(|p|, |e|) absolute - each update rounds p - e once and the
fmaf once, and the weight carries one fp32 rounding; the reference chain is ema_ref.update on the fp32 values, rounded to fp32
after every update like the stored average.  The two sums against numpy fp64 on the fp32 values the kernel stored: n 2^-52
relative (squares do not cancel; only the summation order differs).  Everything that compares two runs of the same kernel on the
same inputs is bit-for-bit.

Shapes: n around the 8 192-float chunk (a one-vector launch, two vectors, the last float4 of a chunk, the first of the next, several
chunks and a last workgroup with a single float4, 2^20 + 12); dcgan_64 at batch 4, n_past 2, n_future 2 for the Trainer."""
import io
import os
import types

import numpy as np
import pytest
import torch

from tests import ema_ref as ref, train_harness

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = ref.CHUNK
SIZES = [4, 8, CHUNK - 4, CHUNK, CHUNK + 4, 3 * CHUNK + 8, 2 ** 20 + 12]
KEYS = {"encoder", "decoder", "frame_predictor", "likelihood", "gp_layer", "gp_layer_optimizer", "opt"}


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
def _average(p, decay, e0=None):
    """A WeightAverage over the flat tensor p (a stand-in arena that has only `.p`); e0: the starting average (default: p)."""
    from dvg_amd.ema import WeightAverage
    avg = WeightAverage(decay, types.SimpleNamespace(p=p))
    if e0 is not None:
        avg.e.copy_(e0)
    return avg


def _randn(n, seed):
    return torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2000 + seed))


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("decay", [0.0, 0.9, 0.9999])
def test_updates_against_fp64(decay):
    """50 updates with another random p each, the count advanced between the launches (the warm-up branch (1 + k) / (10 + k) and
    the constant branch are both crossed: 0.9 is reached at k = 80 > 50, 0 at once, so 0.9 and 0.9999 stay in the warm-up and 0
    is constant); checked after K = 1, 3 and 50 updates."""
    from dvg_amd import ops
    worst_e, worst_s = 0.0, 0.0
    for n in SIZES:
        p = _randn(n, 0)
        avg = _average(p, decay, e0=_randn(n, 1))
        assert avg.partials.numel() == 2 * ref.blocks(n) == 2 * ops.ema_update_blocks(n)
        want = avg.e.cpu().numpy()
        top = 0.0
        for k in range(50):
            p.copy_(_randn(n, 10 + k))
            pk = p.cpu().numpy()
            avg.update()
            want = ref.update(want, pk, decay, k).astype(np.float32)
            top = max(top, float(np.abs(pk).max()), float(np.abs(want).max()))
            K = k + 1
            if K not in (1, 3, 50):
                continue
            got = avg.e.cpu().numpy()
            assert int(avg.updates) == K
            err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
            bar = K * 2.0 ** -23 * top
            worst_e = max(worst_e, err / bar)
            assert err <= bar, (decay, n, K, err, bar)
            # the sums: numpy fp64 on the fp32 average the kernel stored
            part = avg.partials.cpu().numpy()
            pw = ref.chunk_sums(pk, got)
            assert part.shape == pw.shape
            off, allowed = np.abs(part - pw), min(n, CHUNK) * 2.0 ** -52 * pw      # (a sum may be exactly 0: p == e' everywhere)
            worst_s = max(worst_s, float((off[pw > 0] / allowed[pw > 0]).max()))
            assert np.all(off <= allowed), (decay, n, K, float((off - allowed).max()))
            tot, tw = part.reshape(-1, 2).sum(0), ref.sums(pk, got)
            assert all(abs(a - b) <= n * 2.0 ** -52 * b for a, b in zip(tot, tw)), (decay, n, K, tot, tw)
    print(f"\nema decay {decay}: worst |e - fp64| / bar {worst_e:.3f}, worst partial-sum error / bar {worst_s:.3f}")


def test_both_branches_of_the_schedule_in_one_chain():
    """decay = 0.5: the warm-up for k < 8, the constant from k = 8 on - twelve updates cross the switch."""
    n = CHUNK + 4
    p = _randn(n, 3)
    avg = _average(p, 0.5, e0=torch.zeros(n, device=DEV))
    want, top = np.zeros(n, dtype=np.float32), 0.0
    for k in range(12):
        p.copy_(_randn(n, 40 + k))
        avg.update()
        want = ref.update(want, p.cpu().numpy(), 0.5, k).astype(np.float32)
        top = max(top, float(p.abs().max()), float(np.abs(want).max()))
    err = float(np.abs(avg.e.cpu().numpy().astype(np.float64) - want).max())
    assert err <= 12 * 2.0 ** -23 * top and avg.read_lag()["decay_eff"] == 0.5
    assert ref.decay_at(0.5, 7) < 0.5 == ref.decay_at(0.5, 8)


def test_constant_parameter_eager_and_replayed():
    """p = c, e_0 = 0, twelve updates with decay 0.999: the closed form c (1 - prod d_k) of tests/test_ema_host.py; the twelve
    updates eagerly and as ONE captured update replayed twelve times agree bit for bit - a replay reads the advanced count."""
    from dvg_amd import graphs
    c, n, K = 0.75, CHUNK + 8, 12
    p = torch.full((n,), c, device=DEV)
    eager = _average(p, 0.999, e0=torch.zeros(n, device=DEV))
    for _ in range(K):
        eager.update()
    want = ref.closed_form(c, 0.999, K)
    got = eager.e.cpu().numpy().astype(np.float64)
    assert float(np.abs(got - want).max()) <= K * 2.0 ** -23 * c, (got[0], want)
    assert float(eager.e.min()) == float(eager.e.max())              # every element took the same path
    replayed = _average(p, 0.999, e0=torch.zeros(n, device=DEV))
    torch.cuda.synchronize()
    with graphs.capturing() as graph:
        replayed.update()
    assert int(replayed.updates) == 0                                # a capture executes nothing
    for _ in range(K):
        graph.replay()
    torch.cuda.synchronize()
    assert int(replayed.updates) == K == int(eager.updates)
    assert torch.equal(_bits(replayed.e), _bits(eager.e)) and torch.equal(_bits(replayed.partials), _bits(eager.partials))
    d = replayed.read_lag()
    assert d["updates"] == K and d["decay_eff"] == ref.decay_at(0.999, K - 1) == 12.0 / 21.0
    assert abs(d["lag"] - ref.lag(p.cpu().numpy(), replayed.e.cpu().numpy())) <= 1e-12 * d["lag"]


def test_an_average_equal_to_the_parameters_does_not_move():
    for n in SIZES:
        p = _randn(n, 5)
        avg = _average(p, 0.9)                                        # e = a clone of p
        before = avg.e.clone()
        avg.update()
        part = avg.partials.cpu().numpy().reshape(-1, 2)
        assert torch.equal(_bits(avg.e), _bits(before)) and np.all(part[:, 0] == 0.0), n
        want = ref.sums(p.cpu().numpy(), p.cpu().numpy())[1]
        assert abs(part[:, 1].sum() - want) <= n * 2.0 ** -52 * want, n
        assert avg.read_lag()["lag"] == 0.0


def test_twenty_launches_give_the_same_bits():
    n = 3 * CHUNK + 8
    p, e0 = _randn(n, 6), _randn(n, 7)
    first = None
    for _ in range(20):
        avg = _average(p, 0.9, e0=e0)
        avg.updates.fill_(3)
        avg.update()
        got = (_bits(avg.e).clone(), _bits(avg.partials).clone())
        first = first or got
        assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])


def test_nothing_outside_the_ranges_is_written():
    """Sentinels before and after e[0:n) and after partials[0:2 blocks) stay; param is bit-unchanged."""
    from dvg_amd import ops
    pad = 64
    for n in SIZES:
        nb = ref.blocks(n)
        ebuf = torch.full((n + 2 * pad,), 12345.0, device=DEV)
        pbuf = torch.full((2 * nb + pad,), -7.0, dtype=torch.float64, device=DEV)
        e = ebuf[pad:pad + n]
        e.copy_(_randn(n, 8))
        p = _randn(n, 9)
        p0 = p.clone()
        updates = torch.tensor([5], dtype=torch.int32, device=DEV)
        assert ops.ema_update(e, p, 0.9, updates, pbuf) == nb
        assert bool((ebuf[:pad] == 12345.0).all()) and bool((ebuf[pad + n:] == 12345.0).all()), n
        assert bool((pbuf[2 * nb:] == -7.0).all()) and bool((pbuf[:2 * nb] >= 0).all()), n
        assert torch.equal(_bits(p), _bits(p0)) and int(updates) == 5      # the kernel reads the count, the caller advances it


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_nonfinite_parameter_reaches_its_own_element_only(bad):
    n = 3 * CHUNK + 8
    p, e0 = _randn(n, 11), _randn(n, 12)
    clean = _average(p, 0.9, e0=e0)
    clean.update()
    for pos in (CHUNK - 1, CHUNK):                       # just before and just after a chunk edge
        q = p.clone()
        q[pos] = bad
        avg = _average(q, 0.9, e0=e0)
        avg.update()
        got = avg.e.clone()
        assert not bool(torch.isfinite(got[pos])) and (bool(torch.isnan(got[pos])) == (bad != bad)), (bad, pos)
        got[pos] = clean.e[pos]
        assert torch.equal(_bits(got), _bits(clean.e)), (bad, pos)
        part, ok = avg.partials.view(-1, 2), clean.partials.view(-1, 2)
        hit = pos // CHUNK
        assert not bool(torch.isfinite(part[hit, 0])), (bad, pos)
        rest = [b for b in range(part.shape[0]) if b != hit]
        assert torch.equal(_bits(part[rest].contiguous()), _bits(ok[rest].contiguous())), (bad, pos)


def test_wrapper_checks():
    from dvg_amd import ops
    e, p = torch.zeros(8, device=DEV), torch.ones(8, device=DEV)
    u, part = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ema_update(e.cpu(), p, 0.9, u, part)
    with pytest.raises(RuntimeError, match="float32"):
        ops.ema_update(e.double(), p, 0.9, u, part)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.ema_update(torch.zeros(16, device=DEV)[::2], p, 0.9, u, part)
    with pytest.raises(RuntimeError, match="one size"):
        ops.ema_update(e, torch.ones(12, device=DEV), 0.9, u, part)
    with pytest.raises(RuntimeError, match="int32"):
        ops.ema_update(e, p, 0.9, u.long(), part)
    with pytest.raises(RuntimeError, match="do not fit"):
        ops.ema_update(e, p, 0.9, u, part[:1])
    with pytest.raises(RuntimeError, match="same buffer"):
        ops.ema_update(e, e, 0.9, u, part)
    with pytest.raises(RuntimeError, match="decay"):
        ops.ema_update(e, p, 1.0, u, part)
    assert float(e.abs().max()) == 0.0 and int(u) == 0


# ---- the Trainer ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batches():
    return train_harness.make_batches(4)


def _iterate(tr, xs, graphed, warmup=1, resume_after=None, flags=()):
    """The iterations over xs, eager or as GraphedIteration; clones of arena.p after each; resume_after = k: after k iterations
    the state goes through a file image into a fresh Trainer with another seed, which does the rest."""
    import train
    step = train.GraphedIteration(tr, warmup=warmup) if graphed else tr.iteration
    torch.manual_seed(77)                    # the GP samples of the iterations
    ps = []
    for i, x in enumerate(xs):
        if resume_after is not None and i == resume_after:
            f = io.BytesIO()
            torch.save(tr.state_dict(epoch=0), f)
            f.seek(0)
            del tr, step
            tr = train_harness.trainer(flags, seed=99)
            tr.load_state_dict(torch.load(f, weights_only=False))
            step = train.GraphedIteration(tr, warmup=max(warmup - resume_after, 0)) if graphed else tr.iteration
        step(x)
        ps.append(tr.arena.p.clone())
    torch.cuda.synchronize()
    if graphed:
        assert not step.failed and step.graph is not None            # the step did not fall back to eager iterations
    return tr, ps


def _walk(o):
    if torch.is_tensor(o):
        yield o
    elif isinstance(o, dict):
        for v in o.values():
            yield from _walk(v)
    elif isinstance(o, (list, tuple)):
        for v in o:
            yield from _walk(v)
    elif isinstance(o, torch.nn.Module):
        yield from o.parameters()
        yield from o.buffers()


def test_without_the_flag_nothing_exists(batches, tmp_path):
    tr = train_harness.trainer()
    assert tr.ema is None
    tr.iteration(batches[0])
    sd = tr.state_dict()
    assert "e" not in sd["arena"] and "ema" not in sd and sorted(sd["arena"]) == ["g_gp", "g_gp_range", "m", "p", "v"]
    tr.save(str(tmp_path / "model.pth"))
    assert os.listdir(str(tmp_path)) == ["model.pth"]


@pytest.fixture(scope="module")
def runs(batches):
    """Four iterations without the flag and with --ema_decay 0.9, eager and as GraphedIteration (capture at the second)."""
    out = {}
    for graphed in (False, True):
        plain, _ = _iterate(train_harness.trainer(), batches, graphed)
        kept = {n: getattr(plain.arena, n).clone() for n in ("p", "m", "v")}
        del plain
        avg = train_harness.trainer(["--ema_decay", "0.9"])
        p0 = avg.arena.p.clone()
        assert torch.equal(avg.ema.e, p0) and avg.ema.e.data_ptr() != avg.arena.p.data_ptr() and int(avg.ema.updates) == 0
        avg, ps = _iterate(avg, batches, graphed)
        out[graphed] = {"plain": kept, "tr": avg, "ps": ps, "p0": p0}
    return out


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])
def test_the_average_only_reads(runs, graphed):
    r = runs[graphed]
    for n in ("p", "m", "v"):
        assert torch.equal(getattr(r["tr"].arena, n), r["plain"][n]), n          # bit-equal to the run without the flag
    assert r["tr"].ema is not None and int(r["tr"].ema.updates) == 4
    assert torch.equal(r["tr"].arena.p, r["ps"][-1])


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])
def test_trainer_average_against_fp64(runs, graphed):
    """e against ema_ref fed the arena.p clones taken after each iteration, from the initial parameters (the same seed)."""
    r = runs[graphed]
    want, top = r["p0"].cpu().numpy(), 0.0
    for k, p in enumerate(r["ps"]):
        pk = p.cpu().numpy()
        want = ref.update(want, pk, 0.9, k).astype(np.float32)
        top = max(top, float(np.abs(pk).max()), float(np.abs(want).max()))
    err = float(np.abs(r["tr"].ema.e.cpu().numpy().astype(np.float64) - want).max())
    bar = 4 * 2.0 ** -23 * top
    print(f"\nTrainer average ({'graph' if graphed else 'eager'}): |e - fp64| {err:.3e} / bar {bar:.3e}")
    assert err <= bar
    assert not torch.equal(r["tr"].ema.e, r["tr"].arena.p)


def test_graphed_average_is_the_eager_average(runs):
    """The captured update gives the bits of the eager kernel: the four updates launched eagerly over the parameter clones of
    the GRAPHED run reproduce its average bit for bit.  Graphed and eager iterations themselves agree in the parameters only
    within test_graphed_iteration_matches_eager's tolerances (other kernel paths); where their parameters ARE bit-equal, so
    are the two averages."""
    r = runs[True]
    p = r["p0"].clone()
    again = _average(p, 0.9)
    for pk in r["ps"]:
        p.copy_(pk)
        again.update()
    assert torch.equal(_bits(again.e), _bits(r["tr"].ema.e)) and int(again.updates) == int(r["tr"].ema.updates) == 4
    assert torch.equal(_bits(again.partials), _bits(r["tr"].ema.partials))
    same = all(torch.equal(a, b) for a, b in zip(runs[False]["ps"], r["ps"]))
    print(f"\ngraphed and eager parameters bit-equal over the four iterations: {same}")
    if same:
        assert torch.equal(_bits(runs[False]["tr"].ema.e), _bits(r["tr"].ema.e))


def test_read_lag(runs):
    from dvg_amd import graphs
    for graphed in (False, True):
        tr = runs[graphed]["tr"]
        d = tr.ema.read_lag()
        want = ref.lag(tr.arena.p.cpu().numpy(), tr.ema.e.cpu().numpy())
        assert d["updates"] == 4 and d["decay_eff"] == ref.decay_at(0.9, 3) == 4.0 / 13.0
        assert want > 0 and abs(d["lag"] - want) <= 1e-12 * want, (d, want)
        line = tr.ema.epoch_line()
        assert line.startswith("     ema: decay 0.9 (effective 0.307692)  updates 4  lag |p-ema|/|p| "), line
    avg = runs[False]["tr"].ema
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="capture"):
        with graphs.capturing():
            avg.read_lag()


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])
def test_resume_continues_the_average(runs, batches, graphed):
    """Four iterations in one go (the module's run) against 2 + (save to a file image, fresh Trainer, load) + 2; the graph forms
    capture at the fourth iteration.  The rule of test_gpu_resume.test_continuation: A-versus-A is measured first, bit-identical
    runs demand a bit-identical continuation - parameters, average and count."""
    flags = ["--ema_decay", "0.9"]
    a1, _ = _iterate(train_harness.trainer(flags), batches, graphed, warmup=3)
    a2, _ = _iterate(train_harness.trainer(flags), batches, graphed, warmup=3)
    noise = float((a2.arena.p - a1.arena.p).abs().max())
    b, _ = _iterate(train_harness.trainer(flags), batches, graphed, warmup=3, resume_after=2, flags=flags)
    print(f"\nresume with an average ({'graph' if graphed else 'eager'}): A vs A {noise:.3e}")
    assert int(b.ema.updates) == int(a1.ema.updates) == 4
    if noise == 0.0:
        assert torch.equal(b.arena.p, a1.arena.p) and torch.equal(_bits(b.ema.e), _bits(a1.ema.e))
    else:
        assert float((b.ema.e - a1.ema.e).abs().max()) <= 2 * noise


def test_states_with_and_without_an_average(batches, capsys):
    flags = ["--ema_decay", "0.9"]
    with_avg, _ = _iterate(train_harness.trainer(flags), batches[:2], False)
    sd = with_avg.state_dict(epoch=1)
    assert sd["ema"] == {"decay": 0.9, "updates": 2} and torch.equal(sd["arena"]["e"], with_avg.ema.e)
    assert sd["format"] == 1 and "ema_decay" not in sd["fingerprint"]
    tensors = list(_walk(sd))
    assert len(tensors) > 20
    for t in tensors:                                                  # every tensor of the state owns its storage
        assert t.untyped_storage().nbytes() == t.numel() * t.element_size()
    plain, _ = _iterate(train_harness.trainer(), batches[:1], False)
    # a state without an average into a run with the flag: the average restarts from the restored parameters
    fresh = train_harness.trainer(flags, seed=99)
    fresh.ema.updates.fill_(7)
    capsys.readouterr()
    fresh.load_state_dict(plain.state_dict(epoch=1))
    out = capsys.readouterr().out
    assert torch.equal(fresh.arena.p, plain.arena.p) and torch.equal(fresh.ema.e, plain.arena.p) and int(fresh.ema.updates) == 0
    assert out.count("\n") == 1 and "restarts" in out
    # a state with an average into a run without the flag: loads, says so, builds nothing
    bare = train_harness.trainer(seed=98)
    bare.load_state_dict(sd)
    out = capsys.readouterr().out
    assert bare.ema is None and torch.equal(bare.arena.p, with_avg.arena.p) and out.count("\n") == 1 and "ignored" in out
    # with the flag: through the existing buffers, this run's decay
    other = train_harness.trainer(["--ema_decay", "0.5"], seed=97)
    e_ptr = other.ema.e.data_ptr()
    other.load_state_dict(sd)
    assert capsys.readouterr().out == ""
    assert other.ema.e.data_ptr() == e_ptr and torch.equal(other.ema.e, with_avg.ema.e) and int(other.ema.updates) == 2
    assert other.ema.decay == 0.5


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_command_line_writes_and_reads_the_averaged_checkpoint(tmp_path, capsys):
    import generate_frames
    import train
    out = str(tmp_path / "run")
    tr = train.main(train_harness.ARGS + ["--ema_decay", "0.5", "--niter", "1", "--epoch_size", "2", "--no_images", "--output_path", out])
    text = capsys.readouterr().out
    lines = text.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("     train frames/s:")]
    assert len(at) == 1 and lines[at[0] + 1].startswith("     ema: decay 0.5 (effective 0.181818)  updates 2  lag "), text
    ck = torch.load(os.path.join(out, "model.pth"), weights_only=False)
    ek = torch.load(os.path.join(out, "model_ema.pth"), weights_only=False)
    assert set(ek) == set(ck) == KEYS
    e, base = tr.ema.e, tr.arena.p.data_ptr()

    def averaged(live):
        off = (live.data_ptr() - base) // 4
        return e[off:off + live.numel()].view(live.shape).cpu()
    checked = 0
    for name, live_mod in (("encoder", tr.encoder), ("decoder", tr.decoder), ("frame_predictor", tr.frame_predictor)):
        mine, theirs = dict(ek[name].named_parameters()), dict(ck[name].named_parameters())
        for k, live in live_mod.named_parameters():
            assert torch.equal(mine[k].detach().cpu(), averaged(live)), (name, k)
            checked += 1
        assert any(not torch.equal(mine[k], theirs[k]) for k in mine), name     # (a bias in front of a BatchNorm never moves)
        mb, tb = dict(ek[name].named_buffers()), dict(ck[name].named_buffers())
        assert set(mb) == set(tb) and all(torch.equal(mb[k], tb[k]) for k in mb), name
    for name, live_mod in (("gp_layer", tr.gp_layer), ("likelihood", tr.likelihood)):
        params = dict(live_mod.named_parameters())
        assert list(ek[name]) == list(ck[name]) and params
        for k in ek[name]:
            if k in params:
                assert torch.equal(ek[name][k].cpu(), averaged(params[k])), (name, k)
                checked += 1
            else:
                assert torch.equal(ek[name][k], ck[name][k]), (name, k)         # buffers: the live ones
        assert any(not torch.equal(ek[name][k], ck[name][k]) for k in params), name
    assert checked == sum(1 for m in tr.modules for _ in m.parameters())
    assert str(ek["gp_layer_optimizer"]["state"].keys()) == str(ck["gp_layer_optimizer"]["state"].keys())
    for t in _walk(ek):                                              # no tensor carries the arena's storage
        assert t.untyped_storage().nbytes() == t.numel() * t.element_size()
    sd = torch.load(os.path.join(out, "train_state.pth"), weights_only=False)
    assert sd["ema"] == {"decay": 0.5, "updates": 2} and torch.equal(sd["arena"]["e"].to(DEV), e)
    gen_args = ["--model_dir", out, "--dataset", "smmnist", "--synthetic_data", "--batch_size", "4", "--n_eval", "6", "--n_future",
                "4", "--nsample", "2", "--nbatches", "1", "--no_images", "--log_dir", out + "/logs"]
    gen = generate_frames.main(gen_args + ["--ema"])
    res = torch.load(os.path.join(out, "logs", "gen", "sample_lstm_0.pt"))
    assert bool(torch.isfinite(res["psnr"]).all())
    w_live = next(tr.encoder.parameters())
    w_gen = next(gen.encoder.parameters())
    assert torch.equal(w_gen.detach().cpu(), averaged(w_live)) and not torch.equal(w_gen.detach().cpu(), w_live.detach().cpu())
    os.remove(os.path.join(out, "model_ema.pth"))
    with pytest.raises(SystemExit) as exc:
        generate_frames.main(gen_args + ["--ema"])
    msg = str(exc.value)
    assert "smmnist_ema.pth" in msg and "model_ema.pth" in msg and "\n" not in msg


def test_two_ranks_average_alike_and_resume(tmp_path):
    """Two ranks on one GPU over gloo (the rehearsal switches and fresh child processes of test_two_ranks_clip_alike): every rank
    computes the same average from the same parameters without a collective - as a chain of hipGraphs (SegmentedIteration,
    captured at the third iteration) and eagerly; rank 0's train_state.pth holds it; three epochs in one go and two + a resume
    + one end with the same bits in the parameters and in the average.  The resume legs run with --no_hip_graph: a fresh process
    starts with eager warm-up iterations where the uninterrupted run replays, and those agree to a tolerance only
    (test_graphed_iteration_matches_eager) - the single-process test above lines the capture points up instead."""
    args = ["--model", "dcgan", "--dataset", "smmnist", "--n_past", "2", "--n_future", "2", "--n_eval", "4", "--batch_size", "8",
            "--save_every", "1", "--no_images", "--print_param_checksum", "--ema_decay", "0.9"]

    def run(extra):
        r = train_harness.run_train_py(args + extra, ranks=2, env=train_harness.REHEARSAL)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "capture failed" not in r.stderr
        sums = {ln.split()[1]: ln.split()[4:] for ln in r.stdout.splitlines() if " ema checksum " in ln}
        pars = {ln.split()[1]: ln.split()[-2:] for ln in r.stdout.splitlines() if " param checksum " in ln}
        assert set(sums) == {"0", "1"} and sums["0"] == sums["1"], sums          # both ranks: the same average
        assert pars["0"] == pars["1"]
        return r, sums["0"], pars["0"]

    r, graphed, _ = run(["--niter", "1", "--epoch_size", "4", "--no_save"])
    assert graphed[-1] == "4" and r.stdout.count("     ema: decay 0.9 ") == 1    # rank 0 alone prints, once per epoch
    split, whole = str(tmp_path / "split"), str(tmp_path / "whole")
    eager = ["--no_hip_graph", "--epoch_size", "2"]
    r, two, _ = run(eager + ["--niter", "2", "--output_path", split])
    assert two[-1] == "4" and r.stdout.count("     ema: decay 0.9 ") == 2
    sd = torch.load(os.path.join(split, "train_state.pth"), weights_only=False)
    e = sd["arena"]["e"].to(DEV).double()
    assert sd["ema"] == {"decay": 0.9, "updates": 4}
    assert ['%.17g' % float(e.sum()), '%.17g' % float(e.abs().sum())] == two[:2]  # rank 0's file holds that average
    assert os.path.exists(os.path.join(split, "model_ema.pth"))
    r, resumed, p_resumed = run(eager + ["--niter", "3", "--output_path", split, "--resume", split])
    assert "resumed from" in r.stdout and "restarts" not in r.stdout and resumed[-1] == "6" and resumed != two
    _, straight, p_straight = run(eager + ["--niter", "3", "--output_path", whole])
    assert (resumed, p_resumed) == (straight, p_straight)
