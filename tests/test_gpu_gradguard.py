"""GPU: the gradient guard - dvg_grad_sumsq / dvg_grad_guard_finish / dvg_adam_step_guarded (grad_guard.hip), optim.GradGuard and
guarded_step, and train.py --clip_grad_norm / --skip_nonfinite through the Trainer, a hipGraph, a resume and the command line.

Bars.  The norm: an fp64 sum of n exact squares errs by at most n 2^-53 relative (n <= 2^20 + 12 here: 1.2e-10), the square root
by 2^-53, the one rounding to fp32 by 2^-24 = 6e-8; one more fp32 ulp is allowed for the reference's own conversion: 1.2e-7
relative on stat[0], and the same on the clip factor against torch.nn.utils.clip_grad_norm_ run on an fp64 copy.  Adam against
torch: test_fused_adam_matches_torch_adam's own rtol = 2e-6, atol = 2e-7 (measured here: printed by the test).  Everything that
compares a guarded run with another run of the same kernels on the same inputs is bit-for-bit.

Shapes: n around the 16 384-float chunk of the reduction (one block, the last float of a block, the first of the next, several
blocks and a ragged last one), dcgan_64 at batch 4, n_past 2, n_future 2 for the Trainer (the shapes of
test_graphed_iteration_matches_eager and test_gpu_resume)."""
import io

import numpy as np
import pytest
import torch

from tests import gradguard_ref as ref, train_harness

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = ref.CHUNK
BAR = 1.2e-7
SIZES = [4, 1024, CHUNK - 4, CHUNK, CHUNK + 4, 3 * CHUNK + 8, 2 ** 20 + 12]


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
def _verdict(g, max_norm, skip):
    """One step site over the flat tensor g with a fresh guard: (partials, stat, counters) as host lists."""
    from dvg_amd import ops
    from dvg_amd.optim import GradGuard
    guard = GradGuard(max_norm, skip, g.device)
    nb = ops.grad_sumsq_blocks(g.numel())
    part = guard.reserve(nb)
    assert ops.grad_sumsq(g, part) == nb == ref.blocks(g.numel())
    ops.grad_guard_finish(part, nb, guard.max_norm, guard.skip_nonfinite, guard.stat, guard.counters)
    return part[:nb].clone(), guard.stat.clone(), guard.counters.tolist()


def _data(kind, n, seed=0):
    gen = torch.Generator(device=DEV).manual_seed(1000 + seed)
    g = torch.randn(n, device=DEV, generator=gen)
    return {"randn": g, "huge": g * 1e25, "tiny": g * 1e-25, "zeros": torch.zeros(n, device=DEV)}[kind]


def _torch_coef(g, max_norm, probe):
    """The factor torch.nn.utils.clip_grad_norm_ applies to an fp64 copy of g, read off a finite non-zero element."""
    p = torch.nn.Parameter(torch.zeros(g.numel(), dtype=torch.float64, device=g.device))
    p.grad = g.double().clone()
    torch.nn.utils.clip_grad_norm_([p], max_norm)
    return float(p.grad[probe] / g[probe].double())


@pytest.mark.parametrize("kind", ["randn", "huge", "tiny", "zeros"])
def test_norm_against_numpy_fp64(kind):
    worst = 0.0
    for n in SIZES:
        g = _data(kind, n)
        part, stat, counters = _verdict(g, 1.0, True)
        x = g.cpu().numpy().astype(np.float64)
        want = float(np.sqrt(np.sum(x * x)))
        got = float(stat[0])
        assert stat[2] == 0 and counters[0] == 1 and counters[2] == 0, (kind, n)      # 1e25: squares overflow fp32, not the sum
        if kind == "zeros":
            assert got == 0.0 and float(stat[1]) == 1.0 and counters[1] == 0 and float(stat[3]) == 0.0
            continue
        assert np.isfinite(got) and float(stat[3]) == got
        worst = max(worst, abs(got - want) / want)
        # the partial sums themselves: fp64 sums of exact squares of each chunk
        pw = np.array([np.sum(x[i:i + CHUNK] ** 2) for i in range(0, n, CHUNK)])
        assert np.allclose(part.cpu().numpy(), pw, rtol=CHUNK * 2.0 ** -53, atol=0)
    print(f"\ngrad norm {kind}: worst relative error {worst:.3e} / bar {BAR:.1e}")
    assert worst <= BAR


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_nonfinite_detection_on_both_sides_of_a_chunk_edge(bad):
    n = 3 * CHUNK + 8
    for pos in (0, n - 1, CHUNK - 1, CHUNK):
        g = _data("randn", n, seed=1)
        g[pos] = bad
        _, stat, counters = _verdict(g, 1.0, True)
        assert float(stat[2]) == 1.0 and counters == [1, 0, 1] and float(stat[3]) == 0.0, (bad, pos)
        _, stat0, counters0 = _verdict(g, 1.0, False)
        assert float(stat0[2]) == 0.0 and counters0[2] == 0, (bad, pos)
        want = _torch_coef(g, 1.0, probe=7)
        for s in (stat, stat0):                     # 0 for an infinite norm, NaN for a NaN one - as torch on the same tensor
            got = float(s[1])
            assert (np.isnan(want) and np.isnan(got)) or got == want == 0.0, (bad, pos, got, want)
        assert np.isnan(want) == (bad != bad)


def test_twenty_launches_give_the_same_bits():
    g = _data("randn", 3 * CHUNK + 8, seed=2)
    p0, s0, _ = _verdict(g, 0.5, True)
    for _ in range(19):
        p, s, _ = _verdict(g, 0.5, True)
        assert torch.equal(p.view(torch.int64), p0.view(torch.int64)) and torch.equal(s.view(torch.int32), s0.view(torch.int32))


def test_clip_factor_against_torch():
    g = _data("randn", 3 * CHUNK + 8, seed=3)
    nrm = float(g.double().norm())
    for c, clips in ((0.25 * nrm, True), (4.0 * nrm, False)):
        _, stat, counters = _verdict(g, c, False)
        want, got = _torch_coef(g, c, probe=7), float(stat[1])
        print(f"\nclip factor, C = {c:.4g}, norm {nrm:.6g}: {got!r} against torch {want!r} (bar {BAR:.1e} relative)")
        assert abs(got - want) <= BAR * want and counters == [1, int(clips), 0]
        assert (got < 1.0) if clips else (got == 1.0 and want == 1.0)
    _, stat, counters = _verdict(g, 0.0, False)     # no clipping asked for
    assert float(stat[1]) == 1.0 and counters == [1, 0, 0]


def test_guarded_adam_with_factor_one_is_bit_identical_to_the_plain_step():
    """dvg_adam_step_guarded with stat[1] == 1 against dvg_adam_step on copies of the same buffers, with and without weight decay,
    host and device step counts, a ragged tail; and with stat[2] == 1 nothing but the skip counter moves."""
    from dvg_amd import ops
    from dvg_amd._lib import check, lib
    torch.manual_seed(4)
    for n, wd in ((4 * 4096 * 256 + 8, 0.0), (1031, 0.01)):
        p, g, m, v = (torch.randn(n, device=DEV) for _ in range(4))
        v = v.abs()
        stat = torch.tensor([1.0, 1.0, 0.0, 0.0], device=DEV)
        skips = torch.tensor([2], dtype=torch.int32, device=DEV)
        tdev = torch.tensor([7], dtype=torch.int32, device=DEV)
        t5 = torch.tensor([5], dtype=torch.int32, device=DEV)
        for step_dev in (None, tdev):
            a, b = [t.clone() for t in (p, m, v)], [t.clone() for t in (p, m, v)]
            check(lib().dvg_adam_step(ops._p(a[0]), ops._p(g), ops._p(a[1]), ops._p(a[2]), n, 2e-3, 0.9, 0.999, 1e-8, wd, 5,
                                      ops._p(None if step_dev is None else t5), ops._stream()), "dvg_adam_step")
            ops.adam_step_guarded(b[0], g, b[1], b[2], 2e-3, 0.9, 0.999, 1e-8, wd, 7, step_dev, stat, skips)   # 7 - 2 skipped = 5
            for x, y in zip(a, b):
                assert torch.equal(x, y), (n, wd, step_dev is not None)
            assert int(skips) == 2
        stat[2] = 1.0
        b = [t.clone() for t in (p, m, v)]
        ops.adam_step_guarded(b[0], g, b[1], b[2], 2e-3, 0.9, 0.999, 1e-8, wd, 7, None, stat, skips)
        assert int(skips) == 3 and all(torch.equal(x, y) for x, y in zip(b, (p, m, v)))


# ---- FusedAdam + GradGuard -----------------------------------------------------------------------------------------------------
SHAPES = [(64, 3, 3, 3), (64,), (17, 5), (1,), (90, 40, 40)]


def _two_optimizers(seed=0):
    """test_fused_adam_matches_torch_adam's two groups (the second with weight decay), split over two FusedAdam that share one
    arena; plus the torch.optim.Adam twin on copies."""
    from dvg_amd.optim import FlatArena, FusedAdam
    torch.manual_seed(seed)
    ref_p = [torch.nn.Parameter(torch.randn(*s, device=DEV)) for s in SHAPES]
    mine = [torch.nn.Parameter(p.detach().clone()) for p in ref_p]
    arena = FlatArena(FlatArena.size_for(mine), DEV)
    o1 = FusedAdam([{"params": mine[:3]}], lr=2e-3, arena=arena)
    o2 = FusedAdam([{"params": mine[3:], "weight_decay": 0.01}], lr=2e-3, arena=arena)
    o_ref = torch.optim.Adam([{"params": ref_p[:3]}, {"params": ref_p[3:], "weight_decay": 0.01}], lr=2e-3)
    return ref_p, mine, arena, (o1, o2), o_ref


def _grads(step, scale=1.0):
    gen = torch.Generator(device=DEV).manual_seed(50 + step)
    return [torch.randn(*s, device=DEV, generator=gen) * scale for s in SHAPES]


def _counts(opts):
    return [int(o.state[p]["step"]) for o in opts for g in o.param_groups for p in g["params"]]


def test_guarded_step_matches_clip_grad_norm_and_torch_adam():
    """5 steps of clip_grad_norm_(all parameters, C) + torch.optim.Adam.step() against guarded_step over two FusedAdam in one
    arena, MultiStepLR on both sides.  The gradient norms are about 382 (even steps) and 3.8 (odd steps); C = 50 clips the
    former only.  Bars rtol = 2e-6, atol = 2e-7 as test_fused_adam_matches_torch_adam."""
    from dvg_amd.optim import GradGuard, guarded_step
    ref_p, mine, arena, opts, o_ref = _two_optimizers()
    sched = [torch.optim.lr_scheduler.MultiStepLR(o, milestones=[2], gamma=0.1) for o in (o_ref,) + opts]
    guard = GradGuard(50.0, False, DEV)
    worst = 0.0
    for it in range(5):
        for p, q, g in zip(ref_p, mine, _grads(it, 1.0 if it % 2 == 0 else 0.01)):
            p.grad = g.clone()
            q.grad.copy_(g)
        torch.nn.utils.clip_grad_norm_(ref_p, 50.0)
        o_ref.step()
        guarded_step(opts, guard)
        for s in sched:
            s.step()
        for p, q in zip(ref_p, mine):
            worst = max(worst, float(((p - q).abs() / (2e-7 + 2e-6 * p.abs())).max()))
            assert torch.allclose(p, q, rtol=2e-6, atol=2e-7), it
    d = guard.read_and_reset()
    print(f"\nguarded_step against torch: worst |difference| / (atol + rtol |p|) = {worst:.3f}; {d}")
    assert d["sites"] == 5 and d["clipped"] == 3 and d["skipped"] == 0 and 300 < d["max"] < 500 and 2 < d["last"] < 500
    assert guard.read_and_reset() == {"max": 0.0, "last": d["last"], "sites": 0, "clipped": 0, "skipped": 0}
    assert _counts(opts) == [5] * 5
    # a partially used group cannot be guarded, and says so before anything is launched
    mine[1].grad = None
    before = arena.p.clone()
    with pytest.raises(RuntimeError, match="partially used"):
        guarded_step(opts, guard)
    assert torch.equal(arena.p, before) and guard.read_and_reset()["sites"] == 0


def _run_steps(steps, poison=None, graph=False):
    """guarded_step (skip_nonfinite, C = 50) over the gradients of `steps`; poison = k: a NaN in one gradient element of step k.
    graph: the sequence [zero_grads tick, copy of the gradients from a staging buffer, guarded_step] captured once, replayed
    per step.  Returns the arena, the optimisers, the guard and the (p, m, v) clones taken before and after the poisoned step."""
    from dvg_amd import graphs
    from dvg_amd.optim import GradGuard, guarded_step, zero_grads
    if graph:
        _run_steps([0])                      # every kernel of the sequence has been launched once before the capture
    _, mine, arena, opts, _ = _two_optimizers()
    guard = GradGuard(50.0, True, DEV)
    staging = torch.zeros_like(arena.g)
    around = {}

    def fill(k):
        off = 0
        for g in _grads(k):
            staging[off:off + g.numel()].copy_(g.reshape(-1))
            off += (g.numel() + 3) // 4 * 4
        if k == poison:
            staging[SHAPES[0][0] * 27 + 5] = float("nan")       # in the second parameter of the first optimiser

    def body():
        zero_grads(opts)
        arena.g.copy_(staging)
        guarded_step(opts, guard)
    graph_obj = None
    if graph:
        guard.attach(opts)
        for o in opts:
            o.begin_capture()
        torch.cuda.synchronize()
        with graphs.capturing() as graph_obj:
            body()
        for o in opts:
            o.end_capture()
    for k in steps:
        fill(k)
        if k == poison:
            around["before"] = [t.clone() for t in (arena.p, arena.m, arena.v)]
        if graph:
            for o in opts:
                o.check_graph_fresh()
            graph_obj.replay()
            for o in opts:
                o.after_graph_replay()
        else:
            body()
        if k == poison:
            around["after"] = [t.clone() for t in (arena.p, arena.m, arena.v)]
    torch.cuda.synchronize()
    return arena, opts, guard, around, graph_obj


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_a_skipped_step_changes_no_state(graph):
    """4 steps, a NaN in one gradient element of the second: p, m, v of every group are bit-equal across it, the counts of
    applied steps are 3, and the end state is bit-equal to a run of the three clean steps alone (eager, host step counts) -
    also when the four steps are replays of one captured graph (device step counts minus the device skip counters)."""
    arena, opts, guard, around, graph_obj = _run_steps([0, 1, 2, 3], poison=1, graph=graph)
    for a, b in zip(around["before"], around["after"]):
        assert torch.equal(a, b)
    assert not torch.equal(arena.p, around["after"][0])                      # the later steps were applied
    assert _counts(opts) == [4] * 5                                          # counted on the host, skipped on the device
    for o in opts:
        o.sync_step_counts()
    assert _counts(opts) == [3] * 5
    assert all(int(f["skips"]) == 0 for o in opts for f in o._flat.values())
    d = guard.read_and_reset()
    assert (d["sites"], d["clipped"], d["skipped"]) == (4, 3, 1) and 300 < d["max"] < 500
    clean, clean_opts, _, _, _ = _run_steps([0, 2, 3])
    for name in ("p", "m", "v"):
        assert torch.equal(getattr(arena, name), getattr(clean, name)), name
    assert all(bool(torch.isfinite(getattr(arena, n)).all()) for n in ("p", "m", "v"))
    assert _counts(clean_opts) == [3] * 5
    sd = opts[0].state_dict()
    assert float(sd["state"][0]["step"]) == 3.0 and opts[1].host_state()["steps"] == [[3, 3]]
    if graph:
        assert all(int(f["tdev"]) == 3 for o in opts for f in o._flat.values())     # sync took the skip off the device count too
        for o in opts:
            for f in o._flat.values():
                f["tdev"].fill_(99)
            o.begin_capture()
        assert all(int(f["tdev"]) == 3 for o in opts for f in o._flat.values())     # seeded with the steps really applied


def test_load_state_dict_forgets_pending_skips():
    """A torch-layout state loaded after a skipped step: its step counts are counts of applied steps, so the skip counters
    start again from zero (else the next sync would take the old skip off the loaded counts)."""
    _, opts, _, _, _ = _run_steps([0, 1], poison=1)
    saved = [o.state_dict() for o in opts]                     # folds the skip: 1 step applied
    assert _counts(opts) == [1] * 5
    _, opts2, _, _, _ = _run_steps([0, 1, 2], poison=2)          # a skip is pending in opts2
    assert any(int(f["skips"]) == 1 for o in opts2 for f in o._flat.values())
    for o, sd in zip(opts2, saved):
        o.load_state_dict(sd)
    assert all(int(f["skips"]) == 0 for o in opts2 for f in o._flat.values())
    for o in opts2:
        o.sync_step_counts()
    assert _counts(opts2) == [1] * 5


# ---- the Trainer ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batches():
    return train_harness.make_batches(4)


def test_trainer_builds_a_guard_only_when_asked(batches):
    assert train_harness.trainer().guard is None
    tr = train_harness.trainer(["--skip_nonfinite"])
    assert tr.guard is not None and tr.guard.max_norm == 0.0 and tr.guard.skip_nonfinite
    assert tr.guard.partials.numel() >= sum(ref.blocks(f["g"].numel()) for o in tr.optimizers() for f in o._flat.values())


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])
def test_a_guard_that_never_bites_changes_nothing(batches, graphed):
    """--clip_grad_norm 1e30: factor exactly 1 at every site - parameters and both moments bit-equal to the unguarded Trainer
    from the same seed and batches after 3 iterations, eager and as a hipGraph (capture at the second iteration)."""
    plain, guarded = train_harness.trainer(), train_harness.trainer(["--clip_grad_norm", "1e30"])
    train_harness.iterate(plain, batches[:3], graphed)
    train_harness.iterate(guarded, batches[:3], graphed)
    a, b = train_harness.arena(plain), train_harness.arena(guarded)
    for n in a:
        assert torch.equal(a[n], b[n]), n
    d = guarded.guard.read_and_reset()
    assert (d["sites"], d["clipped"], d["skipped"]) == (6, 0, 0) and 0 < d["last"] <= d["max"] < float("inf")


def test_trainer_norm_is_the_norm_of_the_whole_site(batches):
    """--no_ft: the only site is train_model's, over [GP | likelihood | LSTM | decoder | encoder].  stat[0] is the fp64 norm of
    that range of arena.g (the guard does not write g) to 1.2e-7; with C = half of it the site is clipped, and the graphed
    run agrees with the eager one within test_graphed_iteration_matches_eager's bars."""
    tr = train_harness.trainer(["--no_ft", "--clip_grad_norm", "1e30"])
    train_harness.iterate(tr, batches[:1], False)
    lo, hi = tr.rng_gp[0], tr.rng_enc[1]
    want, got = float(tr.arena.g[lo:hi].double().norm()), float(tr.guard.stat[0])
    print(f"\nTrainer site norm {got!r} against fp64 {want!r}: relative {abs(got - want) / want:.3e} / bar {BAR:.1e}")
    assert want > 0 and abs(got - want) <= BAR * want and float(tr.guard.stat[1]) == 1.0
    flags = ["--no_ft", "--clip_grad_norm", repr(want / 2)]
    eager = train_harness.trainer(flags)
    train_harness.iterate(eager, batches[:1], False)
    d = eager.guard.read_and_reset()
    assert (d["sites"], d["clipped"], d["skipped"]) == (1, 1, 0) and abs(d["last"] - want) <= 1e-3 * want
    assert abs(float(eager.guard.stat[1]) - 0.5) < 1e-2
    train_harness.iterate(eager, batches[1:3], False)
    graph = train_harness.trainer(flags)
    train_harness.iterate(graph, batches[:3], True)
    assert graph.guard.read_and_reset()["clipped"] >= 1
    assert torch.allclose(graph.arena.p, eager.arena.p, rtol=2e-3, atol=2e-5)


def _poisoned(tr, at):
    """Wrap tr._ar: right before the steps of train_model's site in iteration `at` (0-based) a NaN goes into one encoder
    gradient; the arena is cloned there and again when the next all-reduce point (the fine-tuning site's) is reached."""
    seen = {"site": 0}
    orig = tr._ar
    whole = (tr.rng_gp[0], tr.rng_enc[1])

    def ar(*actions):
        orig(*actions)
        last = actions[-1]
        if "before" in seen and "after" not in seen:
            seen["after"] = train_harness.arena(tr)
        if last == ("finish", "b") or (last[0] == "reduce" and tuple(last[1]) == whole):
            if seen["site"] == at:
                seen["before"] = train_harness.arena(tr)
                tr.arena.g[tr.rng_enc[0] + 5] = float("nan")
            seen["site"] += 1
    tr._ar = ar
    return seen


def _skip_run(xs, flags, resume_after=None, graphed=False, poison_at=1):
    """len(xs) iterations with the poison of _poisoned in iteration `poison_at` (None: none); resume_after = k: after k
    iterations the state goes through a file image into a fresh Trainer with another seed, which does the rest."""
    import train
    tr = train_harness.trainer(flags)
    seen = _poisoned(tr, poison_at) if poison_at is not None else {}
    step = train.GraphedIteration(tr, warmup=3) if graphed else tr.iteration
    torch.manual_seed(77)
    for i, x in enumerate(xs):
        if resume_after is not None and i == resume_after:
            f = io.BytesIO()
            torch.save(tr.state_dict(epoch=0), f)
            f.seek(0)
            del tr, step
            tr = train_harness.trainer(flags, seed=99)
            tr.load_state_dict(torch.load(f, weights_only=False))
            step = train.GraphedIteration(tr, warmup=3 - resume_after) if graphed else tr.iteration
        step(x)
    torch.cuda.synchronize()
    return tr, seen, step


def test_trainer_skips_a_poisoned_site_and_trains_on(batches):
    """--skip_nonfinite, eager: a NaN written into arena.g just before the steps of the second iteration's train_model site.
    Parameters and moments are bit-equal across that site, the encoder's count of applied steps is one behind the iteration
    count, the third iteration trains on finite values.  Without the flag the same poison leaves NaN parameters."""
    from dvg_amd import train_state
    tr, seen, _ = _skip_run(batches[:3], ["--skip_nonfinite"])
    for n in ("p", "m", "v"):
        assert torch.equal(seen["before"][n], seen["after"][n]), n
    d = tr.guard.read_and_reset()
    assert (d["sites"], d["clipped"], d["skipped"]) == (6, 0, 1)
    for o in tr.optimizers():
        o.sync_step_counts()
    assert train_state.global_step(tr) == 2 and int(tr.decoder_optimizer.host_state()["steps"][0][0]) == 2
    assert int(tr.frame_predictor_optimizer.host_state()["steps"][0][0]) == 5      # 3 fine-tuning steps + 2 of train_model
    assert not torch.equal(tr.arena.p, seen["after"]["p"])
    assert all(bool(torch.isfinite(getattr(tr.arena, n)).all()) for n in ("p", "m", "v"))
    bad, _, _ = _skip_run(batches[:2], [])
    assert bad.guard is None and bool(torch.isnan(bad.arena.p).any())              # the failure the flag prevents


def _same(a, b, noise):
    """Bit-equal where two identical runs are (noise == 0), else within twice their difference (test_gpu_resume's rule)."""
    if noise == 0.0:
        return all(torch.equal(getattr(a.arena, n), getattr(b.arena, n)) for n in ("p", "m", "v"))
    return float((a.arena.p - b.arena.p).abs().max()) / float(b.arena.p.abs().max()) <= 2 * noise


def _rel(a, b):
    return float((a.arena.p - b.arena.p).abs().max()) / float(b.arena.p.abs().max())


def test_resume_after_a_skipped_iteration_continues_like_the_uninterrupted_run(batches):
    """The run of test_trainer_skips_a_poisoned_site_and_trains_on saved after the skipped iteration (Trainer.state_dict folds
    the skip counters into the step counts), restored into a fresh Trainer and continued: as the uninterrupted run."""
    from dvg_amd import train_state
    flags = ["--skip_nonfinite", "--clip_grad_norm", "1e30"]
    a1, _, _ = _skip_run(batches[:3], flags)
    a2, _, _ = _skip_run(batches[:3], flags)
    noise = _rel(a2, a1)
    b, _, _ = _skip_run(batches[:3], flags, resume_after=2)
    print(f"\nresume after a skip: A vs A {noise:.3e}, resumed vs A {_rel(b, a1):.3e}")
    assert _same(b, a1, noise)
    assert train_state.global_step(b) == 2 and b.state_dict()["global_step"] == 2
    assert a1.state_dict()["global_step"] == 2


def test_graphed_continuation_with_a_clip_that_bites(batches):
    """4 iterations as GraphedIteration (capture at the 4th) with --clip_grad_norm 0.5, against 2 + (save, fresh Trainer, load)
    + 2: as the uninterrupted run (rule of test_gpu_resume.test_continuation), sites clipped on the way."""
    flags = ["--clip_grad_norm", "0.5"]
    a1, _, _ = _skip_run(batches, flags, graphed=True, poison_at=None)
    clipped = a1.guard.read_and_reset()["clipped"]
    a2, _, _ = _skip_run(batches, flags, graphed=True, poison_at=None)
    noise = _rel(a2, a1)
    b, _, step = _skip_run(batches, flags, resume_after=2, graphed=True, poison_at=None)
    print(f"\ngraphed continuation, clipping: A vs A {noise:.3e}, resumed vs A {_rel(b, a1):.3e}; clipped sites {clipped} of 8")
    assert clipped >= 1 and not step.failed and step.graph is not None and step.calls == 2
    assert _same(b, a1, noise)
    for o in b.optimizers():
        for f in o._flat.values():
            assert int(f["tdev"]) == int(o.state[f["params"][0]]["step"])


# ---- the command line ----------------------------------------------------------------------------------------------------------
def test_command_line_prints_the_epoch_line(capsys):
    import train
    tr = train.main(train_harness.ARGS + ["--clip_grad_norm", "0.5", "--skip_nonfinite", "--niter", "1", "--epoch_size", "2", "--no_save"])
    out = capsys.readouterr().out
    lines = out.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("     train frames/s:")]
    assert len(at) == 1 and lines[at[0] + 1].startswith("     grad norm: max "), out
    assert lines[at[0] + 1].endswith(" skipped 0  of 4 steps"), lines[at[0] + 1]      # two sites x two iterations
    assert tr.guard.counters.tolist() == [0, 0, 0]


def test_two_ranks_clip_alike():
    """Two ranks on one GPU over gloo (the rehearsal switches of tests/test_gpu_multirank.py): the norm is taken after the
    all-reduce, so both ranks compute the same factor without another collective and end with identical parameters."""
    args = ["--model", "dcgan", "--dataset", "smmnist", "--batch_size", "8", "--n_past", "2", "--n_future", "2", "--n_eval", "4",
            "--niter", "1", "--epoch_size", "4", "--no_save", "--save_every", "1000", "--print_param_checksum", "--clip_grad_norm", "0.5"]
    r = train_harness.run_train_py(args, ranks=2, env=train_harness.REHEARSAL)
    assert r.returncode == 0, r.stderr[-2000:]
    sums = {ln.split()[1]: ln.split()[-2:] for ln in r.stdout.splitlines() if "param checksum" in ln}
    assert set(sums) == {"0", "1"} and sums["0"] == sums["1"], sums
    line = [ln for ln in r.stdout.splitlines() if "grad norm:" in ln]
    assert len(line) == 1 and line[0].endswith("of 8 steps") and " clipped 0 " not in line[0], r.stdout[-1500:]
    assert "capture failed" not in r.stderr
