"""GPU: train.py --lr_schedule - dvg_lr_schedule_tick against the fp64 oracle (tests/lr_schedule_ref.py), dvg_adam_step_scheduled
against the two Adam kernels it stands for (scale 1: the same bits) and against torch.optim.Adam + LambdaLR, and the Trainer: a
zero rate moves no parameter, the flag alone changes nothing, one hipGraph capture serves a multiplier that moves every
iteration, a skipped step still counts as an iteration, and a resumed run continues bit for bit.

Shapes of the Trainer tests: tests/test_gpu_train.py's (dcgan_64 / vgg_64, batch 4, 2 + 2 frames, the in-repo synthetic smmnist)."""
import io

import numpy as np
import pytest
import torch

from tests import lr_schedule_ref as ref, train_harness

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, N, K, R, G = 3, 12, 4, 0.1, 0.5                  # the tick's case
INT_MAX = ref.INT_MAX


def _buffers(k=0):
    return torch.tensor([k], dtype=torch.int32, device=DEV), torch.full((1,), -1.0, device=DEV)


def _ticks(kind, n, r=R, g=G):
    """n launches from k = 0: the scale after each (one read at the end), and the count."""
    from dvg_amd import ops
    iters, scale = _buffers(0)
    seen = torch.zeros(n, device=DEV)
    for i in range(n):
        ops.lr_schedule_tick(kind, W, N, K, r, g, iters, scale)
        seen[i:i + 1].copy_(scale)
    return seen.cpu().numpy(), int(iters)


# ---- 1. the tick against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.KINDS)
def test_tick_against_the_oracle(kind):
    """16 launches from k = 0 run through the warm-up, the decay and four iterations past N.  One fp32 ulp: the device's fp64
    cos / pow may differ from the host's in the last fp64 bits, which moves the fp32 rounding by at most one step."""
    got, count = _ticks(kind, 16)
    want = np.array([ref.s32(kind, k, W, N, R, K, G) for k in range(16)], dtype=np.float32)
    ulps = [ref.ulps32(a, b) for a, b in zip(got, want)]
    print(f"\ntick {kind}: ulps against float32(s_ref(k)), k = 0..15: {ulps}")
    assert got.dtype == np.float32 and max(ulps) <= 1, (kind, got, want)
    assert count == 16


@pytest.mark.parametrize("kind", ["constant", "linear", "step"])
def test_tick_is_bit_exact_where_every_operation_is(kind):
    """Dyadic R and G: no cos, pow is exact - the device does the oracle's operations in the oracle's order."""
    got, _ = _ticks(kind, 16, r=0.125, g=0.5)
    want = np.array([ref.s32(kind, k, W, N, 0.125, K, 0.5) for k in range(16)], dtype=np.float32)
    assert got.tobytes() == want.tobytes(), (kind, got, want)


def test_the_count_saturates_and_the_scale_stays_at_the_floor():
    from dvg_amd import ops
    iters, scale = _buffers(INT_MAX - 1)
    for want in (INT_MAX, INT_MAX, INT_MAX):
        ops.lr_schedule_tick("linear", W, N, K, R, G, iters, scale)
        assert int(iters) == want and np.float32(float(scale)) == np.float32(R)


# ---- 2. scale 1 is the old kernel -----------------------------------------------------------------------------------------------------
HYPER = (2e-3, 0.9, 0.999, 1e-8)
# one grid pass covers 4096 x 256 x 4 floats: the last size is the smallest that runs the grid-stride loop a second time with a tail
SIZES = [1, 3, 4, 1027, 4 * 4096 * 256 + 1031]


@pytest.mark.parametrize("n", SIZES)
def test_scale_one_is_bit_identical_to_the_kernels_it_stands_for(n):
    """dvg_adam_step_scheduled with *lr_scale_dev == 1 on copies of the same buffers: against dvg_adam_step (no guard), against
    dvg_adam_step_guarded under stat = {., 0.37, 0, .}; with stat[2] = 1 nothing but the skip counter moves.  Host and device
    step counts, with and without weight decay."""
    from dvg_amd import ops
    torch.manual_seed(n % 1000)
    p, g, m, v = (torch.randn(n, device=DEV) for _ in range(4))
    v = v.abs()
    one = torch.ones(1, device=DEV)
    stat = torch.tensor([3.0, 0.37, 0.0, 3.0], device=DEV)
    t5 = torch.tensor([5], dtype=torch.int32, device=DEV)
    t7 = torch.tensor([7], dtype=torch.int32, device=DEV)
    for wd in (0.0, 0.01):
        for dev_step in (False, True):
            a, b = [t.clone() for t in (p, m, v)], [t.clone() for t in (p, m, v)]
            ops.adam_step(a[0], g, a[1], a[2], *HYPER, wd, 5, t5 if dev_step else None)
            ops.adam_step(b[0], g, b[1], b[2], *HYPER, wd, 5, t5 if dev_step else None, lr_scale=one)
            for x, y, name in zip(a, b, "pmv"):
                assert torch.equal(x, y), (n, wd, dev_step, name)
            assert not torch.equal(a[0], p)
            skips_a = torch.tensor([2], dtype=torch.int32, device=DEV)
            skips_b = skips_a.clone()
            a, b = [t.clone() for t in (p, m, v)], [t.clone() for t in (p, m, v)]
            ops.adam_step(a[0], g, a[1], a[2], *HYPER, wd, 7, t7 if dev_step else None, stat, skips_a)       # 7 - 2 skipped = 5
            ops.adam_step(b[0], g, b[1], b[2], *HYPER, wd, 7, t7 if dev_step else None, stat, skips_b, one)
            for x, y, name in zip(a, b, "pmv"):
                assert torch.equal(x, y), (n, wd, dev_step, name, "guarded")
            assert int(skips_a) == int(skips_b) == 2
    stat[2] = 1.0
    skips = torch.tensor([2], dtype=torch.int32, device=DEV)
    b = [t.clone() for t in (p, m, v)]
    ops.adam_step(b[0], g, b[1], b[2], *HYPER, 0.01, 7, None, stat, skips, one)
    assert int(skips) == 3 and all(torch.equal(x, y) for x, y in zip(b, (p, m, v)))


def test_the_rate_is_the_product_formed_in_fp64():
    """lr x scale in fp64 before the division by bc1: a scale of 1/2 is the step at half the rate, bit for bit (a power of two
    commutes with every rounding), and a scale of 0 moves the moments and not the parameters."""
    from dvg_amd import ops
    torch.manual_seed(2)
    n = 1027
    p, g, m, v = (torch.randn(n, device=DEV) for _ in range(4))
    v = v.abs()
    a, b, c = ([t.clone() for t in (p, m, v)] for _ in range(3))
    ops.adam_step(a[0], g, a[1], a[2], 1e-3, *HYPER[1:], 0.01, 3, None)
    ops.adam_step(b[0], g, b[1], b[2], 2e-3, *HYPER[1:], 0.01, 3, None, lr_scale=torch.full((1,), 0.5, device=DEV))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ops.adam_step(c[0], g, c[1], c[2], 2e-3, *HYPER[1:], 0.01, 3, None, lr_scale=torch.zeros(1, device=DEV))
    assert torch.equal(c[0], p) and torch.equal(c[1], a[1]) and torch.equal(c[2], a[2])


# ---- 3. against torch ----------------------------------------------------------------------------------------------------------------
def test_fused_adam_with_a_schedule_matches_torch_adam_with_lambda_lr():
    """test_fused_adam_matches_torch_adam's shapes and groups (the second with weight decay) and its bars, 7 steps through cosine
    W = 2, N = 6; at step 3 one parameter has no gradient (the per-parameter launches read the multiplier too)."""
    from dvg_amd import lr_schedule
    from dvg_amd.optim import FusedAdam
    torch.manual_seed(0)
    shapes = [(64, 3, 3, 3), (64,), (17, 5), (1,), (90, 40, 40)]
    theirs = [torch.nn.Parameter(torch.randn(*s, device=DEV)) for s in shapes]
    mine = [torch.nn.Parameter(p.detach().clone()) for p in theirs]
    mk = lambda cls, ps: cls([{"params": ps[:3]}, {"params": ps[3:], "weight_decay": 0.01}], lr=2e-3)  # noqa: E731
    o_ref, o_mine = mk(torch.optim.Adam, theirs), mk(FusedAdam, mine)
    s_ref = torch.optim.lr_scheduler.LambdaLR(o_ref, lambda k: ref.s("cosine", k, 2, 6, 0.0))
    sched = lr_schedule.LrSchedule({"kind": "cosine", "warmup": 2, "total": 6, "min_ratio": 0.0, "step_every": 1, "gamma": 1.0,
                                    "lr": 2e-3}, DEV)
    sched.attach([o_mine])
    assert o_mine.lr_scale is sched.scale
    sd_before = o_mine.state_dict()
    for it in range(7):
        grads = [torch.randn_like(p) for p in theirs]
        for p, q, g in zip(theirs, mine, grads):
            p.grad, q.grad = g.clone(), g.clone()
        if it == 3:
            theirs[1].grad = None
            mine[1].grad = None
        assert abs(o_ref.param_groups[0]["lr"] - 2e-3 * ref.s("cosine", it, 2, 6)) < 1e-18
        sched.tick()
        o_ref.step()
        o_mine.step()
        s_ref.step()
        assert float(sched.scale) == float(ref.s32("cosine", it, 2, 6))
        for p, q in zip(theirs, mine):
            assert torch.allclose(p, q, rtol=2e-6, atol=2e-7), it
    assert [g["lr"] for g in o_mine.param_groups] == [2e-3, 2e-3]                   # the base rate stays where it is
    assert sorted(o_mine.state_dict()) == sorted(sd_before)                           # state_dict() has no new key
    assert sched.read() == {"iters": 7, "scale": 0.0}


# ---- the Trainer ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batches():
    return train_harness.make_batches(5)


def test_trainer_builds_a_schedule_only_when_asked():
    plain = train_harness.trainer()
    assert plain.lr_schedule is None and all(o.lr_scale is None for o in plain.optimizers())
    assert {g["lr"] for o in plain.optimizers() for g in o.param_groups} == {0.002}
    assert "lr_schedule" not in plain.state_dict()
    tr = train_harness.trainer(["--lr_schedule", "cosine", "--lr_warmup", "4", "--lr_total", "9", "--lr", "0.01"])
    assert {g["lr"] for o in tr.optimizers() for g in o.param_groups} == {0.01}     # --lr is the base rate of all four
    assert all(o.lr_scale is tr.lr_schedule.scale for o in tr.optimizers())
    assert float(tr.lr_schedule.scale) == 0.25 and int(tr.lr_schedule.iters) == 0   # s(0) = 1 / W before the first tick
    line = tr.lr_schedule.epoch_line()
    assert "cosine" in line and "0 / 9" in line and "0.25" in line and "0.0025" in line, line
    from dvg_amd import graphs
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="capture"):
        with graphs.capturing():
            tr.lr_schedule.epoch_line()


# ---- 4. a zero rate moves nothing ----------------------------------------------------------------------------------------------------
def test_a_zero_rate_moves_no_parameter(batches):
    """linear, R = 0, the count set to N: the multiplier of the iteration is exactly 0.  All six Adam launches run - the moments
    move - and no parameter changes a bit."""
    tr = train_harness.trainer(["--lr_schedule", "linear", "--lr_total", "8"])
    tr.gp_layer(torch.zeros(4, 90, device=DEV))          # the one-off prior initialisation of the variational parameters
    tr.lr_schedule.load_state(8)
    before = train_harness.arena(tr)
    tr.iteration(batches[0])
    torch.cuda.synchronize()
    assert tr.lr_schedule.read() == {"iters": 9, "scale": 0.0}
    assert torch.equal(tr.arena.p, before["p"])
    assert not torch.equal(tr.arena.m, before["m"]) and not torch.equal(tr.arena.v, before["v"])


# ---- 5. the flag alone changes nothing ----------------------------------------------------------------------------------------------
def _iterate(tr, xs, graphed=False, warmup=2):
    step, out = train_harness.iterate(tr, xs, graphed, warmup, each=lambda tr, step, i: (
        tr.last_loss, step.graph if graphed else None, tr.lr_schedule.read() if tr.lr_schedule is not None else None))
    return step, [(res + (loss,), graph, sched) for res, (loss, graph, sched) in out]


def test_constant_at_the_reference_rate_is_the_run_without_the_flag(batches):
    """--lr_schedule constant --lr 0.002, no warm-up: the multiplier is 1 at every iteration, so every Adam launch has the operands
    of the unscheduled one - parameters and both moments bit-equal after three eager iterations from one seed."""
    plain, sched = train_harness.trainer(), train_harness.trainer(["--lr_schedule", "constant", "--lr", "0.002"])
    _iterate(plain, batches[:3])
    _iterate(sched, batches[:3])
    a, b = train_harness.arena(plain), train_harness.arena(sched)
    for n in a:
        assert torch.equal(a[n], b[n]), n
    assert sched.lr_schedule.read() == {"iters": 3, "scale": 1.0}


# ---- 6. one capture -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["dcgan", "vgg"])
def test_one_capture_serves_a_multiplier_that_moves_every_iteration(batches, model):
    """GraphedIteration under cosine W = 2, N = 5, five iterations (two eager, the capture, two more replays) against the eager
    loop, within test_graphed_iteration_matches_eager's bars; the graph of the first replay is the graph of the last, and the
    multiplier read after iteration i is the oracle's s(i - 1) in both runs."""
    flags = ["--lr_schedule", "cosine", "--lr_warmup", "2", "--lr_total", "5"]
    res = []
    for graphed in (False, True):
        tr = train_harness.trainer(flags, seed=11, model=model)
        step, out = _iterate(tr, batches[:5], graphed, warmup=2)
        for i, (_, _, d) in enumerate(out, start=1):
            assert d["iters"] == i and np.float32(d["scale"]) == ref.s32("cosine", i - 1, 2, 5), (graphed, i, d)
        if graphed:
            assert not step.failed and out[2][1] is not None and all(g is out[2][1] for _, g, _ in out[2:])
            assert out[0][1] is None and out[1][1] is None and step.calls == 5
        res.append(([o[0] for o in out], [{k: t.detach().clone() for k, t in m.state_dict().items()} for m in tr.modules], train_harness.arena(tr),
                    float(tr.encoder_optimizer.state_dict()["state"][0]["step"])))
    (la, sa, aa, stepa), (lb, sb, ab, stepb) = res
    assert stepa == stepb == 5.0
    for a, b in zip(la, lb):
        for u, v in zip(a, b):
            assert abs(u - v) <= 2e-4 * max(1.0, abs(u)), (la, lb)
    for a, b in zip(sa, sb):                             # parameters and buffers of every module
        for k in a:
            assert torch.allclose(a[k].float(), b[k].float(), rtol=2e-3, atol=2e-5), k
    for n in ("m", "v"):                                 # the optimisers' state
        assert torch.allclose(aa[n], ab[n], rtol=2e-3, atol=2e-5), n


# ---- 7. guard and resume --------------------------------------------------------------------------------------------------------------
def test_a_skipped_step_still_counts_as_an_iteration(batches):
    """--skip_nonfinite: an Inf written into one encoder gradient right before the steps of the second iteration's train_model
    site.  The site is skipped - parameters and moments bit-equal across it - and the count of iterations has advanced all the
    same: it counts iterations, not optimiser steps."""
    from dvg_amd import train_state
    tr = train_harness.trainer(["--skip_nonfinite", "--lr_schedule", "linear", "--lr_warmup", "2", "--lr_total", "10"])
    seen = {"site": 0}
    orig, whole = tr._ar, (tr.rng_gp[0], tr.rng_enc[1])

    def ar(*actions):
        orig(*actions)
        last = actions[-1]
        if "before" in seen and "after" not in seen:     # the next all-reduce point: the fine-tuning site's
            seen["after"], seen["iters_after"] = train_harness.arena(tr), int(tr.lr_schedule.iters)
        if last == ("finish", "b") or (last[0] == "reduce" and tuple(last[1]) == whole):
            if seen["site"] == 1:
                seen["before"] = train_harness.arena(tr)
                tr.arena.g[tr.rng_enc[0] + 5] = float("inf")
            seen["site"] += 1
    tr._ar = ar
    _iterate(tr, batches[:3])
    for n in ("p", "m", "v"):
        assert torch.equal(seen["before"][n], seen["after"][n]), n
    assert seen["iters_after"] == 2                      # the tick of the skipped iteration had run
    d = tr.guard.read_and_reset()
    assert (d["sites"], d["skipped"]) == (6, 1)
    assert tr.lr_schedule.read() == {"iters": 3, "scale": float(ref.s32("linear", 2, 2, 10))}
    sd = tr.state_dict()
    assert sd["lr_schedule"]["iters"] == 3 and sd["global_step"] == train_state.global_step(tr) == 2
    assert all(bool(torch.isfinite(getattr(tr.arena, n)).all()) for n in ("p", "m", "v"))


RESUME_FLAGS = ["--lr_schedule", "cosine", "--lr_warmup", "2", "--lr_total", "6", "--lr_min_ratio", "0.1"]


def _run(n, resume_after=None, flags=RESUME_FLAGS, load_flags=None):
    """tests/test_gpu_resume.py's `_run`, eager: n iterations from seed 3 on the continued data stream; resume_after = k: after k
    iterations the state goes through a file image into a FRESH Trainer with another seed, in front of a fresh data stream."""
    import train
    from dvg_amd.data import make_batch_generator

    def stream():
        return train.BatchPrefetcher(make_batch_generator(train_harness.opt(), 4, 5, torch.device(DEV)))
    tr, gen = train_harness.trainer(flags, seed=3), stream()
    tr.scheduler.step()
    for i in range(n):
        if resume_after is not None and i == resume_after:
            f = io.BytesIO()
            torch.save(tr.state_dict(epoch=0, train_gen=gen), f)
            f.seek(0)
            del tr
            tr, gen = train_harness.trainer(flags if load_flags is None else load_flags, seed=99), stream()
            tr.load_state_dict(torch.load(f, weights_only=False), train_gen=gen)
        tr.iteration(next(gen)())
    torch.cuda.synchronize()
    return tr


def test_a_resumed_run_takes_the_same_third_iteration():
    """Two iterations, the state through a file image into a fresh Trainer, a third: arena.p bit-equal to the uninterrupted run's
    (A against A is printed first: it shows whether the eager loop itself repeats its bits on this machine)."""
    a = _run(3)
    pa = a.arena.p.clone()
    assert a.lr_schedule.read() == {"iters": 3, "scale": float(ref.s32("cosine", 2, 2, 6, 0.1))}
    a2 = _run(3)
    print(f"\nA vs A, three scheduled iterations: max |dp| = {float((a2.arena.p - pa).abs().max()):.3e}")
    del a, a2
    b = _run(3, resume_after=2)
    print(f"resumed vs A: max |dp| = {float((b.arena.p - pa).abs().max()):.3e}")
    assert torch.equal(b.arena.p, pa)
    assert b.lr_schedule.read() == {"iters": 3, "scale": float(ref.s32("cosine", 2, 2, 6, 0.1))}


def test_restore_refuses_another_spec_and_says_what_it_does_with_old_and_unwanted_states(batches, capsys):
    saver = train_harness.trainer(RESUME_FLAGS)
    saver.iteration(batches[0])
    sd = saver.state_dict(epoch=0)
    assert sd["lr_schedule"] == {"spec": dict(saver.lr_schedule.spec), "iters": 1}
    with pytest.raises(SystemExit, match="lr_schedule.total "):          # another spec than the saved one: the field is named
        train_harness.trainer(RESUME_FLAGS[:5] + ["7"] + RESUME_FLAGS[6:]).load_state_dict(sd)
    capsys.readouterr()
    dropped = train_harness.trainer()                                                 # a state with the key, restored without the flag
    dropped.load_state_dict(sd)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "ignored" in out and dropped.lr_schedule is None
    old_sd = dropped.state_dict(epoch=0)                                 # ... and what it writes is a state from before the flag
    assert "lr_schedule" not in old_sd and old_sd["global_step"] == 1
    late = train_harness.trainer(["--lr_schedule", "constant"])
    late.load_state_dict(old_sd)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "counts from global step 1" in out and late.lr_schedule.read()["iters"] == 1
    with pytest.raises(SystemExit, match="lr_schedule.lr "):             # the restored rate of the optimisers is not this --lr
        train_harness.trainer(["--lr_schedule", "constant", "--lr", "0.01"]).load_state_dict(old_sd)
