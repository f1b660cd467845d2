"""GPU: train.py --optimizer / --weight_decay - dvg_optim_step against the fp64 restatement (tests/optim_ref.py) and the torch
classes, its bit equalities with dvg_adam_step and with itself under a mask, a guard and a schedule, the Fused* classes against
torch.optim's, what a Trainer decays, the rules inside a GraphedIteration, the untouched default, resume, and train.py end to end.

Bars: rtol 2e-6, atol 2e-7 on the parameters, those of tests/test_gpu_train.py::test_fused_adam_matches_torch_adam.

The restatement is given the hyper-parameters the kernel is given: the C ABI carries lr, a, b, eps and weight_decay as fp32, so
`_f32` rounds them first (beta2 = 0.999 is off by 2e-8 in fp32, and 1 - beta2 - the weight of every gradient in exp_avg_sq - by 2e-5
of itself; under RMSprop with weight decay, an element whose g + wd p nearly cancels moves by 10 lr times the sign of what is left,
so the last bits of wd decide it).  The arithmetic is what the tests compare, on the same inputs.

The state buffers are held to rtol 2e-6 and an absolute 4 * STEPS * 2^-24 * max|buffer|: an update of a buffer is at most four
fp32 operations, each rounded to half an ulp of a value no larger than the buffer's largest; where two terms of an update
cancel, a relative bar says nothing."""
import os

import numpy as np
import pytest
import torch

from tests import optim_ref as ref
from tests import train_harness

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 2e-6, 2e-7
LR = 2e-3
STRIDE = 4096 * 256 * 4              # floats one sweep of the capped grid covers: 4 194 304
BIG = STRIDE + 1027
IDS = [c[0] for c in ref.CASES]


@pytest.fixture(scope="module")
def data():
    """Standard-normal parameters and 5 gradients of the largest size, made once; a size n uses their first n values."""
    g = torch.Generator(device="cpu").manual_seed(12)
    p = torch.randn(BIG, generator=g)
    grads = [torch.randn(BIG, generator=g) for _ in range(5)]
    return {"p": p.to(DEV), "g": [x.to(DEV) for x in grads]}


def _run(rule, p0, grads, a, b, wd, nesterov=False, mask=None, stat=None, skips=None, scale=None, device_count=False):
    """Steps of dvg_optim_step from zero state; returns (p, m, v)."""
    from dvg_amd import ops
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for t, g in enumerate(grads, 1):
        tdev = torch.tensor([t], dtype=torch.int32, device=p.device) if device_count else None
        ops.optim_step(rule, p, g, m, None if rule == ref.SGD else v, LR, a, b, 1e-8, wd, ops.NESTEROV if nesterov else 0, mask,
                       0 if device_count else t, tdev, stat, skips, scale)
    torch.cuda.synchronize()
    return p, m, v


def _close(got, want, what):
    want = torch.as_tensor(want, dtype=torch.float64, device=got.device)
    err = float((got.double() - want).abs().max())
    print(f"{what}: max |error| {err:.3e}")
    assert torch.allclose(got.double(), want, rtol=RTOL, atol=ATOL), (what, err)


def _close_state(got, want, steps, what):
    want = torch.as_tensor(want, dtype=torch.float64, device=got.device)
    atol = 4 * steps * 2.0 ** -24 * float(want.abs().max())
    err = float((got.double() - want).abs().max())
    print(f"{what}: max |error| {err:.3e} (absolute bar {atol:.3e})")
    assert torch.allclose(got.double(), want, rtol=RTOL, atol=atol), (what, err, atol)


def _f32(x):
    """The value of a hyper-parameter once the C ABI has carried it as a float."""
    return float(np.float32(x))


def _ref(rule, p0, grads, a, b, wd, nesterov, **kw):
    """The restatement on the kernel's inputs: fp32 parameters and gradients, fp32-rounded hyper-parameters."""
    return ref.run(rule, p0.cpu().numpy(), [g.cpu().numpy() for g in grads], _f32(LR), _f32(a), _f32(b), eps=_f32(1e-8),
                   weight_decay=_f32(wd), nesterov=nesterov, **kw)


# ---- 1. against the restatement and the torch class ---------------------------------------------------------------------------
@pytest.mark.parametrize("wd", ref.DECAYS)
@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_kernel_matches_the_restatement_and_the_torch_class(case, wd, data):
    name, rule, a, b, nesterov = case
    for n, steps in ((1, 5), (3, 5), (1027, 5), (BIG, 2)):
        p0, grads = data["p"][:n].clone(), [g[:n].clone() for g in data["g"][:steps]]
        p, m, v = _run(rule, p0, grads, a, b, wd, nesterov)
        rp, rm, rv = _ref(rule, p0, grads, a, b, wd, nesterov)
        _close(p, rp, f"{name} wd {wd} n {n} p vs fp64")
        if rule != ref.SGD or a != 0:
            if rule != ref.RMSPROP or b > 0:
                _close_state(m, rm, steps, f"{name} wd {wd} n {n} m vs fp64")
        if rule != ref.SGD:
            _close_state(v, rv, steps, f"{name} wd {wd} n {n} v vs fp64")
        else:
            assert not v.any()                              # SGD leaves the second buffer alone
        q = torch.nn.Parameter(p0.clone())
        o = ref.torch_optimizer(rule, [q], LR, a, b, weight_decay=wd, nesterov=nesterov)
        for g in grads:
            q.grad = g.clone()
            o.step()
        _close(p, q.detach(), f"{name} wd {wd} n {n} p vs torch on the device")


# ---- 2. bit equalities ---------------------------------------------------------------------------------------------------------
def _adam(p0, grads, wd):
    from dvg_amd import ops
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for t, g in enumerate(grads, 1):
        ops.adam_step(p, g, m, v, LR, 0.9, 0.999, 1e-8, wd, t, None)
    return p, m, v


def _same(x, y):
    return all(torch.equal(s, t) for s, t in zip(x, y))


@pytest.mark.parametrize("n", [1027, BIG])
def test_rule_0_and_rule_1_have_the_bits_of_dvg_adam_step(n, data):
    p0, grads = data["p"][:n].clone(), [g[:n] for g in data["g"][:3]]
    ones = torch.ones((n + 3) // 4, dtype=torch.uint8, device=DEV)
    for wd in ref.DECAYS:
        want = _adam(p0, grads, wd)
        assert _same(_run(ref.ADAM, p0, grads, 0.9, 0.999, wd), want), wd
        assert _same(_run(ref.ADAM, p0, grads, 0.9, 0.999, wd, mask=ones), want), wd
        assert _same(_run(ref.ADAM, p0, grads, 0.9, 0.999, wd, mask=ones * 255), want), wd
    assert _same(_run(ref.ADAMW, p0, grads, 0.9, 0.999, 0.0), _adam(p0, grads, 0.0))
    assert not _same(_run(ref.ADAMW, p0, grads, 0.9, 0.999, 0.01), _adam(p0, grads, 0.01))      # the two decays differ


@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_all_ones_mask_is_no_mask_and_a_mixed_mask_selects_per_piece(case, data):
    """n = one sweep of the capped grid + 1027: bytes 0 at the first piece, the last whole piece, the tail piece, one side of
    two 256-piece block boundaries and a piece only the second stride reaches; random bytes (0, 1, 255) elsewhere."""
    name, rule, a, b, nesterov = case
    n, wd = BIG, 0.01
    p0, grads = data["p"][:n].clone(), [g[:n] for g in data["g"][:2]]
    pieces = (n + 3) // 4
    assert n % 4 == 3 and pieces - 1 == n // 4 > STRIDE // 4
    g = torch.Generator(device="cpu").manual_seed(3)
    mask = torch.tensor([0, 1, 255], dtype=torch.uint8)[torch.randint(0, 3, (pieces,), generator=g)]
    second_stride = STRIDE // 4 + 5
    mask[[0, pieces - 2, pieces - 1, 255, 512, second_stride]] = 0
    mask[[1, pieces - 3, 256, 511, second_stride + 1, second_stride - 1]] = 1
    mask = mask.to(DEV)
    full = _run(rule, p0, grads, a, b, wd, nesterov)
    assert _same(_run(rule, p0, grads, a, b, wd, nesterov, mask=torch.ones_like(mask)), full)
    none = _run(rule, p0, grads, a, b, 0.0, nesterov)
    mixed = _run(rule, p0, grads, a, b, wd, nesterov, mask=mask)
    off = torch.repeat_interleave(mask == 0, 4)[:n]
    assert bool(off[0]) and bool(off[-1]) and bool(off[n - 4]) and int(off.sum()) > n // 4
    for got, decayed, bare in zip(mixed, full, none):
        assert torch.equal(got[off], bare[off]) and torch.equal(got[~off], decayed[~off]), name
    assert not torch.equal(full[0][off], none[0][off])       # the decay does change these bits


@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_guard_schedule_and_step_count_forms_have_the_same_bits(case, data):
    name, rule, a, b, nesterov = case
    n, wd = 1027, 0.01
    p0, grads = data["p"][:n].clone(), [g[:n] for g in data["g"][:3]]
    stat = torch.tensor([5.0, 1.0, 0.0, 7.0], device=DEV)
    skips = torch.zeros(1, dtype=torch.int32, device=DEV)
    one = torch.ones(1, device=DEV)
    plain = _run(rule, p0, grads, a, b, wd, nesterov)
    assert _same(_run(rule, p0, grads, a, b, wd, nesterov, stat=stat, skips=skips), plain), name
    assert _same(_run(rule, p0, grads, a, b, wd, nesterov, scale=one), plain), name
    assert _same(_run(rule, p0, grads, a, b, wd, nesterov, stat=stat, skips=skips, scale=one), plain), name
    assert _same(_run(rule, p0, grads, a, b, wd, nesterov, device_count=True), plain), name
    assert int(skips) == 0
    # the clip factor: the product with the gradient is rounded on its own
    stat[1] = 0.37
    scaled = [g * stat[1] for g in grads]
    assert _same(_run(rule, p0, grads, a, b, wd, nesterov, stat=stat, skips=skips), _run(rule, p0, scaled, a, b, wd, nesterov)), name
    # the rate multiplier: (double)lr * scale, against the restatement (no fp32 rate to pre-multiply bit for bit)
    half = torch.full((1,), 0.25, device=DEV)
    p = _run(rule, p0, grads, a, b, wd, nesterov, scale=half)[0]
    rp = _ref(rule, p0, grads, a, b, wd, nesterov, lr_scale=0.25)[0]
    _close(p, rp, f"{name} at a quarter of the rate")
    # a skipped step: nothing but the counter moves, and the next step's bias corrections do not count it
    stat[1], stat[2] = 1.0, 1.0
    from dvg_amd import ops
    p, m, v = _run(rule, p0, grads[:1], a, b, wd, nesterov)
    kept = (p.clone(), m.clone(), v.clone())
    args = (rule, p, grads[1], m, None if rule == ref.SGD else v, LR, a, b, 1e-8, wd, ops.NESTEROV if nesterov else 0, None)
    ops.optim_step(*args, 2, None, stat, skips)
    torch.cuda.synchronize()
    assert _same((p, m, v), kept) and int(skips) == 1, name
    stat[2] = 0.0
    ops.optim_step(*args, 3, None, stat, skips)              # host count 3, one skipped: the second step applied
    torch.cuda.synchronize()
    assert _same((p, m, v), _run(rule, p0, grads[:2], a, b, wd, nesterov)) and int(skips) == 1, name


# ---- 3. the classes against torch's ------------------------------------------------------------------------------------------
CLASSES = [("adamw", "FusedAdamW", torch.optim.AdamW, {}),
           ("sgd_nesterov", "FusedSGD", torch.optim.SGD, {"momentum": 0.9, "nesterov": True}),
           ("sgd_plain", "FusedSGD", torch.optim.SGD, {}),
           ("rmsprop", "FusedRMSprop", torch.optim.RMSprop, {}),
           ("rmsprop_momentum", "FusedRMSprop", torch.optim.RMSprop, {"momentum": 0.9})]


@pytest.mark.parametrize("arena", [False, True], ids=["own", "arena"])
@pytest.mark.parametrize("case", CLASSES, ids=[c[0] for c in CLASSES])
def test_fused_classes_match_the_torch_classes(case, arena):
    """test_fused_adam_matches_torch_adam's scenario for the new classes: two groups (the second with weight decay), a rate change
    from MultiStepLR, a step with one gradient missing, version counters, state_dict into the torch class and back."""
    from dvg_amd import optim
    name, mine_cls, ref_cls, kw = case
    mine_cls = getattr(optim, mine_cls)
    torch.manual_seed(0)
    shapes = [(64, 3, 3, 3), (64,), (17, 5), (1,), (90, 40, 40)]
    ref_p = [torch.nn.Parameter(torch.randn(*s, device=DEV)) for s in shapes]
    mine = [torch.nn.Parameter(p.detach().clone()) for p in ref_p]

    def groups(ps):
        return [{"params": ps[:3], "weight_decay": 0.0}, {"params": ps[3:], "weight_decay": 0.01}]

    def fused(ps):
        extra = {"arena": optim.FlatArena(optim.FlatArena.size_for(ps), DEV)} if arena else {}
        return mine_cls(groups(ps), lr=2e-3, **kw, **extra)
    o_ref, o_mine = ref_cls(groups(ref_p), lr=2e-3, **kw), fused(mine)
    assert (o_mine.arena is not None) == arena and mine[0].data_ptr() == o_mine._flat[0]["p"].data_ptr()
    s_ref = torch.optim.lr_scheduler.MultiStepLR(o_ref, milestones=[2], gamma=0.1)
    s_mine = torch.optim.lr_scheduler.MultiStepLR(o_mine, milestones=[2], gamma=0.1)
    for it in range(5):
        grads = [torch.randn_like(p) for p in ref_p]
        for p, q, g in zip(ref_p, mine, grads):
            p.grad, q.grad = g.clone(), g.clone()
        if it == 3:                       # partially used group: torch skips the parameter without a gradient
            ref_p[1].grad = None
            mine[1].grad = None
        v0 = mine[0]._version
        o_ref.step()
        o_mine.step()
        s_ref.step()
        s_mine.step()
        assert mine[0]._version > v0, "weight caches key on the version counter"
        for p, q in zip(ref_p, mine):
            assert torch.allclose(p, q, rtol=RTOL, atol=ATOL), (name, it, float((p - q).abs().max()))
    assert o_mine.param_groups[0]["lr"] == pytest.approx(2e-4)
    sd = o_mine.state_dict()
    assert all("decay_mask" not in g for g in sd["param_groups"])
    for t in (t for st in sd["state"].values() for t in st.values() if torch.is_tensor(t)):
        assert t.untyped_storage().nbytes() == t.numel() * t.element_size()          # owned copies, not arena views
    o_new = ref_cls(groups([torch.nn.Parameter(p.detach().clone()) for p in mine]), lr=2e-3, **kw)
    o_new.load_state_dict(sd)             # interchangeable state layout
    theirs = o_ref.state_dict()["state"]
    assert set(sd["state"]) == set(theirs)
    for k, st in theirs.items():
        assert set(sd["state"][k]) == set(st), (name, k, sorted(sd["state"][k]), sorted(st))
        for key, t in st.items():
            if key == "step":
                assert float(sd["state"][k][key]) == float(t) == (4.0 if k == 1 else 5.0)
            elif t is None:
                assert sd["state"][k][key] is None
            else:
                # two fp32 implementations whose weights 1 - c differ by up to 2^-24 / (1 - c) of themselves (torch rounds
                # 1 - c from fp64, the kernel forms it from the fp32 c; c: the rule's coefficient nearest 1): 5 steps of that,
                # relative to the largest entry
                c = {"adamw": 0.999, "sgd_nesterov": 0.9, "sgd_plain": 0.9, "rmsprop": 0.99, "rmsprop_momentum": 0.99}[name]
                bar = 5 * 2.0 ** -24 / (1 - c) * float(t.abs().max())
                assert torch.allclose(sd["state"][k][key], t, rtol=1e-5, atol=bar), (name, k, key, float((sd["state"][k][key] - t).abs().max()), bar)
    o_back = fused(mine)
    o_back.load_state_dict(o_ref.state_dict())
    for p, q in zip(ref_p, mine):
        g = torch.randn_like(p)
        p.grad, q.grad = g.clone(), g.clone()
    o_ref.step()
    o_back.step()
    for p, q in zip(ref_p, mine):
        assert torch.allclose(p, q, rtol=RTOL, atol=ATOL), name


def test_fused_adam_with_a_mask_goes_through_rule_0_and_matches_two_torch_groups(monkeypatch):
    """One FusedAdam group with weight decay and a mask over its first parameter only, against torch.optim.Adam with that
    parameter in a group of its own; a FusedAdam constructed as always - weight decay, no mask - never calls ops.optim_step."""
    from dvg_amd import ops, optim
    calls = []
    real = ops.optim_step
    monkeypatch.setattr(ops, "optim_step", lambda *a, **k: (calls.append(a[0]), real(*a, **k))[1])
    torch.manual_seed(1)
    shapes = [(33, 7), (33,), (5, 5)]
    ref_p = [torch.nn.Parameter(torch.randn(*s, device=DEV)) for s in shapes]
    mine = [torch.nn.Parameter(p.detach().clone()) for p in ref_p]
    plain = [torch.nn.Parameter(p.detach().clone()) for p in ref_p]
    o_ref = torch.optim.Adam([{"params": ref_p[:1], "weight_decay": 0.05}, {"params": ref_p[1:]}], lr=2e-3)
    o_mine, o_plain = optim.FusedAdam(mine, lr=2e-3, weight_decay=0.05), optim.FusedAdam(plain, lr=2e-3, weight_decay=0.05)
    o_mine.set_decay_mask(0, optim.decay_mask(mine, lambda p: p is mine[0]).to(DEV))
    assert o_mine.param_groups[0]["decay_mask"].tolist() == [1] * 58 + [0] * 9 + [0] * 7
    for it in range(3):
        for p, q, r in zip(ref_p, mine, plain):
            g = torch.randn_like(p)
            p.grad, q.grad, r.grad = g.clone(), g.clone(), g.clone()
        o_ref.step()
        o_plain.step()
        assert calls == [ops.ADAM] * it
        o_mine.step()
        for p, q in zip(ref_p, mine):
            assert torch.allclose(p, q, rtol=RTOL, atol=ATOL), it
    assert torch.allclose(plain[0], mine[0], rtol=RTOL, atol=ATOL) and not torch.allclose(plain[2], mine[2], rtol=RTOL, atol=ATOL)
    assert calls == [ops.ADAM] * 3
    assert "decay_mask" not in o_mine.state_dict()["param_groups"][0] and "decay_mask" not in o_mine.host_state()["param_groups"][0]
    with pytest.raises(ValueError, match="decay_mask"):
        o_mine.set_decay_mask(0, torch.ones(3, dtype=torch.uint8, device=DEV))


# ---- 4. what a Trainer decays --------------------------------------------------------------------------------------------------
def test_trainer_decays_the_weight_matrices_of_three_modules_and_nothing_else():
    from dvg_amd import train_state
    tr = train_harness.trainer(["--optimizer", "adamw", "--weight_decay", "0.1"])
    assert [type(o).__name__ for o in tr.optimizers()] == ["FusedAdamW"] * 4
    tr.arena.g.zero_()
    before = tr.arena.p.clone()
    for o in tr.optimizers():
        o.step()
    torch.cuda.synchronize()
    decays = torch.zeros(before.numel(), dtype=torch.bool, device=DEV)
    n_decaying = 0
    for name, o in train_state.named_optimizers(tr):
        for f in o._flat.values():
            for p, off in zip(f["params"], f["offsets"]):
                if name in ("encoder", "decoder", "frame_predictor") and p.dim() >= 2:
                    decays[f["lo"] + off:f["lo"] + off + p.numel()] = True
                    n_decaying += p.numel()
    assert 0 < n_decaying < before.numel() and not decays[slice(*tr.rng_gp)].any()
    after = tr.arena.p
    assert torch.equal(after[~decays], before[~decays])                  # biases, BatchNorm, GP, likelihood, padding: the same bits
    want = (before.double() * (1.0 - 0.002 * 0.1)).float()
    lo, hi = torch.nextafter(want, want.new_full((), -float("inf"))), torch.nextafter(want, want.new_full((), float("inf")))
    assert bool(((after >= lo) & (after <= hi))[decays].all())           # p (1 - lr wd) to one ulp
    assert not torch.equal(after[decays], before[decays])
    line = tr.optim_report.epoch_line()
    assert "adamw" in line and "weight decay 0.1" in line and f"of {before.numel()} floats" in line


# ---- 5. the rules inside a hipGraph ----------------------------------------------------------------------------------------------
# --lr_total: the harness options train for niter * epoch_size = 1 iteration, which no warm-up of 2 fits into
ALL_ON = ["--clip_grad_norm", "1", "--skip_nonfinite", "--lr_schedule", "cosine", "--lr_warmup", "2", "--lr_total", "6", "--ema_decay", "0.9"]
GRAPH_CASES = [("adamw", ["--optimizer", "adamw", "--weight_decay", "0.01"]),
               ("sgd", ["--optimizer", "sgd", "--nesterov", "--weight_decay", "0.01"]),
               ("rmsprop", ["--optimizer", "rmsprop", "--momentum", "0.9", "--weight_decay", "0.01", "--lr", "2e-4"]),
               ("adamw_all_on", ["--optimizer", "adamw", "--weight_decay", "0.01"] + ALL_ON)]


@pytest.mark.parametrize("case", GRAPH_CASES, ids=[c[0] for c in GRAPH_CASES])
def test_graphed_iteration_matches_eager_under_every_rule(case):
    """Three harness iterations eagerly and as a GraphedIteration from one seed, to test_graphed_iteration_matches_eager's bars:
    losses 2e-4 relative, arena and BatchNorm buffers rtol 2e-3, atol 2e-5.  iterate() asserts that the graph did not fall back."""
    from dvg_amd import train_state
    xs = train_harness.make_batches(3)
    res = []
    for graphed in (False, True):
        tr = train_harness.trainer(case[1])
        _, out = train_harness.iterate(tr, xs, graphed, warmup=1, each=lambda tr, step, i: tr.last_loss)
        res.append(([triple + (loss,) for triple, loss in out], train_harness.arena(tr),
                    {k: b.clone() for k, b in train_state.named_buffers(tr)},
                    [o.host_state()["steps"] for o in tr.optimizers()]))
    (la, aa, ba, sa), (lb, ab, bb, sb) = res
    assert sa == sb
    for a, b in zip(la, lb):
        for u, v in zip(a, b):
            assert abs(u - v) <= 2e-4 * max(1.0, abs(u)), (la, lb)
    for k in ("p", "m", "v"):
        assert torch.allclose(aa[k], ab[k], rtol=2e-3, atol=2e-5), (case[0], k, float((aa[k] - ab[k]).abs().max()))
    for k in ba:
        assert torch.allclose(ba[k].float(), bb[k].float(), rtol=2e-3, atol=2e-5), (case[0], k)


# ---- 6. nothing moves by default -------------------------------------------------------------------------------------------------
def test_adam_without_weight_decay_issues_the_launches_of_before(monkeypatch):
    from dvg_amd import ops
    calls = {"optim": 0, "adam": 0}
    real_optim, real_adam = ops.optim_step, ops.adam_step
    monkeypatch.setattr(ops, "optim_step", lambda *a, **k: (calls.__setitem__("optim", calls["optim"] + 1), real_optim(*a, **k))[1])
    monkeypatch.setattr(ops, "adam_step", lambda *a, **k: (calls.__setitem__("adam", calls["adam"] + 1), real_adam(*a, **k))[1])
    xs = train_harness.make_batches(2)
    arenas = []
    for flags in ([], ["--optimizer", "adam", "--weight_decay", "0"]):
        tr = train_harness.trainer(flags)
        assert tr.optim_report is None and [type(o).__name__ for o in tr.optimizers()] == ["FusedAdam"] * 4
        train_harness.iterate(tr, xs)
        arenas.append(train_harness.arena(tr))
    for k in ("p", "m", "v"):
        assert torch.equal(arenas[0][k], arenas[1][k]), k
    assert calls["optim"] == 0 and calls["adam"] > 0


# ---- 7. resume ---------------------------------------------------------------------------------------------------------------------
def test_sgd_run_resumes_to_the_same_bits():
    """Four eager iterations in one go against 2 + (save, fresh Trainer with another seed, load) + 2 on the continued data stream."""
    import io
    import train
    from dvg_amd.data import make_batch_generator
    flags = ["--optimizer", "sgd", "--weight_decay", "0.01"]

    def stream():
        return train.BatchPrefetcher(make_batch_generator(train_harness.opt(flags), 4, 5, torch.device(DEV)))

    def run(resume_after=None):
        tr, gen = train_harness.trainer(flags, seed=3), stream()
        tr.scheduler.step()
        for i in range(4):
            if i == resume_after:
                f = io.BytesIO()
                torch.save(tr.state_dict(epoch=0, train_gen=gen), f)
                f.seek(0)
                tr, gen = train_harness.trainer(flags, seed=99), stream()
                tr.load_state_dict(torch.load(f, weights_only=False), train_gen=gen)
            tr.iteration(next(gen)())
        torch.cuda.synchronize()
        return tr
    a, b = run(), run(resume_after=2)
    assert type(a.encoder_optimizer).__name__ == "FusedSGD" and a.state_dict(0)["fingerprint"]["optimizer"] == "sgd"
    for k in ("p", "m", "v"):
        assert torch.equal(getattr(a.arena, k), getattr(b.arena, k)), k
    assert not a.arena.v.any()              # SGD never touches the second buffer
    # the hyper-parameters are state: another command line is refused naming the field; another rule by the fingerprint
    sd = a.state_dict(0)
    other = train_harness.trainer(["--optimizer", "sgd", "--weight_decay", "0.02"], seed=4)
    with pytest.raises(SystemExit, match=r"optimizers\.frame_predictor\.weight_decay is 0\.01 in the file and 0\.02 in this run"):
        other.load_state_dict(sd)
    with pytest.raises(SystemExit, match=r"optimizers\.frame_predictor\.lr is 0\.002 in the file and 0\.004 in this run"):
        train_harness.trainer(flags + ["--lr", "0.004"], seed=4).load_state_dict(sd)
    with pytest.raises(SystemExit, match="optimizer is 'sgd' in the file and 'adam' in this run"):
        train_harness.trainer(seed=4).load_state_dict(sd)


# ---- 8. end to end -----------------------------------------------------------------------------------------------------------------
def test_train_py_runs_rmsprop_and_saves_the_torch_layout(tmp_path):
    out = str(tmp_path)
    r = train_harness.run_train_py(train_harness.ARGS + ["--optimizer", "rmsprop", "--weight_decay", "1e-4", "--niter", "1",
                                                         "--epoch_size", "2", "--no_images", "--output_path", out])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "capture failed" not in r.stderr
    lines = [ln for ln in r.stdout.splitlines() if "optimizer:" in ln]
    assert len(lines) == 1 and "rmsprop alpha 0.99 momentum 0" in lines[0] and "weight decay 0.0001 on " in lines[0], r.stdout[-1500:]
    ck = torch.load(os.path.join(out, "model.pth"), map_location="cpu", weights_only=False)
    sd = ck["gp_layer_optimizer"]
    n = sum(len(g["params"]) for g in sd["param_groups"])
    assert len(sd["param_groups"]) == 2 and n > 0 and set(sd["state"]) == set(range(n))
    for st in sd["state"].values():
        assert set(st) == {"step", "square_avg"} and float(st["step"]) == 4.0          # two step sites an iteration
    o = torch.optim.RMSprop([{"params": [torch.nn.Parameter(torch.zeros_like(sd["state"][k]["square_avg"])) for k in g["params"]]}
                             for g in sd["param_groups"]], lr=0.002)
    o.load_state_dict(sd)
    assert o.param_groups[0]["alpha"] == 0.99 and o.param_groups[0]["weight_decay"] == 0.0      # the GP layer does not decay
    assert np.isfinite(float(o.state[o.param_groups[0]["params"][0]]["square_avg"].sum()))
