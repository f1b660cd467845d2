"""CPU: the host side of the learning-rate schedule (train.py --lr_schedule) - the oracle's fixed points, the options and the rule
that builds a schedule, the resume fingerprint untouched by the flags, the two entry points in the header, the binding table and
the built library, their argument checks, and the round trip of the spec and the count through a plain training state."""
import argparse
import ctypes
import math
import os

import pytest

from tests import lr_schedule_ref as ref
from tests.common import header_declaration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECAYING = ("linear", "cosine")


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.KINDS)
def test_warmup_fixed_points(kind):
    W, N = 5, 40
    assert ref.s(kind, 0, W, N, 0.1, 4, 0.5) == 1.0 / W
    assert ref.s(kind, W - 1, W, N, 0.1, 4, 0.5) == 1.0
    assert ref.s(kind, W, W, N, 0.1, 4, 0.5) == 1.0                       # u = 0: every kind starts its decay at 1
    assert [ref.s(kind, k, W, N, 0.1, 4, 0.5) for k in range(W)] == [(k + 1.0) / W for k in range(W)]
    assert ref.s(kind, 0, 1, N) == 1.0 and ref.s(kind, 0, 0, N) == 1.0    # W = 1 and W = 0: no iteration runs below the base rate


@pytest.mark.parametrize("kind", DECAYING)
@pytest.mark.parametrize("R", [0.0, 0.1, 0.25, 1.0])
def test_decay_ends_at_the_floor_and_never_rises(kind, R):
    W, N = 3, 50
    for k in (N, N + 1, 10 * N, ref.INT_MAX):
        assert ref.s(kind, k, W, N, R) == R, (k, R)
    tail = [ref.s(kind, k, W, N, R) for k in range(W, N + 3)]
    assert all(a >= b for a, b in zip(tail, tail[1:])), kind
    assert all(R <= v <= 1.0 for v in tail)
    assert kind != "linear" or ref.s(kind, 27, 3, 51, 0.0) == 0.5                        # halfway: (k - W) / (N - W) = 24 / 48
    assert kind != "cosine" or abs(ref.s(kind, 27, 3, 51, 0.0) - 0.5) < 1e-16            # cos(pi / 2) = 6e-17 in fp64


def test_step_drops_by_gamma_exactly_at_its_multiples_and_stops_at_the_floor():
    W, N, K, G, R = 3, 1000, 4, 0.5, 0.1
    for j in range(0, 3):                          # 1, 1/2, 1/4, then 1/8, then the floor: 1/16 < R
        lo, hi = W + j * K, W + (j + 1) * K
        assert {ref.s("step", k, W, N, R, K, G) for k in range(lo, hi)} == {G ** j}
        assert ref.s("step", hi, W, N, R, K, G) == max(R, G * ref.s("step", hi - 1, W, N, R, K, G))
    assert ref.s("step", W + 3 * K, W, N, R, K, G) == 0.125 and ref.s("step", W + 4 * K, W, N, R, K, G) == R
    assert all(ref.s("step", k, W, N, R, K, G) >= R for k in range(0, 200))
    assert ref.s("step", ref.INT_MAX, W, N, R, K, G) == R and ref.s("step", ref.INT_MAX, W, N, 0.0, K, G) == 0.0
    assert ref.s("step", 10 ** 6, 0, 1, 0.0, 1, 1.0) == 1.0                              # G = 1: a constant


@pytest.mark.parametrize("kind", ref.KINDS)
def test_degenerate_spans_give_finite_values(kind):
    for W, N in ((0, 1), (0, 7), (6, 7), (1, 2)):  # no warm-up; N - W = 1: the decay is one iteration long
        vals = [ref.s(kind, k, W, N, 0.25, 1, 0.5) for k in range(0, N + 3)]
        assert all(math.isfinite(v) and 0.0 < v <= 1.0 for v in vals), (W, N, vals)
        assert ref.s(kind, W, W, N, 0.25, 1, 0.5) == 1.0
        if kind in DECAYING and N - W == 1:
            assert ref.s(kind, W + 1, W, N, 0.25) == 0.25
    assert ref.s32("linear", 5, 3, 12, 0.1).dtype.name == "float32" and ref.ulps32(1.0, 1.0 + 2.0 ** -23) == 1


def test_the_package_restates_the_oracle():
    """dvg_amd.lr_schedule.multiplier (the initial scale, the restored scale) is the oracle, bit for bit."""
    from dvg_amd import lr_schedule as L
    for kind in ref.KINDS:
        step = kind == "step"
        spec = L.check_spec({"kind": kind, "warmup": 3, "total": 12, "min_ratio": 0.1, "step_every": 4 if step else 1,
                             "gamma": 0.7 if step else 1.0, "lr": 0.002})
        for k in list(range(0, 20)) + [ref.INT_MAX]:
            assert L.multiplier(spec, k) == ref.s(kind, k, 3, 12, 0.1, 4 if step else 1, 0.7 if step else 1.0), (kind, k)
    assert L.KINDS == ref.KINDS


# ---- options -------------------------------------------------------------------------------------------------------------------
def _parse(argv):
    import train
    return train.build_parser().parse_args(list(argv))


def test_without_the_flag_nothing_is_built():
    from dvg_amd import lr_schedule as L
    o = _parse([])
    assert o.lr_schedule is None and L.schedule_options(o) is None and L.make_schedule(o, "cpu") is None
    assert L.schedule_options(argparse.Namespace()) is None and L.make_schedule(argparse.Namespace(), None) is None
    assert L.base_rate(o) == L.base_rate(argparse.Namespace()) == 0.002
    assert L.base_rate(_parse(["--lr", "0.01"])) == 0.002                  # --lr stays unused without a schedule


def test_defaults_and_the_base_rate_under_the_flag():
    from dvg_amd import lr_schedule as L
    o = _parse(["--lr_schedule", "cosine", "--niter", "7", "--epoch_size", "11", "--lr", "0.01"])
    assert L.schedule_options(o) == {"kind": "cosine", "warmup": 0, "total": 77, "min_ratio": 0.0, "step_every": 1, "gamma": 1.0,
                                     "lr": 0.01}
    assert L.base_rate(o) == 0.01
    o = _parse(["--lr_schedule", "step", "--epoch_size", "11", "--lr_warmup", "5", "--lr_total", "99", "--lr_min_ratio", "0.25"])
    assert L.schedule_options(o) == {"kind": "step", "warmup": 5, "total": 99, "min_ratio": 0.25, "step_every": 11, "gamma": 0.5,
                                     "lr": 0.002}
    o = _parse(["--lr_schedule", "step", "--lr_step_every", "3", "--lr_gamma", "0.9"])
    assert (L.schedule_options(o)["step_every"], L.schedule_options(o)["gamma"]) == (3, 0.9)
    import train
    assert "base rate" in train.build_parser().format_help()               # --lr's help says what it becomes


@pytest.mark.parametrize("argv,option", [
    (["--lr_schedule", "linear", "--lr_warmup", "-1"], "--lr_warmup"),
    (["--lr_schedule", "linear", "--lr_total", "0"], "--lr_total"),
    (["--lr_schedule", "linear", "--lr_warmup", "5", "--lr_total", "5"], "--lr_total"),
    (["--lr_schedule", "linear", "--lr_total", str(2 ** 31)], "--lr_total"),
    (["--lr_schedule", "cosine", "--lr_min_ratio", "-0.1"], "--lr_min_ratio"),
    (["--lr_schedule", "cosine", "--lr_min_ratio", "1.5"], "--lr_min_ratio"),
    (["--lr_schedule", "cosine", "--lr_min_ratio", "nan"], "--lr_min_ratio"),
    (["--lr_schedule", "step", "--lr_step_every", "0"], "--lr_step_every"),
    (["--lr_schedule", "step", "--lr_gamma", "0"], "--lr_gamma"),
    (["--lr_schedule", "step", "--lr_gamma", "1.5"], "--lr_gamma"),
    (["--lr_schedule", "step", "--lr_gamma", "nan"], "--lr_gamma"),
    (["--lr_schedule", "constant", "--lr", "-1"], "--lr"),
    (["--lr_schedule", "constant", "--lr", "inf"], "--lr"),
    (["--lr_schedule", "constant", "--lr", "nan"], "--lr"),
    (["--lr_schedule", "cosine", "--lr_gamma", "0.5"], "--lr_gamma"),      # a companion of another kind
    (["--lr_schedule", "linear", "--lr_step_every", "3"], "--lr_step_every"),
    (["--lr_warmup", "3"], "--lr_warmup"),                                 # companions without the flag they belong to
    (["--lr_total", "3"], "--lr_total"),
    (["--lr_min_ratio", "0.5"], "--lr_min_ratio"),
    (["--lr_step_every", "3"], "--lr_step_every"),
    (["--lr_gamma", "0.5"], "--lr_gamma"),
])
def test_every_invalid_value_names_its_option(argv, option):
    from dvg_amd import lr_schedule as L
    with pytest.raises(SystemExit) as exc:
        L.schedule_options(_parse(argv))
    msg = str(exc.value)
    assert option in msg and "\n" not in msg, msg
    with pytest.raises(SystemExit):
        L.make_schedule(_parse(argv), "cpu")


def test_an_unknown_kind_is_refused_by_the_parser(capsys):
    with pytest.raises(SystemExit):
        _parse(["--lr_schedule", "exponential"])
    assert "--lr_schedule" in capsys.readouterr().err


def test_the_flags_are_not_part_of_the_resume_fingerprint():
    """option_fingerprint(opt) is the parent's for the same options: the fields are the fourteen of before and `world`."""
    from dvg_amd import train_state
    assert train_state.FORMAT == 1 and train_state.OPTION_FIELDS == (
        "model", "image_width", "channels", "g_dim", "rnn_size", "predictor_rnn_layers", "batch_size", "n_past", "n_future",
        "n_eval", "dataset", "num_digits", "last_frame_skip", "ft")
    plain = _parse([])
    sched = _parse(["--lr_schedule", "cosine", "--lr_warmup", "10", "--lr", "0.01"])
    for o in (plain, sched):
        o.ft, o.world = True, 1
    fp = train_state.option_fingerprint(plain)
    assert fp == train_state.option_fingerprint(sched) and sorted(fp) == sorted(train_state.OPTION_FIELDS + ("world",))
    assert fp == {**{k: getattr(plain, k) for k in train_state.OPTION_FIELDS}, "world": 1}
    train_state.check_fingerprint(fp, train_state.option_fingerprint(sched), "<state>")          # no SystemExit


# ---- the entry points --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dvg_lr_schedule_tick", "dvg_adam_step_scheduled"])
def test_header_binding_table_and_library_agree(name):
    """Declared, returning int, exported by both builds, within ABI 9 (tests/test_abi.py holds the binding of every declaration
    to the header, argument by argument)."""
    from dvg_amd import _lib
    ret, params = header_declaration(name)
    assert ret == "int" and _lib.SIGNATURES[name][0] is ctypes.c_int and len(_lib.SIGNATURES[name][1]) == len(params)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} is not exported by the built library"
    native = os.path.join(os.path.dirname(_lib.LIB_PATH), "libdvg_hip_f32mfma.so")
    assert hasattr(ctypes.CDLL(native), name)
    assert _lib.lib().dvg_abi_version() == 9                               # additions within ABI 9


def test_the_scheduled_step_takes_the_guarded_arguments_and_one_more():
    from dvg_amd import _lib
    guarded, scheduled = _lib.SIGNATURES["dvg_adam_step_guarded"][1], _lib.SIGNATURES["dvg_adam_step_scheduled"][1]
    assert list(scheduled) == list(guarded[:-1]) + [ctypes.c_void_p, guarded[-1]]       # ..., lr_scale_dev, stream
    assert "lr_schedule.hip" in open(os.path.join(ROOT, "dvg_amd", "csrc", "Makefile")).read().split("SRCS")[1].split("\n")[0]


SHAPE, NULL, ALIGN = 1, 2, 4


def test_tick_checks_fire_before_any_launch():
    from dvg_amd import _lib
    lib = _lib.lib()
    ok, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)          # never dereferenced: every call fails a check
    tick = lib.dvg_lr_schedule_tick
    assert tick(1, 3, 12, 4, 0.1, 0.5, None, ok, None) == NULL and tick(1, 3, 12, 4, 0.1, 0.5, ok, None, None) == NULL
    assert b"dvg_lr_schedule_tick" in lib.dvg_last_error()
    for kind in (-1, 4, 99):
        assert tick(kind, 3, 12, 4, 0.1, 0.5, ok, ok, None) == SHAPE, kind
    assert b"kind" in lib.dvg_last_error()
    for W, N in ((-1, 12), (3, 3), (3, 2), (0, 0), (0, -5)):
        assert tick(2, W, N, 4, 0.1, 0.5, ok, ok, None) == SHAPE, (W, N)
    for R in (-0.1, 1.5, float("nan"), float("inf")):
        assert tick(2, 3, 12, 4, R, 0.5, ok, ok, None) == SHAPE, R
    assert b"R =" in lib.dvg_last_error()
    for K, G in ((0, 0.5), (-3, 0.5), (4, 0.0), (4, -0.5), (4, 1.5), (4, float("nan"))):
        assert tick(3, 3, 12, K, 0.1, G, ok, ok, None) == SHAPE, (K, G)
        for kind in (0, 1, 2):                                  # K and G belong to `step` alone: the others pass on to ...
            assert tick(kind, 3, 12, K, 0.1, G, odd, ok, None) == ALIGN, (kind, K, G)      # ... the next check
    assert tick(3, 3, 12, 4, 0.1, 0.5, odd, ok, None) == ALIGN and tick(3, 3, 12, 4, 0.1, 0.5, ok, odd, None) == ALIGN


def test_scheduled_step_checks_fire_before_any_launch():
    from dvg_amd import _lib
    lib = _lib.lib()
    ok, odd4, odd = ctypes.c_void_p(64), ctypes.c_void_p(68), ctypes.c_void_p(66)
    step = lib.dvg_adam_step_scheduled
    hyper = (2e-3, 0.9, 0.999, 1e-8, 0.0)

    def call(p=ok, g=ok, m=ok, v=ok, n=8, t=1, tdev=None, stat=None, skips=None, scale=ok):
        return step(p, g, m, v, n, *hyper, t, tdev, stat, skips, scale, None)
    for k in ("p", "g", "m", "v", "scale"):
        assert call(**{k: None}) == NULL, k
    assert b"dvg_adam_step_scheduled" in lib.dvg_last_error()
    assert call(stat=ok) == NULL and call(skips=ok) == NULL     # the guard's two pointers go together
    assert b"together" in lib.dvg_last_error()
    assert call(n=0) == SHAPE and call(n=-4) == SHAPE and call(t=0) == SHAPE
    for k in ("p", "g", "m", "v"):
        assert call(**{k: odd4}) == ALIGN, k
    assert call(scale=odd) == ALIGN and call(tdev=odd, t=0) == ALIGN
    assert call(stat=odd, skips=ok) == ALIGN and call(stat=ok, skips=odd) == ALIGN


# ---- the training state ------------------------------------------------------------------------------------------------------------
def _schedule(argv):
    from dvg_amd import lr_schedule as L
    return L.make_schedule(_parse(argv), "cpu")                 # the two buffers on the host: no launch in these tests


COSINE = ["--lr_schedule", "cosine", "--lr_warmup", "2", "--lr_total", "6", "--lr_min_ratio", "0.1"]


def test_state_round_trip_through_plain_dicts(capsys):
    from dvg_amd import lr_schedule as L
    a = _schedule(COSINE)
    assert float(a.scale) == float(ref.s32("cosine", 0, 2, 6, 0.1)) == 0.5 and int(a.iters) == 0
    a.load_state(4)
    st = a.state()
    assert st == {"spec": {"kind": "cosine", "warmup": 2, "total": 6, "min_ratio": 0.1, "step_every": 1, "gamma": 1.0, "lr": 0.002},
                  "iters": 4}
    assert all(type(v) in (str, int, float) for v in st["spec"].values())
    b = _schedule(COSINE)
    iters_ptr, scale_ptr = b.iters.data_ptr(), b.scale.data_ptr()
    L.restore(b, {"lr_schedule": st}, "<state>", global_step=99)
    assert int(b.iters) == 4 and float(b.scale) == float(ref.s32("cosine", 4, 2, 6, 0.1))
    assert (b.iters.data_ptr(), b.scale.data_ptr()) == (iters_ptr, scale_ptr)      # through the existing buffers
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("argv,field", [
    (["--lr_schedule", "linear", "--lr_warmup", "2", "--lr_total", "6", "--lr_min_ratio", "0.1"], "kind"),
    (["--lr_schedule", "cosine", "--lr_warmup", "3", "--lr_total", "6", "--lr_min_ratio", "0.1"], "warmup"),
    (["--lr_schedule", "cosine", "--lr_warmup", "2", "--lr_total", "7", "--lr_min_ratio", "0.1"], "total"),
    (["--lr_schedule", "cosine", "--lr_warmup", "2", "--lr_total", "6", "--lr_min_ratio", "0.2"], "min_ratio"),
    (COSINE + ["--lr", "0.001"], "lr"),
])
def test_a_spec_mismatch_is_refused_naming_the_field(argv, field):
    from dvg_amd import lr_schedule as L
    saved = _schedule(COSINE).state()
    with pytest.raises(SystemExit) as exc:
        L.restore(_schedule(argv), {"lr_schedule": saved}, "<state>", global_step=0)
    assert f"lr_schedule.{field} " in str(exc.value) and "<state>" in str(exc.value)
    step = ["--lr_schedule", "step", "--lr_total", "60", "--lr_step_every", "4", "--lr_gamma", "0.5"]
    for other, f in ((step[:-1] + ["0.25"], "gamma"), (step[:-3] + ["5", "--lr_gamma", "0.5"], "step_every")):
        with pytest.raises(SystemExit, match=f"lr_schedule.{f} "):
            L.restore(_schedule(other), {"lr_schedule": _schedule(step).state()}, "<state>", global_step=0)


def test_an_old_state_counts_from_its_global_step_and_a_new_one_is_ignored_without_the_flag(capsys):
    from dvg_amd import lr_schedule as L
    b = _schedule(COSINE)
    L.restore(b, {"global_step": 3}, "<state>", global_step=3, restored_lr=0.002)
    out = capsys.readouterr().out
    assert int(b.iters) == 3 and float(b.scale) == float(ref.s32("cosine", 3, 2, 6, 0.1))
    assert out.count("\n") == 1 and "--lr_schedule" in out and "global step 3" in out
    L.restore(_schedule(COSINE), {}, "<state>", global_step=3, rank=1)
    assert capsys.readouterr().out == ""                                   # rank 0 prints
    with pytest.raises(SystemExit, match="lr_schedule.lr "):               # the optimisers' restored rate is not this run's --lr
        L.restore(_schedule(COSINE + ["--lr", "0.01"]), {}, "<state>", global_step=3, restored_lr=0.002)
    L.restore(None, {"lr_schedule": b.state()}, "<state>", global_step=3)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "ignored" in out and "--lr_schedule" in out
    L.restore(None, {}, "<state>", global_step=3)
    assert capsys.readouterr().out == ""                                   # nothing saved, nothing asked: nothing said
