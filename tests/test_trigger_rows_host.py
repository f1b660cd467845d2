"""CPU: the sampler's per-row variance trigger without a GPU - rollout.trigger_rows_host against the literal reference arithmetic
(tests/trigger_rows_ref.py), the rule's closed forms, the conditions on the seeded cases that tests/test_gpu_trigger_rows.py
relies on, generate_frames.py's flags, and dvg_gp_trigger_rows' host-side refusals."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import trigger_rows_ref as ref


def _cases():
    for c in ref.CASES:
        for n_past in ref.n_pasts(c):
            for coef in ref.COEFS:
                for gap in ref.GAPS:
                    yield c, n_past, coef, gap


@pytest.mark.parametrize("c", ref.CASES)
def test_host_rule_is_the_reference_arithmetic_bit_for_bit(c):
    from dvg_amd import rollout
    D, B, W, T = c
    _, values = ref.case(D, B, W, T, ref.SEEDS[c])
    assert values.dtype == np.float32 and values.shape == (T, B)
    for n_past in ref.n_pasts(c):
        for coef in ref.COEFS:
            for gap in ref.GAPS:
                flags, thr = rollout.trigger_rows_host(values, n_past, W, coef, gap)
                f_ref, t_ref, _, _ = ref.decide(values, n_past, W, coef, gap)
                assert flags.dtype == np.int32 and thr.dtype == np.float32
                assert np.array_equal(flags, f_ref), (c, n_past, coef, gap)
                assert np.array_equal(thr.view(np.uint32), t_ref.view(np.uint32)), (c, n_past, coef, gap)
                first = max(n_past, W + 1)
                assert not flags[:first].any() and np.isinf(thr[:first]).all() and np.isfinite(thr[first:]).all()


def test_gap_rule_suppresses_and_still_logs_the_threshold():
    from dvg_amd import rollout
    c = ref.CASES[3]
    _, values = ref.case(*c, ref.SEEDS[c])
    f0, t0 = rollout.trigger_rows_host(values, 2, c[2], -0.5, 0)
    f3, t3 = rollout.trigger_rows_host(values, 2, c[2], -0.5, 3)
    assert np.array_equal(t0.view(np.uint32), t3.view(np.uint32))          # the windows do not depend on the decisions
    assert f3.sum() < f0.sum() and not (f3 & ~f0.astype(bool)).any()       # a subset of the unsuppressed draws
    for b in range(c[1]):
        steps = np.nonzero(f3[:, b])[0]
        assert (np.diff(steps) > 3).all(), (b, steps)
        if len(np.nonzero(f0[:, b])[0]):
            assert steps[0] == np.nonzero(f0[:, b])[0][0]                  # the first draw is never suppressed


def test_closed_forms():
    """A window of equal values never draws (std 0: value == threshold); W = 1 is such a window at every step, whatever coef;
    coef >= sqrt(W - 1) never draws - W = 5 with 2.01 - while coef -0.5 on the same values does."""
    from dvg_amd import rollout
    const = np.full((30, 4), 0.37, dtype=np.float32)
    for coef in (2.01, -0.5, 0.0):
        flags, thr = rollout.trigger_rows_host(const, 2, 6, coef, 0)
        assert not flags.any() and np.array_equal(thr[7:], const[7:])
    _, v1 = ref.case(*ref.CASES[2], ref.SEEDS[ref.CASES[2]])
    _, v1b = ref.case(3, 5, 1, 40, 7)
    for coef in (2.01, -0.5):
        assert not rollout.trigger_rows_host(v1, 2, 1, coef, 0)[0].any()
        assert not rollout.trigger_rows_host(v1b, 2, 1, coef, 0)[0].any()
    c = ref.CASES[0]
    _, v5 = ref.case(*c, ref.SEEDS[c])
    assert 2.01 >= math.sqrt(5 - 1)
    assert not rollout.trigger_rows_host(v5, 2, 5, 2.01, 0)[0].any()
    assert rollout.trigger_rows_host(v5, 2, 5, -0.5, 0)[0].any()
    assert not rollout.VarianceTrigger(5, 2.01).can_draw() and not rollout.VarianceTrigger(1, -0.5).can_draw()
    assert rollout.VarianceTrigger(6, 2.01).can_draw() and rollout.VarianceTrigger(12).can_draw()
    for bad in (dict(window=0), dict(window=65), dict(min_gap=-1)):
        with pytest.raises(ValueError):
            rollout.VarianceTrigger(**bad)
    t = rollout.VarianceTrigger()
    assert (t.window, t.coef, t.min_gap) == (12, 2.01, 0) and t.first_decision(5) == 13 and t.first_decision(20) == 20


def test_the_seeded_cases_meet_the_conditions_the_gpu_test_relies_on():
    """tests/test_gpu_trigger_rows.py compares flags where the reference's margin exceeds 1e-4 and counts the decisions inside
    it: none allowed for the first three cases, 1 % for the fourth; every coef -0.5 case takes both branches.  Both are
    conditions on the seeded inputs, so they are asserted here, on the reference alone."""
    for c, n_past, coef, gap in _cases():
        _, values = ref.case(*c, ref.SEEDS[c])
        flags, _, margins, _ = ref.decide(values, n_past, c[2], coef, gap)
        m = margins[np.isfinite(margins)]
        assert len(m) == (c[3] - max(n_past, c[2] + 1)) * c[1]
        near = int((m <= ref.GUARD).sum())
        print(f"case {c} n_past {n_past} coef {coef} gap {gap}: {len(m)} decisions, {int(flags.sum())} draws, smallest margin "
              f"{m.min():.2e}, {near} inside {ref.GUARD:.0e}")
        if c == ref.CASES[2]:
            # W = 1: the window IS the value, so threshold == value exactly and every decision is a tie that `>` settles as "no
            # draw" - on the device too (an fp64 mean of one float is that float, the deviation 0).  The GPU test therefore
            # compares this case's flags without the margin rule, and it is the one coef -0.5 case with a single branch.
            assert (m == 0.0).all() and not flags.any()
            continue
        if c == ref.CASES[3]:
            assert near <= 0.01 * len(m), (c, coef, gap, near)
        else:
            assert near == 0, (c, coef, gap, near, m.min())
        if coef == -0.5:
            assert 0 < flags.sum() < len(m), (c, n_past, gap, flags.sum())


def test_parser(capsys):
    import generate_frames
    a = generate_frames.parse_args([])
    assert (a.trigger, a.trigger_window, a.trigger_coef, a.trigger_min_gap) == ("period", 12, 2.01, 0)
    assert generate_frames.variance_trigger(a) is None
    a = generate_frames.parse_args(["--trigger", "variance", "--trigger_window", "7", "--trigger_coef", "-0.5", "--trigger_min_gap", "2"])
    assert generate_frames.variance_trigger(a).key() == (7, -0.5, 2)
    assert capsys.readouterr().err == ""
    for bad, word in ((["--trigger", "variance", "--gp_trigger"], "--gp_trigger"), (["--trigger_window", "0"], "--trigger_window"),
                      (["--trigger_window", "65"], "--trigger_window"), (["--trigger_min_gap", "-1"], "--trigger_min_gap"),
                      (["--trigger", "sometimes"], "--trigger")):
        with pytest.raises(SystemExit):
            generate_frames.parse_args(bad)
        assert word in capsys.readouterr().err
    generate_frames.parse_args(["--gp_trigger"])                                     # the period rule goes with it, as before
    # coef >= sqrt(W - 1) can never draw: ONE warning, with the variance rule only
    generate_frames.parse_args(["--trigger", "variance", "--trigger_window", "5"])
    err = capsys.readouterr().err
    assert err.count("WARNING") == 1 and "sqrt" in err and "--trigger_coef" in err
    generate_frames.parse_args(["--trigger", "variance", "--trigger_window", "6"])
    generate_frames.parse_args(["--trigger_window", "5"])
    assert capsys.readouterr().err == ""


def test_abi_entry_point_and_its_host_side_refusals():
    """The pattern of tests/test_abi.py::test_host_side_checks_reject_bad_shapes_without_gpu: fake pointers, never dereferenced -
    every call must fail in the checks, before any launch."""
    from dvg_amd import _lib
    assert "dvg_gp_trigger_rows" in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES["dvg_gp_trigger_rows"]
    assert restype is ctypes.c_int and len(argtypes) == 19
    for so in ("libdvg_hip.so", "libdvg_hip_f32mfma.so"):
        assert hasattr(ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), so)), "dvg_gp_trigger_rows")
    lib = _lib.lib()
    assert lib.dvg_abi_version() == 9
    one = ctypes.c_void_p(16)
    SHAPE, NULL = _lib.CONSTANTS["ERR_SHAPE"], _lib.CONSTANTS["ERR_NULL"]

    def call(var=one, sample=one, h_pred=one, vec=one, D=90, B=4, win=one, window=12, pos=12, decide=1, gap=0, last=one, slot=13):
        return lib.dvg_gp_trigger_rows(var, sample, h_pred, vec, D, B, win, window, pos, decide, 2.01, 13, gap, last, one, one,
                                       one, slot, None)
    assert call(window=65, pos=65) == SHAPE and b"window" in lib.dvg_last_error()
    assert call(window=0, pos=0, decide=0) == SHAPE and b"window" in lib.dvg_last_error()
    assert call(pos=3) == SHAPE                                  # decide with pos < window
    assert call(pos=13) == SHAPE and call(pos=-1, decide=0) == SHAPE
    assert call(var=None) == NULL and call(win=None) == NULL and call(last=None) == NULL
    for missing in ("sample", "h_pred", "vec"):
        assert call(**{missing: None}) == NULL                   # a deciding launch needs all three
    assert call(D=0) == SHAPE and call(B=0) == SHAPE and call(gap=-1) == SHAPE and call(slot=-1) == SHAPE
    with pytest.raises(RuntimeError):
        _lib.check(call(slot=-1), "gp_trigger_rows")
