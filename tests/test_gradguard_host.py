"""CPU: the host side of the gradient guard (train.py --clip_grad_norm / --skip_nonfinite) - flag defaults and the rule that
builds a guard, the partial-sum count as a function of n alone, the argument checks of the three entry points, the resume
fingerprint untouched by the flags, and the fp64 restatement the GPU tests compare against on hand-computed numbers."""
import argparse
import ctypes
import math

import numpy as np
import pytest

from tests import gradguard_ref as ref


def test_parser_defaults_and_the_rule_that_builds_a_guard():
    import train
    p = train.build_parser()
    o = p.parse_args([])
    assert o.clip_grad_norm == 0.0 and o.skip_nonfinite is False
    assert train.guard_options(o) is None
    assert train.guard_options(argparse.Namespace()) is None              # an options object from before the flags
    assert train.guard_options(p.parse_args(["--clip_grad_norm", "0.5"])) == (0.5, False)
    assert train.guard_options(p.parse_args(["--skip_nonfinite"])) == (0.0, True)
    assert train.guard_options(p.parse_args(["--clip_grad_norm", "2", "--skip_nonfinite"])) == (2.0, True)
    for bad in ("-1", "nan"):
        with pytest.raises(SystemExit, match="clip_grad_norm"):
            train.guard_options(p.parse_args(["--clip_grad_norm", bad]))
    assert callable(train.Trainer._step)


def test_partial_sum_count_is_a_function_of_n_alone():
    from dvg_amd import _lib, ops
    lib = _lib.lib()
    chunk = ref.CHUNK
    cases = {4: 1, chunk - 4: 1, chunk: 1, chunk + 4: 2, 3 * chunk + 8: 4, 2 ** 25: 2048, 0: 0, -4: 0}
    for n, want in cases.items():
        assert lib.dvg_grad_sumsq_blocks(n) == want == ref.blocks(n), n
    assert ops.grad_sumsq_blocks(21_100_000) == 1288                       # 21.1 M floats, about vgg_64's arena


def test_argument_checks_fire_before_any_launch():
    from dvg_amd import _lib
    lib = _lib.lib()
    ok, odd = ctypes.c_void_p(64), ctypes.c_void_p(68)       # never dereferenced: every call fails in the checks
    OK, SHAPE, NULL, ALIGN = 0, 1, 2, 4
    assert lib.dvg_grad_sumsq(None, 8, ok, None) == NULL and lib.dvg_grad_sumsq(ok, 8, None, None) == NULL
    for n in (0, -4, 6, 16385):
        assert lib.dvg_grad_sumsq(ok, n, ok, None) == SHAPE, n
    assert b"dvg_grad_sumsq" in lib.dvg_last_error()
    assert lib.dvg_grad_sumsq(odd, 8, ok, None) == ALIGN and lib.dvg_grad_sumsq(ok, 8, odd, None) == ALIGN
    assert lib.dvg_grad_guard_finish(None, 1, 1.0, 0, ok, ok, None) == NULL
    assert lib.dvg_grad_guard_finish(ok, 1, 1.0, 0, None, ok, None) == NULL
    assert lib.dvg_grad_guard_finish(ok, 1, 1.0, 0, ok, None, None) == NULL
    assert lib.dvg_grad_guard_finish(ok, 0, 1.0, 0, ok, ok, None) == SHAPE
    assert lib.dvg_grad_guard_finish(ok, 1, float("nan"), 0, ok, ok, None) == SHAPE
    assert lib.dvg_grad_guard_finish(odd, 1, 1.0, 0, ok, ok, None) == ALIGN
    adam = lambda *a: lib.dvg_adam_step_guarded(*a[:4], a[4], 2e-3, 0.9, 0.999, 1e-8, 0.0, a[5], a[6], a[7], a[8], None)  # noqa: E731
    assert adam(ok, ok, ok, ok, 8, 1, None, None, ok) == NULL             # no stat
    assert adam(ok, ok, ok, ok, 8, 1, None, ok, None) == NULL             # no skip counter
    assert adam(None, ok, ok, ok, 8, 1, None, ok, ok) == NULL
    assert adam(ok, ok, ok, ok, 0, 1, None, ok, ok) == SHAPE
    assert adam(ok, ok, ok, ok, 8, 0, None, ok, ok) == SHAPE              # neither a host step count nor a device one
    assert adam(ok, odd, ok, ok, 8, 1, None, ok, ok) == ALIGN
    assert adam(ok, ok, ok, ok, 8, 1, None, ctypes.c_void_p(66), ok) == ALIGN     # stat, skips_dev, step_dev: 4-byte aligned
    assert adam(ok, ok, ok, ok, 8, 1, None, ok, ctypes.c_void_p(66)) == ALIGN
    assert adam(ok, ok, ok, ok, 8, 1, ctypes.c_void_p(66), ok, ok) == ALIGN
    assert b"dvg_adam_step_guarded" in lib.dvg_last_error()
    assert OK == 0


def test_the_flags_are_not_part_of_the_resume_fingerprint():
    import train
    from dvg_amd import train_state
    assert train_state.OPTION_FIELDS == ("model", "image_width", "channels", "g_dim", "rnn_size", "predictor_rnn_layers",
                                         "batch_size", "n_past", "n_future", "n_eval", "dataset", "num_digits", "last_frame_skip",
                                         "ft")
    p = train.build_parser()
    plain, guarded = p.parse_args([]), p.parse_args(["--clip_grad_norm", "0.5", "--skip_nonfinite"])
    for o in (plain, guarded):
        o.ft, o.world = True, 1
    saved = train_state.option_fingerprint(plain)              # what a state written without the flags carries
    assert "clip_grad_norm" not in saved and "skip_nonfinite" not in saved
    train_state.check_fingerprint(saved, train_state.option_fingerprint(guarded), "<state>")     # no SystemExit
    guarded.n_past = 3
    with pytest.raises(SystemExit, match="n_past"):
        train_state.check_fingerprint(saved, train_state.option_fingerprint(guarded), "<state>")


def test_reference_on_hand_computed_cases():
    assert ref.verdict([3.0, 4.0, 0.0, 0.0], 0.0, True) == (5.0, 1.0, False)
    n, s, skip = ref.verdict([3.0, 4.0, 0.0, 0.0], 2.5, False)
    assert n == 5.0 and s == 2.5 / (5.0 + 1e-6) and not skip
    assert ref.verdict([3.0, 4.0, 0.0, 0.0], 10.0, False)[1] == 1.0
    big = np.full(4, 1e25, dtype=np.float32)                   # squares overflow fp32, not fp64
    n, s, skip = ref.verdict(big, 1.0, True)
    assert math.isfinite(n) and abs(n / 2e25 - 1) < 1e-7 and 0 < s < 1 and not skip
    n, s, skip = ref.verdict([1.0, float("inf"), 0.0, 0.0], 1.0, True)
    assert n == math.inf and s == 0.0 and skip
    n, s, skip = ref.verdict([1.0, float("-inf"), float("nan"), 0.0], 1.0, False)
    assert math.isnan(n) and math.isnan(s) and not skip
    assert ref.verdict([float("nan")] * 4, 0.0, True)[1:] == (1.0, True)
    # one Adam step from zero moments moves every entry by lr against the sign of its gradient, whatever the clip factor
    p, trace = ref.adam_sequence([np.array([1.0, -1.0])], [[np.array([30.0, -40.0], dtype=np.float32)]], 5.0, [[0.1]])
    assert trace == [(50.0, 5.0 / (50.0 + 1e-6))]
    assert np.allclose(p[0], [0.9, -0.9], rtol=0, atol=1e-8)
