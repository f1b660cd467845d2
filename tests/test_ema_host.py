"""CPU: the host side of the weight average (train.py --ema_decay) - the flag's default and the rule that builds an average, the
count of partial-sum pairs as a function of n alone, the argument checks of dvg_ema_update, the resume fingerprint untouched by the
flag, and the fp64 restatement the GPU tests compare against on hand-computed numbers."""
import argparse
import ctypes

import numpy as np
import pytest

from tests import ema_ref as ref


def test_parser_default_and_the_rule_that_builds_an_average():
    import train
    from dvg_amd import ema
    p = train.build_parser()
    assert p.parse_args([]).ema_decay is None
    assert ema.ema_options(p.parse_args([])) is None
    assert ema.ema_options(argparse.Namespace()) is None                  # an options object from before the flag
    assert ema.make_average(argparse.Namespace(), None) is None           # nothing is built, the arena is not even looked at
    assert ema.ema_options(p.parse_args(["--ema_decay", "0.999"])) == 0.999
    assert ema.ema_options(p.parse_args(["--ema_decay", "0"])) == 0.0
    for bad in ("-0.1", "1", "1.5", "nan"):
        with pytest.raises(SystemExit) as exc:
            ema.ema_options(p.parse_args(["--ema_decay", bad]))
        msg = str(exc.value)
        assert "--ema_decay" in msg and "\n" not in msg, (bad, msg)
    import generate_frames
    assert generate_frames.build_parser().parse_args([]).ema is False


def test_pair_count_is_a_function_of_n_alone():
    from dvg_amd import _lib, ops
    lib = _lib.lib()
    chunk = ref.CHUNK
    cases = {chunk - 4: 1, chunk: 1, chunk + 4: 2, 3 * chunk + 8: 4, 0: 0, -4: 0}
    for n, want in cases.items():
        assert lib.dvg_ema_update_blocks(n) == want == ref.blocks(n), n
    assert ops.ema_update_blocks(4) == 1 and ops.ema_update_blocks(21_137_924) == ref.blocks(21_137_924) == 2581


def test_argument_checks_fire_before_any_launch():
    from dvg_amd import _lib
    lib = _lib.lib()
    ok, ok2, odd = ctypes.c_void_p(64), ctypes.c_void_p(128), ctypes.c_void_p(68)   # never dereferenced: every call fails a check
    SHAPE, NULL, ALIGN = 1, 2, 4
    up = lib.dvg_ema_update
    assert up(None, ok2, 8, 0.9, ok, ok, None) == NULL and up(ok, None, 8, 0.9, ok, ok, None) == NULL
    assert up(ok, ok2, 8, 0.9, None, ok, None) == NULL and up(ok, ok2, 8, 0.9, ok, None, None) == NULL
    for n in (0, -4, 6, 8193, 2 ** 45):                        # not positive, no multiple of 4, a block count that does not fit
        assert up(ok, ok2, n, 0.9, ok, ok, None) == SHAPE, n
    assert b"dvg_ema_update" in lib.dvg_last_error()
    for decay in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert up(ok, ok2, 8, decay, ok, ok, None) == SHAPE, decay
    assert b"decay" in lib.dvg_last_error()
    assert up(odd, ok2, 8, 0.9, ok, ok, None) == ALIGN and up(ok, odd, 8, 0.9, ok, ok, None) == ALIGN
    assert up(ctypes.c_void_p(72), ok2, 8, 0.9, ok, ok, None) == ALIGN           # 8-byte aligned is not enough for ema / param
    assert up(ok, ok2, 8, 0.9, ok, odd, None) == ALIGN                             # partials: 8 bytes
    assert up(ok, ok2, 8, 0.9, ctypes.c_void_p(66), ok, None) == ALIGN             # updates_dev: 4 bytes
    assert up(ok, ok, 8, 0.9, ok, ok, None) == SHAPE and b"same buffer" in lib.dvg_last_error()


def test_the_flag_is_not_part_of_the_resume_fingerprint():
    import train
    from dvg_amd import train_state
    assert "ema_decay" not in train_state.OPTION_FIELDS and train_state.FORMAT == 1
    p = train.build_parser()
    plain, averaged = p.parse_args([]), p.parse_args(["--ema_decay", "0.999"])
    for o in (plain, averaged):
        o.ft, o.world = True, 1
    saved = train_state.option_fingerprint(plain)              # what a state written without the flag carries
    assert "ema_decay" not in saved
    train_state.check_fingerprint(saved, train_state.option_fingerprint(averaged), "<state>")     # no SystemExit
    train_state.check_fingerprint(train_state.option_fingerprint(averaged), saved, "<state>")     # nor the other way round
    averaged.n_past = 3
    with pytest.raises(SystemExit, match="n_past"):
        train_state.check_fingerprint(saved, train_state.option_fingerprint(averaged), "<state>")


def test_schedule_on_hand_numbers():
    from dvg_amd import ema
    assert ref.decay_at(0.999, 0) == 0.1 and ref.decay_at(0.999, 1) == 2.0 / 11.0
    assert ref.decay_at(0.05, 0) == 0.05                       # a decay below the warm-up applies from the first update
    for decay, by_hand in ((0.5, 8), (0.9, 80), (0.999, None), (0.9999, None)):       # 9 / 18 = 0.5, 81 / 90 = 0.9
        first = next(k for k in range(10 ** 6) if (1.0 + k) / (10.0 + k) >= decay)
        assert by_hand is None or first == by_hand, decay
        assert all(ref.decay_at(decay, k) == (1.0 + k) / (10.0 + k) < decay for k in range(first))
        assert all(ref.decay_at(decay, k) == decay for k in (first, first + 1, first + 1000))
        assert all(ema.effective_decay(decay, k) == ref.decay_at(decay, k) for k in (0, 1, first - 1, first, first + 7))


def test_constant_parameter_closed_form():
    """p = c, e_0 = 0: e_K = c (1 - prod d_k).  The fp64 chain of ema_ref.update (its weight rounded to fp32, as the kernel holds
    it) agrees to K fp32 roundings of the weight; by hand K = 2: 1 - 0.1 * 2 / 11."""
    assert abs(ref.closed_form(1.0, 0.999, 2) - (1 - 0.1 * 2 / 11)) < 1e-15
    assert ref.closed_form(3.0, 0.0, 5) == 3.0
    c = 0.75
    for decay, K in ((0.999, 12), (0.9, 200), (0.5, 7)):
        e = np.zeros(4)
        for k in range(K):
            e = ref.update(e, np.full(4, c, dtype=np.float32), decay, k)
        want = ref.closed_form(c, decay, K)
        assert np.all(np.abs(e - want) <= K * 2.0 ** -24 * c), (decay, K, e[0], want)
    a, b = ref.sums(np.array([3.0, 0.0], dtype=np.float32), np.array([0.0, 4.0], dtype=np.float32))
    assert (a, b) == (25.0, 9.0) and ref.lag([3.0, 0.0], [0.0, 4.0]) == 5.0 / 3.0
