"""CPU: train.py --val_gp / generate_frames.py --gp_report without a GPU - the library exports and binds dvg_gp_score and
dvg_gp_score_slots, and the host-side checks fire before any launch; tests/gp_score_ref.py (the fp64 restatement the GPU tests
compare the kernel with) on hand-made entries and the margins of its input sets; dvg_amd.gp_score.summarise / report on hand-made
accumulators; the flag; a record with a `gp` key through the log."""
import argparse
import ctypes
import json
import math
import os
import statistics

import numpy as np
import pytest
import torch

from tests import gp_score_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


# ---- the library ----------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_binds_gp_score():
    from dvg_amd import _lib, ops
    assert len(_lib.SIGNATURES["dvg_gp_score"][1]) == 12 and len(_lib.SIGNATURES["dvg_gp_score_slots"][1]) == 2
    for name in ("libdvg_hip.so", "libdvg_hip_f32mfma.so"):
        so = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), name))
        assert hasattr(so, "dvg_gp_score") and hasattr(so, "dvg_gp_score_slots"), name
    assert _lib.lib().dvg_abi_version() == 9
    a, c = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib.lib().dvg_gp_score_slots(ctypes.addressof(a), ctypes.addressof(c)) == 0 and (a.value, c.value) == (14, 14)
    assert ops.GP_SCORE_SLOTS == (14, 14) == ops.gp_score_slots() == (ref.ACC, ref.CNT)
    assert "gp_score.hip" in open(os.path.join(ROOT, "dvg_amd", "csrc", "Makefile")).read().split("SRCS")[1].splitlines()[0]
    header = open(os.path.join(ROOT, "include", "dvg_hip.h")).read()
    assert "int dvg_gp_score_slots(int* acc_slots, int* cnt_slots);" in header and "int dvg_gp_score(const float* mean" in header
    for site in ("generate_frames.py:131,170,229", "train.py:283"):        # the reference call sites the entry point serves
        assert site in header.split("dvg_gp_score_slots")[0].rsplit("/*", 1)[1]
    assert "gp_score" in open(os.path.join(ROOT, "dvg_amd", "csrc", "dvg_common.h")).read().split("enum SumOrder")[0]


def test_host_side_checks_refuse_bad_calls_without_a_gpu():
    from dvg_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(16)          # fake, never dereferenced: every call must fail in the checks
    shape, null = _lib.CONSTANTS["ERR_SHAPE"], _lib.CONSTANTS["ERR_NULL"]

    def call(mean=one, var=one, noise=None, period=0, target=one, B=2, R=6, acc=one, cnt=one):
        return lib.dvg_gp_score(mean, var, noise, period, target, 1, R, B, R, acc, cnt, None)
    assert call(B=0) == shape and b"B and R must be >= 1" in lib.dvg_last_error()
    assert call(R=0) == shape and call(B=-1) == shape and call(R=-4) == shape
    assert call(noise=one, period=-1) == shape and b"noise period" in lib.dvg_last_error()
    assert call(noise=one, period=4) == shape and b"divide R = 6" in lib.dvg_last_error()
    assert call(noise=one, period=12) == shape
    for hole in ("mean", "var", "target", "acc", "cnt"):
        assert call(**{hole: None}) == null, hole
        assert b"NULL" in lib.dvg_last_error()
    with pytest.raises(RuntimeError, match="gp_score"):
        _lib.check(null, "gp_score")


def test_wrapper_refuses_host_tensors():
    from dvg_amd import ops
    z = torch.zeros(3, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gp_score(z, z, z, torch.zeros(3, 14, dtype=torch.float64), torch.zeros(3, 14, dtype=torch.int64))


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def _f(a):
    return np.array(a, np.float32)


def test_reference_on_hand_made_entries():
    # one row, v = 0.25 + 0.75 = 1: e = 0.5 (inside 68 %), -1.5 (inside 95 %), 2.5 (outside), and five entries that are skipped
    mean = _f([[0.0, 0.0, 0.0, NAN, 0.0, 0.0, 0.0, 0.0]])
    var = _f([[0.25, 0.25, 0.25, 0.25, INF, 0.25, -0.75, -2.0]])
    target = _f([[0.5, -1.5, 2.5, 0.0, 0.0, -INF, 0.0, 0.0]])
    acc, cnt, absum = ref.accumulate(mean, var, _f([0.75]), 0, target)
    assert cnt[0].tolist() == [3, 5, 1, 2, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1]     # deciles: Phi(-1.5) = .067, Phi(.5) = .69, Phi(2.5) = .99
    assert acc[0, 1] == 1.5 and acc[0, 2] == 8.75 and acc[0, 3] == 3.0 and acc[0, 4] == 1.5 and acc[0, 5] == 8.75
    assert acc[0, 6] == 1.5 and acc[0, 7] == 8.75 and acc[0, 8] == 3.0 and acc[0, 11] == 4.5 and acc[0, 12] == 0.0 and acc[0, 13] == 3.0
    assert acc[0, 9] == 0.0625 + 5.0625 + 39.0625 and acc[0, 10] == 8.75
    assert acc[0, 0] == pytest.approx(0.5 * (3 * ref.LN_2PI + 8.75), rel=1e-15)
    assert absum[0, 1] == 4.5 and absum[0, 2] == 8.75
    # without noise the same entries have v = 0.25: e^2 <= v only for 0.5 (equality counts), -0.75 and -2.0 stay skipped
    acc0, cnt0, _ = ref.accumulate(mean, var, None, 0, target)
    assert cnt0[0, :4].tolist() == [3, 5, 1, 1] and acc0[0, 3] == 0.75
    # accumulated into: a second call doubles everything; a period: row r uses noise[r % P]
    acc2, cnt2, _ = ref.accumulate(mean, var, _f([0.75]), 0, target, acc.copy(), cnt.copy())
    assert np.array_equal(acc2, 2 * acc) and np.array_equal(cnt2, 2 * cnt)
    m4 = np.zeros((4, 1), np.float32)
    acc4, _, _ = ref.accumulate(m4, m4 + 1, _f([1.0, 3.0]), 2, m4)
    assert acc4[:, 3].tolist() == [2.0, 4.0, 2.0, 4.0]
    # an entry ON an edge has margin 0, the three taken entries above keep away from all of them
    assert ref.margins((m4, m4 + 1, None, 0, m4 + 1)) == 0.0
    assert 0.05 < ref.margins((mean, var, _f([0.75]), 0, target)) < 1.0


def test_input_sets_keep_their_margin_and_carry_the_special_entries():
    for R, B, period in ref.SHAPES:
        for noise in (True, False):
            mean, var, nz, p, target = ref.case(R, B, period, noise)          # asserts the margin
            assert mean.shape == var.shape == target.shape == (R, B) and mean.dtype == var.dtype == target.dtype == np.float32
            assert (nz is None) == (not noise) and p == period
            acc, cnt, absum = ref.accumulate(mean, var, nz, p, target)
            assert int(cnt[:, :2].sum()) == R * B and np.array_equal(cnt[:, 4:].sum(1), cnt[:, 0])
            assert np.all(cnt[:, 2] <= cnt[:, 3]) and np.all(cnt[:, 3] <= cnt[:, 0])
            if R * B >= 32:
                for a in (mean, var, target):
                    assert np.isnan(a).sum() == 1 and np.isposinf(a).sum() == 1 and np.isneginf(a).sum() == 1
                assert (var == 0).sum() == 1 and (var < 0).sum() == 3
                if R * B > 82:        # (below, two special values share an entry)
                    assert int(cnt[:, 1].sum()) == (10 if noise else 12)      # var = 0 and -0.005 are taken once there is noise
            assert np.all(np.isfinite(acc))
    mean, var, nz, p, target = ref.case(90, 128)
    _, cnt, _ = ref.accumulate(mean, var, nz, p, target)
    assert cnt[:, 4:].sum(0).min() > 500                                      # every decile is exercised


# ---- summarise / report ---------------------------------------------------------------------------------------------------------------
def _calibrated_rows(n=200):
    """Hand-made accumulators of a perfectly calibrated row: v = 1, the residuals e are the standard normal's quantiles at
    (i + 1/2) / n - their decile counts are exactly n / 10, 136 of 200 lie within one sigma, 190 within 1.96 - rescaled to unit
    sample variance; y = e."""
    e = [statistics.NormalDist().inv_cdf((i + 0.5) / n) for i in range(n)]
    inside = (sum(x * x <= 1.0 for x in e), sum(x * x <= ref.CHI2_95 for x in e))
    pit = [sum(sum(x * abs(x) > c for c in ref.EDGES) == k for x in e) for k in range(10)]
    scale = 1.0 / math.sqrt(math.fsum(x * x for x in e) / n)
    e = [x * scale for x in e]
    s = lambda f: math.fsum(f(x) for x in e)      # noqa: E731
    acc = [0.5 * (n * ref.LN_2PI + s(lambda x: x * x)), s(lambda x: x), s(lambda x: x * x), float(n), s(lambda x: x),
           s(lambda x: x * x), s(lambda x: x), s(lambda x: x * x), float(n), s(lambda x: x ** 4), s(lambda x: x * x),
           s(abs), 0.0, float(n)]
    return acc, [n, 0, inside[0], inside[1]] + pit


def test_summarise_on_hand_made_accumulators():
    from dvg_amd import gp_score
    acc, cnt = _calibrated_rows()
    s = gp_score.summarise([acc], [cnt])
    assert s["taken"] == 200 and s["skipped"] == 0
    assert s["cover68"] == 0.68 and s["cover95"] == 0.95 and s["pit"] == [0.1] * 10 and s["pit_err"] == 0.0
    assert s["z_std"] == pytest.approx(1.0, abs=1e-12) and s["z_mean"] == pytest.approx(0.0, abs=1e-12)
    assert s["nlpd"] == pytest.approx(0.5 * (ref.LN_2PI + 1.0), rel=1e-12) and s["rmse"] == pytest.approx(1.0, rel=1e-12)
    assert s["mean_var"] == 1.0 and s["smse"] == pytest.approx(1.0, rel=1e-12)          # y = e: the error IS the spread
    assert s["var_err_corr"] is None                                                   # v is the same everywhere: no correlation
    # pooled with a row of nothing but skipped entries: the same numbers; that row alone: None
    nothing = ([0.0] * 14, [0, 7] + [0] * 12)
    both = gp_score.summarise([acc, nothing[0]], [cnt, nothing[1]])
    assert both == dict(s, skipped=7)
    empty = gp_score.summarise([nothing[0]], [nothing[1]])
    assert empty["taken"] == 0 and empty["skipped"] == 7
    assert all(empty[k] is None for k in empty if k not in ("taken", "skipped")) and len(empty) == 14
    assert "null" in json.dumps(empty)
    # a dim whose target never moves: no smse; everything else is there
    n, y, e, v = 4, 0.3, [0.1, -0.2, 0.3, -0.1], [1.0, 2.0, 3.0, 4.0]
    flat = [math.fsum(0.5 * (ref.LN_2PI + math.log(b) + a * a / b) for a, b in zip(e, v)), math.fsum(e),
            math.fsum(a * a for a in e), math.fsum(v), math.fsum(a / math.sqrt(b) for a, b in zip(e, v)),
            math.fsum(a * a / b for a, b in zip(e, v)), n * y, n * y * y, math.fsum(b * b for b in v),
            math.fsum(a ** 4 for a in e), math.fsum(b * a * a for a, b in zip(e, v)), math.fsum(abs(a) for a in e),
            math.fsum(math.log(b) for b in v), math.fsum(math.sqrt(b) for b in v)]
    s = gp_score.summarise([flat], [[n, 0, 4, 4, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0]])
    assert s["smse"] is None and s["cover68"] == 1.0 and s["mae"] == pytest.approx(0.175)
    assert s["var_err_corr"] == pytest.approx(float(np.corrcoef(v, [a * a for a in e])[0, 1]), rel=1e-9)
    assert s["pit_err"] == pytest.approx(0.5 * (4 * 0.15 + 6 * 0.1))
    # a sum that overflowed: nothing finite behind the numbers
    assert gp_score.summarise([[INF] + flat[1:]], [[n, 0, 4, 4, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0]])["nlpd"] is None


def test_report_pools_over_steps_and_dims_like_the_reference():
    from dvg_amd import gp_score
    steps, dims, B = 3, 5, 33
    mean, var, nz, p, target = ref.case(steps * dims, B, dims)
    acc, cnt, _ = ref.accumulate(mean, var, nz, p, target)
    rep = gp_score.report(acc.tolist(), cnt.tolist(), steps, dims)
    assert sorted(rep) == ["per_dim", "per_step", "pooled", "worst_dims"]
    assert len(rep["per_step"]) == steps and len(rep["per_dim"]) == dims

    def by_hand(rows):
        """The scores of the entries of `rows` from the entries themselves, not from per-row sums."""
        taken, v, y, e = ref._entries(mean[rows], var[rows], nz[np.array(rows) % dims], 0, target[rows])
        v, y, e = v[taken], y[taken], e[taken]
        z = e / np.sqrt(v)
        return {"nlpd": float(np.mean(0.5 * (ref.LN_2PI + np.log(v) + e * e / v))), "rmse": float(np.sqrt(np.mean(e * e))),
                "mae": float(np.mean(np.abs(e))), "mean_var": float(np.mean(v)), "z_mean": float(np.mean(z)), "z_std": float(np.std(z)),
                "cover68": float(np.mean(e * e <= v)), "cover95": float(np.mean(e * e <= ref.CHI2_95 * v)),
                "var_err_corr": float(np.corrcoef(v, e * e)[0, 1]), "smse": float(np.sum(e * e) / np.sum((y - y.mean()) ** 2)),
                "taken": int(taken.sum()), "skipped": int((~taken).sum())}

    def same(got, rows):
        want = by_hand(rows)
        for k, w in want.items():
            assert got[k] == pytest.approx(w, rel=1e-10, abs=1e-12), k
        assert sum(got["pit"]) == pytest.approx(1.0) and got["pit_err"] == pytest.approx(0.5 * sum(abs(q - 0.1) for q in got["pit"]))
    same(rep["pooled"], list(range(steps * dims)))
    for s in range(steps):
        same(rep["per_step"][s], list(range(s * dims, (s + 1) * dims)))
    for d in range(dims):
        same(rep["per_dim"][d], [s * dims + d for s in range(steps)])
    nl = [rep["per_dim"][d]["nlpd"] for d in range(dims)]
    assert rep["worst_dims"] == sorted(range(dims), key=lambda d: -nl[d])[:5] and len(rep["worst_dims"]) == 5
    with pytest.raises(ValueError, match="rows"):
        gp_score.report(acc.tolist(), cnt.tolist(), steps, dims + 1)
    assert gp_score.track_steps(2, 5) == {"forced": 4, "rollout": 3}


# ---- the flags and the log ------------------------------------------------------------------------------------------------------------
def test_flag_needs_val_every_and_leaves_no_trace_without_it():
    import generate_frames
    import train
    from dvg_amd import train_state, validate
    assert not hasattr(train.options([]), "val_gp")
    assert validate.options(train.options(["--val_every", "2"])) == {"every": 2, "batches": 8, "nsample": 4}
    with pytest.raises(SystemExit) as exc:
        train.options(["--val_gp"])
    assert "--val_gp" in str(exc.value) and "--val_every" in str(exc.value) and "\n" not in str(exc.value)
    with pytest.raises(SystemExit, match="--val_every"):
        validate.options(argparse.Namespace(val_gp=True, n_eval=4, n_past=2))
    o = train.options(["--val_every", "2", "--val_gp"])
    assert o.val_gp is True and validate.options(o) == {"every": 2, "batches": 8, "nsample": 4, "gp": True}
    plain = train.options(["--val_every", "2"])
    assert train_state.option_fingerprint(o) == train_state.option_fingerprint(plain) and "val_gp" not in train_state.OPTION_FIELDS
    g = generate_frames.build_parser()
    assert g.parse_args([]).gp_report is False and g.parse_args(["--gp_report"]).gp_report is True


def test_a_record_with_a_gp_key_goes_through_the_log(tmp_path):
    from dvg_amd import gp_score, validate
    acc, cnt = _calibrated_rows()
    nothing = ([0.0] * 14, [0, 3] + [0] * 12)
    gp = {"forced": gp_score.report([acc, nothing[0]], [cnt, nothing[1]], 1, 2),
          "rollout": gp_score.report([nothing[0]], [nothing[1]], 1, 1)}
    assert gp["forced"]["worst_dims"] == [0] and gp["rollout"]["worst_dims"] == []
    rec = {"epoch": 0, "global_step": 2, "clips": 8, "steps": 2, "nsample": 0, "score": 0.5, "tracks": {}, "gp": gp}
    plain = validate._plain(rec)
    assert plain == rec and plain is not rec                                  # None stays None, nothing else to replace
    text = validate.log_text([rec, dict(rec, epoch=1, gp=dict(gp, forced=dict(gp["forced"], pooled=dict(gp["forced"]["pooled"], nlpd=NAN))))])
    assert "NaN" not in text and text.count("\n") == 2
    path = validate.write_log([rec], str(tmp_path))
    back = validate.read_log(path)
    assert back == [rec] and back[0]["gp"]["forced"]["pooled"]["cover68"] == 0.68
    assert json.loads(text.splitlines()[1])["gp"]["forced"]["pooled"]["nlpd"] is None
    line = gp_score.line("val gp", gp)
    assert line.startswith("     val gp: nlpd 1.4189 rmse 1.00000 mean var 1.00000 z std 1.000 cover 68/95 0.680 / 0.950 pit err 0.000 "
                           "var~err corr nan  | rollout: nlpd nan z std nan cover 95 nan")
    assert gp_score.curves("forced", gp["forced"]).count("\n") == 1
    out = gp_score.write_report(gp, str(tmp_path / "gen"))
    assert os.path.basename(out) == "gp_report.json" and json.load(open(out)) == gp
    assert sorted(os.listdir(tmp_path / "gen")) == ["gp_report.json"]
