"""CPU: train.py --val_every without a GPU - the library exports and binds dvg_val_accumulate and its host-side checks fire before
any launch; the three flags and the option fingerprint; tests/val_ref.py (the fp64 restatement the GPU tests compare the kernel
with) on hand-made arrays; the selection rule; the history's trip through a state dict into val_log.jsonl and back."""
import argparse
import ctypes
import io
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import val_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


# ---- the library ----------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_binds_val_accumulate():
    from dvg_amd import _lib, ops
    assert "dvg_val_accumulate" in _lib.SIGNATURES and len(_lib.SIGNATURES["dvg_val_accumulate"][1]) == 10
    for name in ("libdvg_hip.so", "libdvg_hip_f32mfma.so"):
        assert hasattr(ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), name)), "dvg_val_accumulate"), name
    assert _lib.lib().dvg_abi_version() == 9
    assert "validate.hip" in open(os.path.join(ROOT, "dvg_amd", "csrc", "Makefile")).read().split("SRCS")[1].splitlines()[0]
    assert callable(ops.val_accumulate) and callable(ops.val_accumulators)


def test_host_side_checks_refuse_bad_calls_without_a_gpu():
    from dvg_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(16)          # fake, never dereferenced: every call must fail in the checks
    assert lib.dvg_val_accumulate(one, one, one, 0, 1, 1, one, one, None, None) == 1 and b"B, S and T" in lib.dvg_last_error()
    assert lib.dvg_val_accumulate(one, one, one, 1, 0, 1, one, one, None, None) == 1
    assert lib.dvg_val_accumulate(one, one, one, 1, 1, -3, one, one, None, None) == 1
    assert lib.dvg_val_accumulate(one, one, one, 1 << 11, 1 << 10, 1 << 10, one, one, None, None) == 1     # B S T = 2^31
    assert b"2^31" in lib.dvg_last_error()
    for hole in range(3):
        args = [one, one, one]
        args[hole] = None
        assert lib.dvg_val_accumulate(*args, 2, 2, 2, one, one, None, None) == 2
    assert lib.dvg_val_accumulate(one, one, one, 2, 2, 2, None, one, None, None) == 2
    assert lib.dvg_val_accumulate(one, one, one, 2, 2, 2, one, None, one, None) == 2 and b"NULL" in lib.dvg_last_error()
    with pytest.raises(RuntimeError, match="val_accumulate"):
        _lib.check(2, "val_accumulate")


def test_wrapper_checks_device_dtype_shape_and_contiguity():
    from dvg_amd import ops
    z = torch.zeros(2, 2, 3)
    acc, cnt = torch.zeros(2, 3, 3, 2, dtype=torch.float64), torch.zeros(2, 3, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.val_accumulate(z, z, z, acc, cnt)


# ---- the flags ------------------------------------------------------------------------------------------------------------------------
def test_parser_takes_the_three_flags_and_the_fingerprint_ignores_them(capsys):
    import train
    from dvg_amd import train_state, validate
    p = train.build_parser()
    o = p.parse_args([])
    assert (o.val_every, o.val_batches, o.val_nsample) == (0, 8, 4) and validate.options(o) is None
    w = p.parse_args(["--val_every", "3", "--val_batches", "2", "--val_nsample", "0"])
    assert validate.options(w) == {"every": 3, "batches": 2, "nsample": 0}
    for bad in (["--val_every", "-1"], ["--val_batches", "0"], ["--val_nsample", "-1"]):
        with pytest.raises(SystemExit) as exc:
            p.parse_args(bad)
        assert bad[0] in str(exc.value)
    for x in (o, w):
        x.ft, x.world = not x.no_ft, 1
    assert train_state.option_fingerprint(o) == train_state.option_fingerprint(w)
    assert not {"val_every", "val_batches", "val_nsample"} & set(train_state.OPTION_FIELDS)
    old = argparse.Namespace(n_eval=4, n_past=2)                      # an options object from before the flags
    assert validate.options(old) is None and validate.make(old, "cpu") is None
    w.n_eval, w.n_past = 5, 5
    with pytest.raises(SystemExit, match="n_eval"):
        validate.options(w)
    import generate_frames
    assert generate_frames.build_parser().parse_args(["--best"]).best is True
    with pytest.raises(SystemExit) as exc:
        validate.best_checkpoint_path("/nonexistent/dir", False)
    assert "model_best.pth" in str(exc.value) and "\n" not in str(exc.value)
    with pytest.raises(SystemExit, match="model_ema_best.pth"):
        validate.best_checkpoint_path("/nonexistent/dir", True)


# ---- the reference on hand-made arrays ------------------------------------------------------------------------------------------------
def _f(a):
    return np.array(a, np.float32)


def test_reference_best_rule():
    ssim = _f([[[0.5, 0.25], [0.25, 0.5], [0.1, 0.1]],           # a tie between samples 0 and 1: the lowest
               [[NAN, 0.9], [-0.5, -0.5], [-0.2, -0.3]],         # a NaN sum loses, -0.5 < -1.0 is false: sample 2
               [[NAN, 0.0], [0.0, NAN], [NAN, NAN]],             # all NaN: 0
               [[-INF, 0.0], [NAN, 1.0], [-INF, 0.0]]])          # -inf is a sum like any other and beats NaN; tie: the lowest
    assert ref.best_samples(ssim).tolist() == [0, 2, 0, 0]
    assert ref.best_samples(_f([[[0.1], [0.3], [0.3], [0.2]]])).tolist() == [1]
    # fp64 sums from 0.0, t ascending: 2^24 + 1 + 1 is 2^24 + 2 in fp64 (fp32 would stay at 2^24 and tie with sample 1)
    big = _f([[[2.0 ** 24, 1.0, 1.0], [2.0 ** 24, 0.0, 1.0]]])
    assert ref.best_samples(big).tolist() == [0] and ref.best_samples(big[:, ::-1]).tolist() == [1]


def test_reference_excludes_what_is_not_finite_and_counts_what_it_takes():
    ssim = _f([[[0.5, 0.5], [0.9, 0.9]], [[0.2, 0.2], [0.1, 0.1]]])          # best: 1, 0
    psnr = _f([[[20.0, INF], [INF, INF]], [[30.0, INF], [NAN, INF]]])
    mse = _f([[[0.5, NAN], [0.25, 0.125]], [[NAN, NAN], [1.0, 0.0]]])
    acc, cnt, best = ref.accumulate(ssim, psnr, mse)
    assert best.tolist() == [1, 0]
    # ssim: everything finite
    assert acc[0, 0, :, 0].tolist() == [float(np.float64(np.float32(0.9)) + np.float64(np.float32(0.2)))] * 2
    assert cnt[:, 0].tolist() == [[2, 2], [2, 2]]
    # psnr, best track: row 0 takes sample 1 (+inf: left out), row 1 sample 0 (30 at step 0, +inf at step 1)
    assert acc[0, 1, 0].tolist() == [30.0, 900.0] and cnt[0, 1].tolist() == [1, 0]
    assert acc[0, 1, 1].tolist() == [0.0, 0.0]                                # a step with nothing finite: sum 0, count 0
    # psnr, mean track: row 0 step 0 = 20 (one finite sample), row 1 step 0 = 30; step 1 has none
    assert acc[1, 1, 0].tolist() == [50.0, 1300.0] and cnt[1, 1].tolist() == [2, 0]
    # mse, best track: row 0 sample 1 -> 0.25, 0.125; row 1 sample 0 -> NaN, NaN
    assert acc[0, 2, :, 0].tolist() == [0.25, 0.125] and cnt[0, 2].tolist() == [1, 1]
    # mse, mean track: row 0 (0.5 + 0.25) / 2, 0.125 / 1; row 1 1.0 / 1, 0.0 / 1
    assert acc[1, 2, :, 0].tolist() == [0.375 + 1.0, 0.125 + 0.0] and cnt[1, 2].tolist() == [2, 2]
    assert acc[1, 2, 0, 1] == 0.375 ** 2 + 1.0
    # accumulated into: a second call doubles everything
    acc2, cnt2, _ = ref.accumulate(ssim, psnr, mse, acc.copy(), cnt.copy())
    assert np.array_equal(acc2, 2 * acc) and np.array_equal(cnt2, 2 * cnt)
    assert np.array_equal(ref.absum(ssim, psnr, mse)[..., 1], acc[..., 1])
    # the log writes a value whose count is 0 as null
    from dvg_amd import validate
    s = validate.summarise(acc[0].tolist(), cnt[0].tolist())
    assert s["psnr"]["curve"] == [30.0, None] and s["psnr"]["std"] == [0.0, None] and s["psnr"]["count"] == [1, 0]
    assert s["psnr"]["mean"] == 30.0 and "null" in json.dumps(validate._plain(s["psnr"]))
    empty = validate.summarise(np.zeros((3, 2, 2)).tolist(), np.zeros((3, 2), int).tolist())
    assert empty["ssim"] == {"mean": None, "curve": [None, None], "std": [None, None], "count": [0, 0]}


def test_reference_inputs_are_what_the_kernel_tests_say():
    for B, S, T in ref.SHAPES:
        ssim, psnr, mse = ref.inputs(B, S, T)
        assert ssim.shape == psnr.shape == mse.shape == (B, S, T) and ssim.dtype == np.float32
        assert np.abs(ssim).max() <= 1.0
        if S > 2:
            assert np.array_equal(ssim[:, 1], ssim[:, 2])
        if B > 2:
            assert np.isinf(psnr[:, :, 0]).all()
    ssim, psnr, mse = ref.inputs(130, 2, 33)
    assert 0.05 < np.isinf(psnr).mean() < 0.2 and 0.02 < np.isnan(mse).mean() < 0.1
    # numpy's pairwise order against the sequential reference stays far inside the bar
    acc, cnt, _ = ref.accumulate(ssim, psnr, mse)
    fin = np.where(np.isfinite(mse), mse.astype(np.float64), 0.0)
    u = fin.sum(1) / np.maximum(np.isfinite(mse).sum(1), 1)
    assert np.all(np.abs(u.sum(0) - acc[1, 2, :, 0]) <= ref.bar(130, 2, ref.absum(ssim, psnr, mse)[1, 2, :, 0]))


# ---- the selection rule and the history -----------------------------------------------------------------------------------------------
def _tracks(post, best):
    def t(v):
        return {m: {"mean": v, "curve": [v], "std": [0.0], "count": [1]} for m in ("ssim", "psnr", "mse")}
    return {"posterior": t(post), "best": t(best), "mean": t(best)}


def test_selection_rule():
    from dvg_amd import validate
    assert validate.selection_score(_tracks(0.3, 0.7), 2) == 0.7
    assert validate.selection_score(_tracks(0.3, None), 0) == 0.3            # no samples: the posterior track
    assert validate.improves(0.5, None) and validate.improves(0.6, 0.5)
    assert not validate.improves(0.5, 0.5) and not validate.improves(0.4, 0.5)   # strictly greater replaces, a tie keeps
    assert not validate.improves(None, None) and not validate.improves(NAN, 0.1) and not validate.improves(NAN, None)


def test_history_survives_a_state_dict_and_the_log(tmp_path):
    from dvg_amd import validate
    v = validate.Validation.__new__(validate.Validation)          # the history alone: no stream, no device
    v.load_state(None)
    assert v.history == [] and v.best_live == {"score": None, "epoch": None} == v.best_ema
    third = 1.0 / 3.0
    rec = {"epoch": 2, "global_step": 6, "clips": 8, "steps": 2, "nsample": 2, "score": third, "tracks": _tracks(0.25, third)}
    rec["tracks"]["best"]["psnr"] = {"mean": None, "curve": [None], "std": [None], "count": [0]}
    v.history.append(rec)
    v.history.append(dict(rec, epoch=3, score=INF))
    v.best_live = {"score": third, "epoch": 2}
    f = io.BytesIO()
    torch.save({"validation": v.state()}, f)
    f.seek(0)
    w = validate.Validation.__new__(validate.Validation)
    w.load_state(torch.load(f, weights_only=False)["validation"])
    assert w.history == v.history and w.best_live == v.best_live and w.best_ema == v.best_ema
    assert w.history is not v.history and w.state()["history"][0] is not w.history[0]
    path = validate.write_log(w.history, str(tmp_path / "out"))
    text = open(path).read()
    assert os.path.basename(path) == "val_log.jsonl" and text == validate.log_text(v.history) and text.count("\n") == 2
    assert "NaN" not in text and "Infinity" not in text
    back = validate.read_log(path)
    assert back[0]["epoch"] == 2 and back[0]["score"] == third and back[0]["tracks"]["best"]["psnr"]["mean"] is None
    assert back[0]["tracks"]["best"]["psnr"]["curve"] == [None] and back[1]["score"] is None
    assert back[0]["tracks"]["posterior"]["ssim"]["mean"] == 0.25
    assert validate.write_log(w.history, str(tmp_path / "out")) == path and open(path).read() == text    # rewritten whole
    assert sorted(os.listdir(tmp_path / "out")) == ["val_log.jsonl"]
    line = validate.line("val", rec, 2)
    assert line.startswith("     val: ssim 0.2500 psnr 0.25 mse 0.25000 | best of 2: ssim 0.3333 psnr nan | mean: ssim 0.3333 ")
    assert line.endswith("(8 clips x 2 steps)  best so far: epoch 2")
    assert " | " not in validate.line("val(ema)", dict(rec, nsample=0), None)
    assert math.isnan(validate._num(None))
