"""CPU: the host side of train.py --optimizer / --weight_decay - the fp64 restatement of the four rules against torch.optim in
fp64, the options and their refusals, the decay-mask builder, the resume fingerprint, and dvg_optim_step in the header, the
derived binding and the built library with its argument checks (no launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import optim_ref as ref
from tests.common import header_declaration


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", ref.DECAYS)
@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_restatement_agrees_with_torch_in_fp64(case, wd):
    """5 steps, two groups (the second with the weight decay, the first without), lr 2e-3: 1e-12 relative."""
    _, rule, a, b, nesterov = case
    rng = np.random.default_rng(5)
    p0 = [rng.standard_normal(1027), rng.standard_normal(38)]
    grads = [[rng.standard_normal(x.size) for x in p0] for _ in range(5)]
    params = [torch.nn.Parameter(torch.tensor(x, dtype=torch.float64)) for x in p0]
    o = ref.torch_optimizer(rule, [{"params": params[:1], "weight_decay": 0.0}, {"params": params[1:], "weight_decay": wd}],
                            2e-3, a, b, nesterov=nesterov)
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = torch.tensor(g, dtype=torch.float64)
        o.step()
    for k, group_wd in enumerate((0.0, wd)):
        p, m, v = ref.run(rule, p0[k], [gs[k] for gs in grads], 2e-3, a, b, weight_decay=group_wd, nesterov=nesterov)
        want = params[k].detach().numpy()
        assert np.max(np.abs(p - want) / np.maximum(np.abs(want), 1e-300)) < 1e-12, (case[0], wd, k)
        st = o.state[params[k]]
        if rule in (ref.ADAM, ref.ADAMW):
            pairs = ((m, st["exp_avg"]), (v, st["exp_avg_sq"]))
        elif rule == ref.SGD:
            pairs = ((m, st["momentum_buffer"]),) if a != 0 else ()
        else:
            pairs = ((v, st["square_avg"]),) + (((m, st["momentum_buffer"]),) if b > 0 else ())
        for mine, theirs in pairs:
            assert np.allclose(mine, theirs.numpy(), rtol=1e-12, atol=0), (case[0], wd, k)


def test_mask_guard_factor_and_rate_multiplier_of_the_restatement():
    """A masked-off piece moves as with weight decay 0, the others as without a mask; the guard factor is a factor of the
    gradient, the multiplier one of the rate."""
    rng = np.random.default_rng(6)
    n = 11
    p0, g = rng.standard_normal(n), rng.standard_normal(n)
    mask = np.array([1, 0, 1], dtype=np.uint8)
    for _, rule, a, b, nesterov in ref.CASES:
        args = dict(lr=2e-3, a=a, b=b, nesterov=nesterov)
        full = ref.run(rule, p0, [g, g], weight_decay=0.1, **args)[0]
        none = ref.run(rule, p0, [g, g], weight_decay=0.0, **args)[0]
        mixed = ref.run(rule, p0, [g, g], weight_decay=0.1, mask=mask, **args)[0]
        assert np.array_equal(mixed[4:8], none[4:8]) and np.array_equal(mixed[:4], full[:4]) and np.array_equal(mixed[8:], full[8:])
        assert not np.array_equal(full, none)
        assert np.array_equal(ref.run(rule, p0, [g], grad_scale=0.37, **args)[0], ref.run(rule, p0, [0.37 * g], **args)[0])
        args2 = dict(args, lr=2e-3 * 0.25)
        assert np.array_equal(ref.run(rule, p0, [g], lr_scale=0.25, **args)[0], ref.run(rule, p0, [g], **args2)[0])


# ---- options -------------------------------------------------------------------------------------------------------------------
def _options(argv):
    import train
    return train.options(list(argv))


@pytest.mark.parametrize("name", ["adam", "adamw", "sgd", "rmsprop"])
def test_the_four_names_are_accepted(name):
    from dvg_amd import optim
    opt = _options(["--optimizer", name])
    assert opt.optimizer == name
    spec = optim.optimizer_options(opt)
    if name == "adam":
        assert spec is None
    else:
        assert spec["rule"] == name and spec["weight_decay"] == 0.0
        assert spec["momentum"] == {"adamw": None, "sgd": 0.9, "rmsprop": 0.0}[name]
        assert spec["alpha"] == (0.99 if name == "rmsprop" else None)


@pytest.mark.parametrize("argv, word", [
    (["--optimizer", "lamb"], "--optimizer"), (["--optimizer", "Adam"], "--optimizer"), (["--optimizer", ""], "--optimizer"),
    (["--weight_decay", "-0.1"], "--weight_decay"), (["--weight_decay", "nan"], "--weight_decay"),
    (["--optimizer", "sgd", "--momentum", "-0.5"], "--momentum"), (["--optimizer", "sgd", "--momentum", "nan"], "--momentum"),
    (["--optimizer", "rmsprop", "--rmsprop_alpha", "-1"], "--rmsprop_alpha"),
    (["--optimizer", "rmsprop", "--rmsprop_alpha", "nan"], "--rmsprop_alpha"),
    (["--optimizer", "rmsprop", "--rmsprop_alpha", "1.0"], "--rmsprop_alpha"),
    (["--optimizer", "sgd", "--nesterov", "--momentum", "0"], "--nesterov"),
    (["--optimizer", "rmsprop", "--nesterov"], "--nesterov"), (["--nesterov"], "--nesterov"),
    (["--momentum", "0.9"], "--momentum"), (["--optimizer", "adamw", "--momentum", "0.9"], "--momentum"),
    (["--optimizer", "sgd", "--rmsprop_alpha", "0.9"], "--rmsprop_alpha")])
def test_refusals_are_one_line_naming_the_option(argv, word):
    with pytest.raises(SystemExit) as e:
        _options(argv)
    msg = str(e.value)
    assert msg.startswith("train.py: ") and word in msg and "\n" not in msg, msg


def test_nesterov_with_the_default_sgd_momentum_is_accepted():
    from dvg_amd import optim
    spec = optim.optimizer_options(_options(["--optimizer", "sgd", "--nesterov", "--weight_decay", "1e-4"]))
    assert spec == {"rule": "sgd", "weight_decay": 1e-4, "momentum": 0.9, "nesterov": True, "alpha": None}
    spec = optim.optimizer_options(_options(["--weight_decay", "0.01"]))
    assert spec == {"rule": "adam", "weight_decay": 0.01, "momentum": None, "nesterov": None, "alpha": None}


# what options([]) gave before the flags, field by field (the derived fields included)
BEFORE = dict(
    lr=0.002, beta1=0.9, batch_size=50, log_dir='logs', model_dir='', resume='', name='', output_path='.', data_root='path/to/data/',
    optimizer='adam', niter=601, seed=1, epoch_size=300, image_width=64, channels=1, dataset='smmnist', num_digits=2, n_past=5,
    no_ft=False, n_future=10, n_eval=15, rnn_size=256, predictor='lstm', predictor_rnn_layers=2, z_dim=10, g_dim=90, model='dcgan',
    data_threads=5, last_frame_skip=False, save_every=4, no_save=False, no_images=False, hip_graph=False, no_hip_graph=False,
    print_param_checksum=False, sync_bn=False, synthetic_data=False, clip_grad_norm=0.0, skip_nonfinite=False, ema_decay=None,
    augment='', val_every=0, val_batches=8, val_nsample=4, lr_schedule=None, lr_warmup=None, lr_total=None, lr_min_ratio=None,
    lr_step_every=None, lr_gamma=None, frame_loss='mse', charbonnier_eps=0.001, gdl_weight=0.0, ssim_weight=0.0, ft=True, rank=0,
    world=1, local_batch=50)


def test_defaults_leave_every_existing_option_as_it_was():
    from dvg_amd import lr_schedule, optim
    opt = _options([])
    have = vars(opt)
    for k, v in BEFORE.items():
        assert have[k] == v, k
    new = {"weight_decay": 0.0, "momentum": None, "nesterov": False, "rmsprop_alpha": None}
    for k, v in new.items():
        assert have[k] == v, k
    assert set(have) == set(BEFORE) | set(new)
    assert optim.optimizer_options(opt) is None
    assert lr_schedule.base_rate(opt) == 0.002 == lr_schedule.base_rate(_options(["--lr", "0.5"]))       # --lr stays unused ...
    assert lr_schedule.base_rate(_options(["--lr", "0.5", "--weight_decay", "0.1"])) == 0.002            # ... for adam
    assert lr_schedule.base_rate(_options(["--lr", "0.5", "--optimizer", "sgd"])) == 0.5
    assert lr_schedule.base_rate(_options(["--optimizer", "sgd"])) == 0.002                              # the default does not move
    old = type("Opt", (), {"lr": 0.1})()                          # an options object from before the flags
    assert optim.optimizer_options(old) is None and lr_schedule.base_rate(old) == 0.002


# ---- the decay mask ----------------------------------------------------------------------------------------------------------------
def _modules():
    import importlib
    from dvg_amd.models import lstm as lstm_models
    from dvg_amd.models.gp_models import GaussianLikelihood, GPRegressionLayer1
    model = importlib.import_module("dvg_amd.models.dcgan_64")
    return {"encoder": model.encoder(16, 1), "decoder": model.decoder(16, 1),
            "frame_predictor": lstm_models.lstm(16, 16, 32, 2, 4), "gp": GPRegressionLayer1(num_dims=16),
            "likelihood": GaussianLikelihood(batch_size=16)}


def test_mask_marks_exactly_the_weight_matrices_in_whole_pieces():
    from dvg_amd import optim
    mods = _modules()
    assert optim.DECAYING_MODULES == ("encoder", "decoder", "frame_predictor")
    for name, mod in mods.items():
        params = [p for p in mod.parameters() if p.requires_grad]
        offs, n = optim.flat_offsets(params)
        assert n % 4 == 0 and all(o % 4 == 0 for o in offs) and n == optim.FlatArena.size_for(params)
        mask = optim.decay_mask(params, lambda p, name=name: optim.decays(name, p))
        assert mask.dtype == torch.uint8 and mask.shape == (n // 4,) and not mask.is_cuda
        want = torch.zeros(n // 4, dtype=torch.uint8)
        kinds = set()
        for p, o in zip(params, offs):
            pieces = slice(o // 4, (o + p.numel() + 3) // 4)
            marked = name in ("encoder", "decoder", "frame_predictor") and p.dim() >= 2
            want[pieces] = int(marked)
            assert bool(mask[pieces].all()) == marked and bool(mask[pieces].any()) == marked, (name, tuple(p.shape))
            kinds.add((p.dim() >= 2, marked))
        assert torch.equal(mask, want), name
        if name in ("gp", "likelihood"):
            assert not mask.any(), name
            assert any(p.dim() >= 2 for p in params) or name == "likelihood"
        else:
            assert kinds == {(True, True), (False, False)}, name      # weights decay; biases and BatchNorm affine do not
    bn = [p for m in mods["encoder"].modules() if isinstance(m, torch.nn.BatchNorm2d) for p in m.parameters()]
    assert bn and not any(optim.decays("encoder", p) for p in bn)
    odd = [torch.nn.Parameter(torch.zeros(3, 3)), torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(2, 1)),
           torch.nn.Parameter(torch.zeros(7), requires_grad=False)]
    assert optim.decay_mask(odd, lambda p: p.dim() >= 2).tolist() == [1, 1, 1, 0, 0, 1]      # 9 -> 12, 5 -> 8, 2 -> 4 floats


# ---- the resume fingerprint -----------------------------------------------------------------------------------------------------
def test_fingerprint_absent_means_adam_and_a_mismatch_names_the_field():
    from dvg_amd import train_state
    assert train_state.ABSENT_MEANS["optimizer"] == "adam" and train_state.ABSENT_MEANS["predictor"] == "lstm"
    adam, sgd = _options([]), _options(["--optimizer", "sgd"])
    fp_adam, fp_sgd = train_state.option_fingerprint(adam), train_state.option_fingerprint(sgd)
    assert sorted(fp_adam) == sorted(train_state.OPTION_FIELDS + ("world",))          # the fingerprint an adam run always wrote
    assert train_state.option_fingerprint(_options(["--weight_decay", "0.1"])) == fp_adam
    assert fp_sgd == {**fp_adam, "optimizer": "sgd"}
    train_state.check_fingerprint(fp_adam, fp_adam, "<state>")
    train_state.check_fingerprint(fp_sgd, fp_sgd, "<state>")
    for saved, now in ((fp_adam, fp_sgd), (fp_sgd, fp_adam), (fp_sgd, train_state.option_fingerprint(_options(["--optimizer", "rmsprop"])))):
        with pytest.raises(SystemExit) as e:
            train_state.check_fingerprint(saved, now, "<state>")
        assert "optimizer is" in str(e.value) and "\n" not in str(e.value)


# ---- the entry point ---------------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree():
    from dvg_amd import _lib
    name = "dvg_optim_step"
    ret, params = header_declaration(name)             # tests/test_abi.py holds every declaration's binding and export
    restype, argtypes = _lib.SIGNATURES[name]
    assert ret == "int" and restype is ctypes.c_int and len(argtypes) == len(params) == 19, (len(argtypes), params)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert hasattr(ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libdvg_hip_f32mfma.so")), name)
    assert _lib.lib().dvg_abi_version() == 9


SHAPE, NULL, ALIGN = 1, 2, 4


def test_argument_checks_fire_before_any_launch():
    """The codes of dvg_adam_step_scheduled's checks, each message naming dvg_optim_step."""
    from dvg_amd import _lib
    lib = _lib.lib()
    ok, odd4, odd = ctypes.c_void_p(64), ctypes.c_void_p(68), ctypes.c_void_p(66)      # never dereferenced
    step = lib.dvg_optim_step

    def call(rule=0, p=ok, g=ok, m=ok, v=ok, n=8, mask=None, t=1, tdev=None, stat=None, skips=None, scale=None):
        rc = step(rule, p, g, m, v, n, 2e-3, 0.9, 0.999, 1e-8, 0.0, 0, mask, t, tdev, stat, skips, scale, None)
        assert rc == 0 or b"dvg_optim_step" in lib.dvg_last_error(), lib.dvg_last_error()
        return rc
    for rule in range(4):
        for k in ("p", "g", "m"):
            assert call(rule, **{k: None}) == NULL, (rule, k)
        assert call(rule, v=None, p=odd4) == (ALIGN if rule == 2 else NULL), rule      # v is SGD's to leave out
        assert call(rule, stat=ok) == NULL and call(rule, skips=ok) == NULL
        assert b"together" in lib.dvg_last_error()
        assert call(rule, n=0) == SHAPE and call(rule, n=-4) == SHAPE and call(rule, t=0) == SHAPE
        for k in ("p", "g", "m", "v"):
            assert call(rule, **{k: odd4}) == ALIGN, (rule, k)
        assert call(rule, scale=odd) == ALIGN and call(rule, tdev=odd, t=0) == ALIGN
        assert call(rule, stat=odd, skips=ok) == ALIGN and call(rule, stat=ok, skips=odd) == ALIGN
    for rule in (-1, 4, 99):
        assert call(rule) == SHAPE, rule
    assert b"rule" in lib.dvg_last_error()


def test_ops_wrapper_refuses_host_tensors_and_unknown_rules():
    from dvg_amd import ops
    z = torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.optim_step(ops.SGD, z, z, z, None, 1e-3, 0.9, 0.0, 0.0, 0.0, 0, None, 1, None)
    with pytest.raises(RuntimeError, match="rule"):
        ops.optim_step(7, z, z, z, z, 1e-3, 0.9, 0.0, 0.0, 0.0, 0, None, 1, None)
    assert (ops.ADAM, ops.ADAMW, ops.SGD, ops.RMSPROP, ops.NESTEROV) == (0, 1, 2, 3, 1)
    assert (ref.ADAM, ref.ADAMW, ref.SGD, ref.RMSPROP) == (0, 1, 2, 3)


def test_classes_refuse_invalid_hyper_parameters():
    from dvg_amd import optim
    p = [torch.nn.Parameter(torch.zeros(4))]
    assert set(optim.RULES) == {"adam", "adamw", "sgd", "rmsprop"}
    assert all(issubclass(c, optim.FusedOptimizer) for c in optim.RULES.values()) and optim.RULES["adam"] is optim.FusedAdam
    for make in (lambda: optim.FusedSGD(p, momentum=-0.1), lambda: optim.FusedSGD(p, nesterov=True),
                 lambda: optim.FusedSGD(p, weight_decay=float("nan")), lambda: optim.FusedRMSprop(p, alpha=1.0),
                 lambda: optim.FusedRMSprop(p, momentum=-1.0), lambda: optim.FusedAdamW(p, weight_decay=-1.0),
                 lambda: optim.FusedAdam(p, betas=(1.0, 0.9))):
        with pytest.raises(ValueError):
            make()
