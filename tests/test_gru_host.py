"""CPU: the GRU / RNN frame predictors (--predictor gru|rnn) as far as they go without a GPU - the reference's own outputs and
gradients (tests/golden/reference_gru.npz) against the fp64 restatement tests/gru_ref.py, the bars of tests/test_gpu_gru.py shown
to catch every planted defect while torch's own fp32 cells pass them, the new entry points in the header / the library / the
binding table and their host-side checks, the reference's pickled modules loading into our classes, the flag and the --resume
fingerprint."""
import ctypes
import gzip
import io
import os

import numpy as np
import pytest
import torch

from oracle import params
from tests import gru_ref
from tests.common import header_symbols, rel_err

HERE = os.path.dirname(os.path.abspath(__file__))
FWD_BAR, GRAD_BAR = 1e-5, 2e-5         # the GPU tests' bars against fp64 (the project's own for the LSTM)
SHAPE, B, STEPS = (90, 90, 64, 2), 5, 3
SEEDS = {"gru": 500, "rnn": 520}        # tests/golden/make_golden_gru.py
NEW_SYMBOLS = ("dvg_gru_cell", "dvg_gru_cell_pre", "dvg_rnn_cell", "dvg_gru_gates_bwd")
CELL_SHAPES = [(5, 64), (33, 64), (9, 128), (64, 256), (5, 256)]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "reference_gru.npz"))


def state_dict(kind):
    import dvg_amd.models.lstm as ours
    return params.fill_state_dict(getattr(ours, kind)(*SHAPE, B).state_dict(), SEEDS[kind])


def fingerprint(t, k=64):
    f = t.detach().double().reshape(-1)
    idx = torch.linspace(0, f.numel() - 1, k).long()
    return torch.cat([torch.stack([f.sum(), f.abs().sum(), (f * f).sum()]), f[idx]])


@pytest.mark.parametrize("kind", ["gru", "rnn"])
def test_golden_outputs_and_gradients_equal_the_fp64_restatement(golden, kind):
    """The reference's fp32 outputs, final states and 3-step BPTT gradients against tests/gru_ref.py in fp64: 1e-6."""
    sd, seed = state_dict(kind), SEEDS[kind]
    sd64 = {k: v.double() for k, v in sd.items()}
    xs = torch.stack([params.normal(seed + 10 + t, B, 90, scale=0.5) for t in range(STEPS)])
    ws = torch.stack([params.normal(seed + 15 + t, B, 90) for t in range(STEPS)])
    hidden = gru_ref.init_hidden(B, SHAPE[2], SHAPE[3])
    ys = torch.stack([gru_ref.module_step(xs[t].double(), sd64, hidden, kind) for t in range(STEPS)])
    assert rel_err(torch.from_numpy(golden[f"{kind}/y"]), ys) < 1e-6
    for i in range(SHAPE[3]):
        assert rel_err(torch.from_numpy(golden[f"{kind}/h{i}"]), hidden[i]) < 1e-6
    y, g = gru_ref.bptt(sd, xs, ws, kind, SHAPE[3])
    assert rel_err(y, ys) == 0.0
    assert abs(float((y * ws.double()).sum()) - float(golden[f"{kind}_grad/loss"][0])) < 1e-5
    for k in sd:
        assert rel_err(torch.from_numpy(golden[f"{kind}_grad/{k}"])[3:], fingerprint(g[k])[3:]) < 1e-6, k
    for t in range(STEPS):
        assert rel_err(torch.from_numpy(golden[f"{kind}_grad/x{t}"]), g["x"][t]) < 1e-6


def cell_case(Bc, H, gates, seed=600):
    x, h = (params.normal(seed + i, Bc, H, scale=0.6) for i in range(2))
    w_ih, w_hh = (params.normal(seed + 2 + i, gates * H, H, scale=1.0 / H ** 0.5) for i in range(2))
    b_ih, b_hh = (params.normal(seed + 4 + i, gates * H, scale=0.3) for i in range(2))
    d = params.normal(seed + 6, Bc, H)
    return x, h, w_ih, w_hh, b_ih, b_hh, d


def autograd_cell(fn, args, d, dtype):
    leaf = [a.to(dtype).clone().requires_grad_(True) for a in args]
    out = fn(*leaf)
    h2 = out[0] if isinstance(out, tuple) else out
    (h2 * d.to(dtype)).sum().backward()
    return h2.detach(), dict(zip(("x", "h", "w_ih", "w_hh", "b_ih", "b_hh"), (a.grad for a in leaf)))


@pytest.mark.parametrize("Bc,H", CELL_SHAPES)
def test_the_bars_catch_every_planted_defect_and_pass_torchs_own_fp32_cells(Bc, H):
    """On the shapes of the GPU tests: (1) the hand-written backward (gru_ref.gru_cell_backward: dvg_gru_gates_bwd's formulas +
    GEMMs) equals fp64 autograd of torch._VF.gru_cell to rounding; (2) torch's fp32 nn.GRUCell / nn.RNNCell arithmetic passes the
    bars against fp64, output and all six gradients; (3) each planted defect misses them."""
    *args, d = cell_case(Bc, H, 3)
    a64 = [a.double() for a in args]
    vf = lambda x, h, wi, wh, bi, bh: torch._VF.gru_cell(x, h, wi, wh, bi, bh)      # noqa: E731
    h_ref, g_ref = autograd_cell(vf, args, d, torch.float64)
    h2, acts = gru_ref.gru_cell(*a64)
    assert rel_err(h2, h_ref) < 1e-14
    hand = gru_ref.gru_cell_backward(d.double(), a64[0], a64[1], a64[2], a64[3], acts)
    for k, v in hand.items():
        assert rel_err(v, g_ref[k]) < 1e-13, k
    h32, g32 = autograd_cell(vf, args, d, torch.float32)
    assert rel_err(h32, h_ref) < FWD_BAR
    for k in g_ref:
        assert rel_err(g32[k], g_ref[k]) < GRAD_BAR, k
    for defect in gru_ref.FORWARD_DEFECTS:
        bad, bad_acts = gru_ref.gru_cell(*a64, defect=defect)
        assert rel_err(bad, h_ref) > 100 * FWD_BAR, defect
    for defect in gru_ref.BACKWARD_DEFECTS:
        bad = gru_ref.gru_cell_backward(d.double(), a64[0], a64[1], a64[2], a64[3], acts, defect=defect)
        worst = max(rel_err(bad[k], g_ref[k]) for k in bad)
        assert worst > 100 * GRAD_BAR, defect
        dGi, dGh, dhp = gru_ref.gates_bwd(d.double(), acts, a64[1])
        bGi, bGh, bhp = gru_ref.gates_bwd(d.double(), acts, a64[1], defect=defect)
        assert max(rel_err(bGh[:, 2 * H:], dGh[:, 2 * H:]), rel_err(bhp, dhp)) > 100 * GRAD_BAR, defect
    # nn.RNNCell
    *rargs, d = cell_case(Bc, H, 1, seed=620)
    rvf = lambda x, h, wi, wh, bi, bh: torch._VF.rnn_tanh_cell(x, h, wi, wh, bi, bh)      # noqa: E731
    r_ref, rg_ref = autograd_cell(rvf, rargs, d, torch.float64)
    r64 = [a.double() for a in rargs]
    r2 = gru_ref.rnn_cell(*r64)
    assert rel_err(r2, r_ref) < 1e-14
    for k, v in gru_ref.rnn_cell_backward(d.double(), r64[0], r64[1], r64[2], r64[3], r2).items():
        assert rel_err(v, rg_ref[k]) < 1e-13, k
    r32, rg32 = autograd_cell(rvf, rargs, d, torch.float32)
    assert rel_err(r32, r_ref) < FWD_BAR
    for k in rg_ref:
        assert rel_err(rg32[k], rg_ref[k]) < GRAD_BAR, k


def test_header_library_and_binding_table_carry_the_new_entry_points():
    from dvg_amd import _lib
    syms = header_symbols()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in syms, f"{s} not declared in include/dvg_hip.h"
        assert hasattr(handle, s), f"{s} not exported by libdvg_hip.so"
        assert s in _lib.SIGNATURES
    assert _lib.lib().dvg_abi_version() == 9        # additions within ABI 9
    txt = open(os.path.join(os.path.dirname(HERE), "include", "dvg_hip.h")).read()
    for line in ("lstm.py:84,101", "lstm.py:116,133"):      # every entry point names the reference line it replaces
        assert line in txt


def test_host_side_checks_reject_before_any_launch():
    """H = 100, an in-place state update, a misaligned pointer, no incoming gradient: refused on the host (fake pointers, never
    dereferenced; no GPU here, so a launch would fail differently)."""
    from dvg_amd import _lib
    lib = _lib.lib()
    SHAPE_ERR, NULL_ERR = 1, 2
    a, b, c, odd = (ctypes.c_void_p(v) for v in (1024, 2048, 4096, 1028))
    # dvg_gru_cell(x, h, w_ih, w_hh, b_ih, b_hh, h_out, acts_out, B, H, stream)
    assert lib.dvg_gru_cell(a, b, a, a, a, a, c, None, 4, 100, None) == SHAPE_ERR and b"multiple of 64" in lib.dvg_last_error()
    assert lib.dvg_gru_cell(a, b, a, a, a, a, b, None, 4, 64, None) == SHAPE_ERR and b"in-place" in lib.dvg_last_error()
    assert lib.dvg_gru_cell(a, b, a, a, a, a, a, None, 4, 64, None) == SHAPE_ERR and b"in-place" in lib.dvg_last_error()
    rc = lib.dvg_gru_cell(odd, b, a, a, a, a, c, None, 4, 64, None)
    assert rc not in (0, SHAPE_ERR, NULL_ERR) and b"alignment" in lib.dvg_last_error()
    assert lib.dvg_gru_cell(a, b, a, a, a, None, c, None, 4, 64, None) == NULL_ERR
    # dvg_gru_cell_pre(pre, h, w_hh, b_hn, h_out, acts_out, B, H, stream)
    assert lib.dvg_gru_cell_pre(a, b, a, a, c, None, 4, 100, None) == SHAPE_ERR
    assert lib.dvg_gru_cell_pre(a, b, a, a, b, None, 4, 64, None) == SHAPE_ERR and b"in-place" in lib.dvg_last_error()
    assert lib.dvg_gru_cell_pre(a, odd, a, a, c, None, 4, 64, None) not in (0, SHAPE_ERR, NULL_ERR)
    # dvg_rnn_cell(x, h, w_ih, w_hh, b_ih, b_hh, h_out, B, H, stream)
    assert lib.dvg_rnn_cell(a, b, a, a, a, a, c, 4, 100, None) == SHAPE_ERR
    assert lib.dvg_rnn_cell(a, b, a, a, a, a, b, 4, 64, None) == SHAPE_ERR and b"in-place" in lib.dvg_last_error()
    assert lib.dvg_rnn_cell(a, b, odd, a, a, a, c, 4, 64, None) not in (0, SHAPE_ERR, NULL_ERR)
    # dvg_gru_gates_bwd(dh_a, dh_b, acts, h_prev, dGi, dGh, dh_prev, B, H, stream)
    assert lib.dvg_gru_gates_bwd(None, None, a, None, b, c, None, 4, 64, None) == NULL_ERR
    assert b"no incoming gradient" in lib.dvg_last_error()
    assert lib.dvg_gru_gates_bwd(a, None, a, None, b, c, odd, 4, 64, None) not in (0, SHAPE_ERR, NULL_ERR)
    assert lib.dvg_gru_gates_bwd(a, None, a, None, b, b, None, 4, 64, None) == SHAPE_ERR
    # the wrappers refuse host tensors and bad shapes as their neighbours do
    from dvg_amd import ops
    t = torch.zeros(4, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gru_cell(t, t, torch.zeros(192, 64), torch.zeros(192, 64), torch.zeros(192), torch.zeros(192))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rnn_cell(t, t, torch.zeros(64, 64), torch.zeros(64, 64), torch.zeros(64), torch.zeros(64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gru_cell_pre(torch.zeros(4, 192), t, torch.zeros(192, 64), torch.zeros(64), torch.zeros(4, 64), None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gru_gates_bwd(t, None, torch.zeros(4, 256), None)
    with pytest.raises(RuntimeError, match="no incoming gradient"):
        ops.gru_gates_bwd(None, None, torch.zeros(4, 256), None)


@pytest.mark.parametrize("kind", ["gru", "rnn"])
def test_reference_pickles_load_into_our_classes(kind):
    """A model.pth whose frame_predictor was pickled as the reference's models.lstm.gru / .rnn (train.py:380-388 stores whole
    modules) unpickles into this repository's classes through the top-level `models.lstm`."""
    import dvg_amd.models.lstm as ours
    raw = gzip.open(os.path.join(HERE, "golden", "reference_pickled_gru.pth.gz")).read()
    fx = torch.load(io.BytesIO(raw), weights_only=False)[kind]
    net = fx["module"]
    assert type(net) is getattr(ours, kind) and type(net).__module__ == "dvg_amd.models.lstm"
    assert list(net.state_dict().keys()) == fx["keys"] == list(getattr(ours, kind)(*fx["shape"], fx["batch"]).state_dict().keys())
    cells = getattr(net, kind)
    assert len(cells) == 2 and isinstance(cells[0], torch.nn.GRUCell if kind == "gru" else torch.nn.RNNCell)
    assert len(net.hidden) == 2 and all(torch.is_tensor(h) and h.shape == (fx["batch"], 64) for h in net.hidden)
    assert len(net.state_tensors()) == 2
    net.set_state_tensors(net.init_hidden())
    assert ours.sequence_applies(net) == (kind == "gru")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(fx["batch"], 90))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.step_state_only(torch.zeros(fx["batch"], 90))


def test_every_predictor_hands_its_state_over_as_a_flat_list():
    import dvg_amd.models.lstm as ours
    for cls, per_layer in ((ours.lstm, 2), (ours.gaussian_lstm, 2), (ours.gru, 1), (ours.rnn, 1)):
        net = cls(90, 90, 64, 3, 4)
        st = net.state_tensors()
        assert len(st) == 3 * per_layer == net.n_layers * net.state_per_layer and all(torch.is_tensor(t) for t in st)
        marks = [torch.full((4, 64), float(i)) for i in range(len(st))]
        net.set_state_tensors(marks)
        assert all(a is b for a, b in zip(net.state_tensors(), marks))
        if per_layer == 2:
            assert all(isinstance(hc, tuple) and hc[0] is marks[2 * l] and hc[1] is marks[2 * l + 1] for l, hc in enumerate(net.hidden))
        else:
            assert all(h is m for h, m in zip(net.hidden, marks))


def test_the_flag_parses_and_an_unknown_kind_is_refused(capsys):
    import generate_frames
    import train
    assert train.options([]).predictor == "lstm"
    for kind in ("lstm", "gru", "rnn"):
        assert train.options(["--predictor", kind]).predictor == kind
        assert generate_frames.build_parser().parse_args(["--predictor", kind]).predictor == kind
    with pytest.raises(SystemExit):
        train.options(["--predictor", "gaussian_gru"])
    assert "--predictor" in capsys.readouterr().err
    import argparse
    import dvg_amd.models.lstm as ours
    opt = argparse.Namespace(model="dcgan", image_width=64, g_dim=90, channels=1, rnn_size=64, predictor_rnn_layers=2,
                             batch_size=4, predictor="gru")
    assert isinstance(generate_frames.synthetic_checkpoint(opt)["frame_predictor"], ours.gru)
    opt.predictor = "rnn"
    assert isinstance(generate_frames.synthetic_checkpoint(opt)["frame_predictor"], ours.rnn)
    del opt.predictor
    assert isinstance(generate_frames.synthetic_checkpoint(opt)["frame_predictor"], ours.lstm)


def test_resume_fingerprint_carries_the_predictor():
    """A state without the field is an `lstm` state: an lstm run accepts it (and writes the fingerprint it always did), a gru run
    refuses it naming the field; so does an lstm run handed a gru state."""
    import train
    from dvg_amd import train_state
    plain, gru = train.options([]), train.options(["--predictor", "gru"])
    old = train_state.option_fingerprint(plain)
    assert "predictor" not in old and old == train_state.option_fingerprint(train.options(["--predictor", "lstm"]))
    new = train_state.option_fingerprint(gru)
    assert new["predictor"] == "gru" and {k: v for k, v in new.items() if k != "predictor"} == old
    train_state.check_fingerprint(old, train_state.option_fingerprint(plain), "<state>")      # no SystemExit
    train_state.check_fingerprint(new, train_state.option_fingerprint(gru), "<state>")
    with pytest.raises(SystemExit, match=r"predictor is 'lstm' in the file and 'gru' in this run"):
        train_state.check_fingerprint(old, new, "<state>")
    with pytest.raises(SystemExit, match=r"predictor is 'gru' in the file and 'lstm' in this run"):
        train_state.check_fingerprint(new, old, "<state>")
    with pytest.raises(SystemExit, match=r"predictor is 'gru' in the file and 'rnn' in this run"):
        train_state.check_fingerprint(new, train_state.option_fingerprint(train.options(["--predictor", "rnn"])), "<state>")
    train_state.check_fingerprint(new, {"world": 1}, "<state>")   # a partial fingerprint: its fields only
