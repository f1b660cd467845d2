"""Host-side proof for tests/test_gpu_dense.py: the fp64 references of tests/dense_ref.py agree with fp64 autograd, the recorded
kernel / split count of every gemm_nt case agrees with dvg_gemm_nt_bias_act's dispatch recomputed from its source text,
torch's fp32 arithmetic is inside every bar and every planted defect outside it, and the cap condition of the cell bars holds
at every case (docs/DESIGN_NOTES_dense_tests.md)."""
import os
import re

import pytest
import torch

from tests import dense_ref as dr
from tests.backward_ref import YARDSTICK_RATIO, sum_bound
from tests.common import ROOT


# ---- the references against fp64 autograd -----------------------------------------------------------------------------
def _consistent_step(B, H, zero_cprev):
    """fp32-rounded saved gates and c' (what the kernels read) with an fp64 c_prev and fp64 pre-activations that reproduce
    them exactly: pre = logit / atanh of the gates, c_prev = (c' - i g) / f (zero_cprev: c' is replaced by i g instead, which
    is then not an fp32 number - the formulas do not care)."""
    dh_a, dh_b, dc, gates, c_prev, c_new, w_hh = dr.bwd_inputs(B, H)
    g64 = gates.double()
    i, f, g, o = (g64[:, k * H:(k + 1) * H] for k in range(4))
    if zero_cprev:
        c_prev64, c_new64 = None, i * g
    else:
        c_new64 = c_new.double()
        c_prev64 = (c_new64 - i * g) / f
    pre = torch.cat([torch.logit(i), torch.logit(f), torch.atanh(g), torch.logit(o)], 1)
    return dh_a.double(), dh_b.double(), dc.double(), g64, c_prev64, c_new64, w_hh.double(), pre


@pytest.mark.parametrize("use_a,use_b,use_dc", [(True, True, True), (True, False, False), (False, False, True), (True, False, True)])
@pytest.mark.parametrize("zero_cprev", [False, True])
def test_backward_references_agree_with_fp64_autograd(use_a, use_b, use_dc, zero_cprev):
    B, H = 5, 64
    dh_a, dh_b, dc, gates, c_prev, c_new, w_hh, pre = _consistent_step(B, H, zero_cprev)
    # forward reference as a function of (h, c_prev) with the pre-activations passing through `pre` at h0
    h0 = dr.cell_inputs(B, H)[1].double()
    hleaf = h0.clone().requires_grad_(True)
    cleaf = (torch.zeros(B, H, dtype=torch.float64) if c_prev is None else c_prev.clone()).requires_grad_(True)
    x_half = (pre - h0 @ w_hh.t()).detach().requires_grad_(True)
    fwd = dr.lstm_cell_ref(None, hleaf, cleaf, None, w_hh, None, None, x_half=x_half)
    assert float((fwd["gates"].detach() - gates).abs().max()) < 1e-14
    assert float((fwd["c"].detach() - c_new).abs().max()) < 1e-14
    dh = (dh_a if use_a else 0) + (dh_b if use_b else 0)
    loss = (fwd["h"] * dh).sum() + ((fwd["c"] * dc).sum() if use_dc else 0)
    loss.backward()
    dG, dcp, dhp, _ = dr.lstm_cell_bwd_ref(dh_a if use_a else None, dh_b if use_b else None, dc if use_dc else None, gates,
                                           c_prev, c_new, w_hh)
    dG2, dcp2 = dr.lstm_gates_bwd_ref(dh if (use_a or use_b) else None, dc if use_dc else None, gates, c_prev, c_new)
    assert torch.equal(dG, dG2) and torch.equal(dcp, dcp2)
    for got, want in ((dG, x_half.grad), (dcp, cleaf.grad), (dhp, hleaf.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_forward_reference_is_nn_lstmcell():
    B, H = 5, 64
    ops = dr.cell_inputs(B, H)
    cell = torch.nn.LSTMCell(H, H).double()
    with torch.no_grad():
        for p, v in zip((cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh), ops[3:]):
            p.copy_(v.double())
        h2, c2 = cell(ops[0].double(), (ops[1].double(), ops[2].double()))
    ref = dr.lstm_cell_ref(*(t.double() for t in ops))
    assert float((ref["h"] - h2).abs().max()) < 1e-14 and float((ref["c"] - c2).abs().max()) < 1e-14
    # the `pre` form and the folded first cell state the same function
    x, h, c, w_ih, w_hh, b_ih, b_hh = (t.double() for t in ops)
    pre = dr.lstm_cell_ref(None, h, c, None, w_hh, None, None, x_half=x @ w_ih.t() + b_ih + b_hh)
    assert float((pre["gates"] - ref["gates"]).abs().max()) < 1e-14
    xo = tuple(t.double() for t in dr.cell_x_inputs(5, 64, 90))
    unfolded = dr.lstm_cell_x_ref(*xo)
    wx, bias = dr.fold_x(xo[3], xo[4], xo[5], xo[7], xo[8], 92)
    assert wx.shape == (256, 92) and wx.dtype == torch.float32 and bool((wx[:, 90:] == 0).all())
    folded = torch.sigmoid((xo[0] @ wx.double()[:, :90].t() + bias.double() + xo[1] @ xo[6].t())[:, :64])
    assert float((folded - unfolded["gates"][:, :64]).abs().max()) < 1e-6


# ---- the dispatch ---------------------------------------------------------------------------------------------------------
def test_case_table_agrees_with_the_dispatch():
    for case in dr.GEMM_CASES:
        kernel, splits, kper = dr.case_dispatch(case)
        assert (kernel, splits) == (case["kernel"], case["splits"]), (case["name"], kernel, splits, kper)
    by = dr.GEMM_BY_NAME
    assert dr.case_dispatch(by["2x2112x200-s3"])[2] == 96 and dr.case_dispatch(by["8x8x520-s3"])[2] == 256
    assert dr.case_dispatch(by["130x33x1001-s4"])[2] == 256 and dr.case_dispatch(by["130x2049x40-s2"])[2] == 32
    # every kernel, with and without a split; the reduce kernel's unrolled trip with and without its tail, and its stride loop
    reached = {(c["kernel"], c["splits"] > 1) for c in dr.GEMM_CASES}
    assert reached >= {("dot_vec", False), ("dot_vec", True), ("dot_scalar", False), ("dot_scalar", True), ("tile_vec", False),
                       ("tile_vec", True), ("tile_scalar", False)}
    assert {c["splits"] for c in dr.GEMM_CASES} >= {32, 11, 3, 2}
    assert any(c["splits"] > 1 and c["M"] * c["N"] > 4096 * 64 for c in dr.GEMM_CASES)
    assert all(name in by and by[name]["N"] % p == 0 and p < by[name]["N"] for name, p in dr.EPILOGUE_CASES.items())
    assert {by[n]["kernel"] for n in dr.EPILOGUE_CASES} == {"dot_vec", "dot_scalar", "tile_scalar"}


def test_dispatch_recomputation_reads_like_the_source():
    """The constants dispatch() rests on, read from dense.hip: a retuned dispatch fails here, not as lost coverage."""
    with open(os.path.join(ROOT, "dvg_amd", "csrc", "dense.hip")) as f:
        src = f.read()
    body = src[src.index('extern "C" int dvg_gemm_nt_bias_act'):src.index('extern "C" int dvg_gemm_tn')]
    flat = re.sub(r"\s+", " ", body)
    assert "if (M <= 1024 && N <= 2048)" in flat
    assert "int kper = (K + splitk - 1) / splitk; kper = ((kper + 31) / 32) * 32;" in flat
    assert "kper = (((K + splitk - 1) / splitk + 255) / 256) * 256;" in flat
    assert flat.count("p.splitk = (K + kper - 1) / kper;") == 2
    assert "p.vec = (K % 4 == 0 && aligned16(w)) ? 1 : 0;" in flat
    assert "p.vec_a = (K % 4 == 0 && lda % 4 == 0 && aligned16(a)) ? 1 : 0;" in flat
    assert "(total + 63) / 64 > 4096 ? 4096" in flat


# ---- products: torch's fp32 inside the derived bound, the planted defects outside ----------------------------------------------
@pytest.mark.parametrize("name", dr.GEMM_NAMES)
def test_product_bound_separates_fp32_from_the_defects(name):
    case = dr.GEMM_BY_NAME[name]
    a, w = dr.gemm_inputs(case)
    ref, mag = dr.gemm_nt_ref(a, w)
    kernel, splits, kper = dr.case_dispatch(case)
    bound = dr.gamma(dr.case_depth(case))
    e32 = dr.elem_err(a @ w.t(), ref, mag)
    assert e32 <= bound, (name, e32, bound)
    applied = 0
    for kind in dr.PRODUCT_DEFECTS:
        try:
            bad = dr.plant_product(kind, a, w, kper, splits)
        except ValueError:
            continue
        applied += 1
        e = dr.elem_err(bad, ref, mag)
        assert e > 2 * bound, (name, kind, e, bound)
    assert applied >= 1
    for kind in ("lane_slice", "split_tail", "row_clamp", "col_clamp"):
        applies = {"lane_slice": case["K"] >= 256, "split_tail": splits > 1, "row_clamp": case["M"] % 8 >= 2,
                   "col_clamp": case["N"] % 8 >= 2}[kind]
        if not applies:
            with pytest.raises(ValueError):
                dr.plant_product(kind, a, w, kper, splits)


@pytest.mark.parametrize("name", list(dr.EPILOGUE_CASES))
def test_epilogue_allowance_separates_fp32_from_the_defects(name):
    case, period = dr.GEMM_BY_NAME[name], dr.EPILOGUE_CASES[name]
    a, w = dr.gemm_inputs(case)
    u = a @ w.t()                                     # stands for the kernel's own raw product
    sc, sh, base = epilogue_operands(case, period)
    idx = torch.arange(case["N"]) % period
    for act in dr.ACTS:
        v32 = u * sc[idx] + sh[idx]
        f = {dr.ACT_NONE: lambda t: t, dr.ACT_LRELU: lambda t: torch.nn.functional.leaky_relu(t, 0.2), dr.ACT_TANH: torch.tanh,
             dr.ACT_SIGMOID: torch.sigmoid}[act]
        ulps = dr.act_ulps_allowed(v32, act) if act in (dr.ACT_TANH, dr.ACT_SIGMOID) else 0.0
        for b in (None, base):
            got = f(v32) if b is None else f(v32) + b
            ref, mag = dr.epilogue_ref(u, sc, sh, period, act, 0.2, b)
            allow = dr.epilogue_allowance(ref, mag, act, b, ulps)
            assert bool(((got.double() - ref).abs() <= allow).all()), (name, act, b is not None)
            for defect in dr.EPILOGUE_DEFECTS:
                if defect == "no_accumulate" and b is None:
                    with pytest.raises(ValueError):
                        dr.epilogue_ref(u, sc, sh, period, act, 0.2, b, defect)
                    continue
                bad, _ = dr.epilogue_ref(u, sc, sh, period, act, 0.2, b, defect)
                assert bool(((bad - ref).abs() > 2 * allow).any()), (name, act, defect)
    with pytest.raises(ValueError):
        dr.epilogue_ref(u, sc, sh, case["N"], dr.ACT_NONE, defect="period")


def epilogue_operands(case, period):
    from oracle import params
    k = dr.GEMM_CASES.index(case)
    return (1 + 0.1 * params.normal(9400 + k, period), 0.1 * params.normal(9450 + k, period),
            params.normal(9480 + k, case["M"], case["N"]))


@pytest.mark.parametrize("R,M,N", dr.GEMM_TN_CASES + [dr.GEMM_TN_STRIDED])
def test_gemm_tn_bound(R, M, N):
    from oracle import params
    a, b = params.normal(570, R, M), params.normal(571, R, N)
    ref, mag, cs, csmag = dr.gemm_tn_ref(a, b)
    bound = dr.gamma(dr.gemm_tn_depth(R))
    assert dr.elem_err(a.t() @ b, ref, mag) <= bound
    assert bool(((a.sum(0).double() - cs).abs() <= sum_bound(csmag, R)).all())
    assert dr.elem_err(dr.plant_product("k_last", a.t(), b.t()), ref, mag) > 2 * bound       # the last row dropped


@pytest.mark.parametrize("KP,K,M,N,period", dr.STEM_CASES)
def test_stem_bound(KP, K, M, N, period):
    vec, w = dr.stem_inputs(KP, K, M, N)
    ref, mag = dr.gemm_nt_ref(vec, w)
    bound = dr.gamma(dr.stem_depth(KP))
    assert dr.elem_err(vec @ w.t(), ref, mag) <= bound
    assert dr.elem_err(dr.plant_product("k_last", vec, w), ref, mag) > 2 * bound
    if M % 8 >= 2:
        assert dr.elem_err(dr.plant_product("row_clamp", vec, w), ref, mag) > 2 * bound


# ---- cells: the bar condition, fp32 inside, defects outside -------------------------------------------------------------------
def _check_bars(f, bars, worst, label):
    plant = min(f["plants"].values())
    for o, e32 in f["e32"].items():
        assert max(YARDSTICK_RATIO * f["e_y"][o], worst[o]) <= 0.5 * plant, (label, o, f["e_y"][o], worst[o], plant)   # the cap condition
        assert e32 <= f["e_y"][o] <= bars[o], (label, o)                                           # torch's fp32 is inside
    for d, e in f["plants"].items():
        assert e > max(bars.values()), (label, d, e, bars)      # its worst output is beyond every output's bar


@pytest.mark.parametrize("kind", ["cell", "pre", "x"])
def test_forward_cell_bars(kind):
    seen = set()
    for key in dr.cell_keys(kind):
        f = dr.cell_figures(kind, key)
        _check_bars(f, dr.cell_bars(kind, key), dr.cell_worst_e32(kind), (kind, key))
        seen |= set(f["plants"])
        B, H = (dr.SAT_CASE if key == "sat" else key)[:2]
        want = {"gate_order", "k_tail"} | ({"bias_once"} if kind != "pre" else set()) | ({"slice2"} if H > 256 else set()) \
            | ({"row_clamp"} if B % 8 >= 2 else set()) | ({"c_stale"} if B - 8 * ((B - 1) // 8) >= 2 else set()) \
            | ({"x_tail"} if kind == "x" else set())
        assert set(f["plants"]) == want, (kind, key, set(f["plants"]), want)
        assert min(f["plants"].values()) >= 4e-2, (kind, key, f["plants"])
    want_all = set(dr.FORWARD_DEFECTS) - ({"x_tail"} if kind != "x" else {"slice2"}) - ({"bias_once"} if kind == "pre" else set())
    assert seen == want_all, (kind, seen)


def test_the_yardstick_is_torch_fp32_and_the_ordered_emulation_states_the_same_cell():
    """Torch's fp32 is the yardstick at every case; the kernel-order emulation (printed beside the kernel's error at the
    saturated case) states the same function: fp32 noise away from fp64 at an ordinary case, reproducible bit for bit.  The
    saturated case's pre-activations are what the case list says."""
    for kind in ("cell", "pre", "x"):
        for key in dr.cell_keys(kind):
            f = dr.cell_figures(kind, key)
            assert f["e_y"] == f["e32"] and ("e_ord" in f) == ((kind, key) in dr.ORDERED_INFO)
    ops = dr.cell_inputs(21, 256)
    em, ref = dr.lstm_cell_ordered(*ops), dr.cell_figures("cell", (21, 256))["ref"]
    assert max(dr.block_err(em[o], ref[o]) for o in ("h", "c")) < 2e-6
    assert max(dr.block_err(v, ref[o]) for o, v in dr.gate_slices(em["gates"]).items()) < 2e-6
    assert torch.equal(dr.lstm_cell_ordered(*ops)["pre"], em["pre"])
    sat = dr.cell_figures("cell", "sat")
    pre64 = dr.lstm_cell_ref(*(t.double() for t in dr.cell_inputs(*dr.SAT_CASE, sat=True)))["pre"].abs().amax(1)
    assert 35 < float(pre64[1]) < 50 and 85 < float(pre64[9]) < 120 and float(pre64[[0, 2, 3, 4, 5, 6, 7, 8]].max()) < 5
    assert max(sat["e_y"].values()) < 1e-5 < 4e-2 <= min(sat["plants"].values())


def test_backward_bars():
    seen = set()
    for key in dr.bwd_case_list():
        f = dr.bwd_figures(*key)
        _check_bars(f, dr.bwd_bars(*key), dr.bwd_worst_e32(), key)
        seen |= set(f["plants"])
        B, H, use_a, use_b, use_dc, use_cprev, with_dhp = key
        want = {"f_prev"} | ({"tanh_c"} if use_a or use_b else set()) | ({"no_dc"} if use_dc else set()) \
            | ({"no_dh_b"} if use_b else set()) | ({"whh_plain"} if with_dhp else set()) | ({"null_cprev"} if not use_cprev else set())
        assert set(f["plants"]) == want, (key, set(f["plants"]), want)
    assert seen == set(dr.BACKWARD_DEFECTS)


def test_dh_prev_bound_rejects_the_untransposed_weight():
    B, H = 21, 256
    dh_a, dh_b, dc, gates, c_prev, c_new, w_hh = (t.double() for t in dr.bwd_inputs(B, H))
    dG, _, dhp, mag = dr.lstm_cell_bwd_ref(dh_a, dh_b, dc, gates, c_prev, c_new, w_hh)
    bound = dr.gamma(dr.LSTM_BWD_DEPTH)
    assert dr.elem_err(dG.float() @ w_hh.float(), dhp, mag) <= bound
    bad = dr.lstm_cell_bwd_ref(dh_a, dh_b, dc, gates, c_prev, c_new, w_hh, "whh_plain")[2]
    assert dr.elem_err(bad, dhp, mag) > 2 * bound


def test_measures_do_not_dilute():
    ref = torch.ones(40, 64, dtype=torch.float64) * 100
    ref[32:, 10:12] = 0.01
    got = ref.clone()
    got[39, 11] += 0.001
    assert abs(dr.block_err(got, ref) - 0.1) < 1e-9                 # against its own block, not the tensor's 100
    got[0, 0] = float("nan")
    assert dr.block_err(got, ref) == float("inf")
    assert dr.elem_err(torch.tensor([[1.0, 0.0]]), torch.tensor([[1.0, 0.0]]), torch.tensor([[2.0, 0.0]])) == 0.0
    assert dr.elem_err(torch.tensor([[1.0, 1e-9]]), torch.tensor([[1.0, 0.0]]), torch.tensor([[2.0, 0.0]])) == float("inf")
    assert dr.gamma(10) == sum_bound(1.0, 11)
