"""GPU: the dense kernels of dvg_amd/csrc/dense.hip (and dvg_lstm_gates_bwd) against the fp64 restatements of tests/dense_ref.py,
wave by wave: every kernel dvg_gemm_nt_bias_act dispatches to (with and without split K, strided, misaligned, accumulating), its
epilogue apart from the product, dvg_gemm_tn, dvg_stem_gemm, the three LSTM forward cells with their saved gates, and the two LSTM
backward kernels.  Measures, bars and planted defects: tests/dense_ref.py; that the bars separate torch's fp32 from every planted
defect: tests/test_dense_ref_host.py; the table of figures: docs/DESIGN_NOTES_dense_tests.md."""
import pytest
import torch

from oracle import params
from tests import dense_ref as dr
from tests.backward_ref import sum_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL, POISON = 7.0, 1e30
ERR_SHAPE, ERR_NULL, ERR_ALIGN = 1, 2, 4          # DVG_ERR_* of include/dvg_hip.h


def dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def offset_view(t, off):
    """t's values in a device buffer whose base lies `off` floats past a 16-byte boundary."""
    flat = torch.full((t.numel() + 8,), POISON, device=DEV)
    v = flat[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
    return v


def column_slice(t, ld, fill):
    """(buffer (rows, ld) filled with `fill`, its column slice that holds t), the slice starting (ld - width) // 2 columns in."""
    rows, width = t.shape
    big = torch.full((rows, ld), fill, device=DEV)
    c0 = (ld - width) // 2
    big[:, c0:c0 + width] = t.to(DEV)
    return big, big[:, c0:c0 + width]


def untouched(big, view_cols, fill=SENTINEL):
    """Every column of `big` outside the slice still holds the fill value."""
    c0 = (big.shape[1] - view_cols) // 2
    return bool((big[:, :c0] == fill).all()) and bool((big[:, c0 + view_cols:] == fill).all())


# ---- gemm_nt: the raw product --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dr.GEMM_NAMES)
def test_gemm_nt_product(name):
    from dvg_amd import ops
    case = dr.GEMM_BY_NAME[name]
    M, N, K = case["M"], case["N"], case["K"]
    a, w = dr.gemm_inputs(case)
    ref, mag = dr.gemm_nt_ref(a, w)
    if case["lda"]:
        a_big, ad = column_slice(a, case["lda"], POISON)
        assert ad.data_ptr() % 16 == 0 and ad.stride(0) == case["lda"]
    else:
        ad = offset_view(a, case["a_off"])
    wd = offset_view(w, case["w_off"])
    depth = dr.case_depth(case)
    for acc in case["accumulate"]:
        base = params.normal(9300, M, N) if acc else torch.full((M, N), SENTINEL)
        big, out = column_slice(base, case["ldo"] or N, SENTINEL)
        ret = ops.gemm_nt(ad, wd, None, None, splitk=case["splitk"], out=out, accumulate=acc)
        assert ret is out
        want, wmag, bound = (ref + base.double(), mag + base.double().abs(), dr.gamma(depth + 1)) if acc else \
            (ref, mag, dr.gamma(depth))
        e = dr.elem_err(out, want, wmag)
        e32 = dr.elem_err(a @ w.t(), ref, mag)
        print(f"\ngemm_nt {name} acc={acc}: {case['kernel']} splits {case['splits']} d {depth} bound {bound:.2e} "
              f"e_hip {e:.2e} e32 {e32:.2e}")
        assert e <= bound, (name, acc, e, bound)
        assert untouched(big, N)
        big2, out2 = column_slice(base, case["ldo"] or N, SENTINEL)
        ops.gemm_nt(ad, wd, None, None, splitk=case["splitk"], out=out2, accumulate=acc)
        assert torch.equal(big2, big)


# ---- gemm_nt: the epilogue, from the kernel's own raw product --------------------------------------------------------------
@pytest.mark.parametrize("name", list(dr.EPILOGUE_CASES))
def test_gemm_nt_epilogue(name):
    from dvg_amd import ops
    case, period = dr.GEMM_BY_NAME[name], dr.EPILOGUE_CASES[name]
    k = dr.GEMM_CASES.index(case)
    a, w = dr.gemm_inputs(case)
    sc, sh = 1 + 0.1 * params.normal(9400 + k, period), 0.1 * params.normal(9450 + k, period)
    base = params.normal(9480 + k, case["M"], case["N"])
    ad, wd, scd, shd = dev(a, w, sc, sh)
    u = ops.gemm_nt(ad, wd, None, None, splitk=case["splitk"])
    assert torch.equal(u, ops.gemm_nt(ad, wd, None, None, splitk=case["splitk"]))      # what makes the own raw u usable
    u = u.cpu()
    idx = torch.arange(case["N"]) % period
    runs = [(act, True, True, False) for act in dr.ACTS] + [(dr.ACT_LRELU, False, True, False), (dr.ACT_LRELU, True, False, False),
                                                             (dr.ACT_LRELU, False, False, False), (dr.ACT_NONE, False, False, True)]
    runs += [(act, True, True, True) for act in dr.ACTS]
    for act, use_sc, use_sh, acc in runs:
        s, t = (sc if use_sc else None), (sh if use_sh else None)
        out = base.to(DEV) if acc else None
        y = ops.gemm_nt(ad, wd, scd if use_sc else None, shd if use_sh else None, act=act, slope=0.2, period=period,
                        splitk=case["splitk"], out=out, accumulate=acc)
        ref, mag = dr.epilogue_ref(u, s, t, period, act, 0.2, base if acc else None)
        ulps = 0.0
        if act in (dr.ACT_TANH, dr.ACT_SIGMOID):
            v32 = u * sc[idx] + sh[idx]                                          # two roundings
            vfma = (u.double() * sc.double()[idx] + sh.double()[idx]).float()     # one
            t_ulps, ulps = dr.torch_act_ulps(v32, act), dr.act_ulps_allowed(v32, act)
            if not acc:       # the device function's own error: against fp64 on whichever fp32 input (fma or not) it is closer to
                f = torch.tanh if act == dr.ACT_TANH else torch.sigmoid
                yy = y.cpu().double()
                k_ulps = float(torch.minimum(*[(yy - f(v.double())).abs() / dr.ulp32(f(v.double())) for v in (v32, vfma)]).max())
                print(f"\nepilogue {name} act={act}: torch {t_ulps:.2f} ulp, kernel {k_ulps:.2f} ulp, allowed {ulps:.2f}")
        allow = dr.epilogue_allowance(ref, mag, act, base if acc else None, ulps)
        worst = float(((y.cpu().double() - ref).abs() / allow.clamp_min(1e-300)).max())
        assert worst <= 1.0, (name, act, use_sc, use_sh, acc, worst)


# ---- gemm_tn ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,M,N", dr.GEMM_TN_CASES)
def test_gemm_tn_elementwise(R, M, N):
    from dvg_amd import ops
    assert ops.GEMM_TN_MAX_ROWS == dr.GEMM_TN_MAX_ROWS
    a, b = params.normal(570, R + 3, M)[3:], params.normal(571, R + 3, N)[3:]
    ref, mag, cs, csmag = dr.gemm_tn_ref(a, b)
    ad, bd = params.normal(570, R + 3, M).to(DEV)[3:], params.normal(571, R + 3, N).to(DEV)[3:]
    d = dr.gemm_tn_depth(R)
    out = ops.gemm_tn(ad, bd)
    e = dr.elem_err(out, ref, mag)
    print(f"\ngemm_tn ({R}, {M}, {N}): d {d} bound {dr.gamma(d):.2e} e_hip {e:.2e} e32 {dr.elem_err(a.t() @ b, ref, mag):.2e}")
    assert out.shape == (M, N) and e <= dr.gamma(d), (e, dr.gamma(d))
    assert torch.equal(out, ops.gemm_tn(ad, bd))
    # accumulate into existing buffers, column sums into two sinks (the R > GEMM_TN_MAX_ROWS fallback included)
    base, c0, c1 = params.normal(572, M, N), params.normal(573, M), params.normal(574, M)
    o2, k0, k1 = dev(base, c0, c1)
    assert ops.gemm_tn(ad, bd, out=o2, accumulate=True, colsums=(k0, None, k1)) is o2
    ea = dr.elem_err(o2, ref + base.double(), mag + base.double().abs())
    assert ea <= dr.gamma(d + 1), (ea, dr.gamma(d + 1))
    for got, c in ((k0, c0), (k1, c1)):
        assert bool(((got.cpu().double() - (cs + c.double())).abs() <= sum_bound(csmag + c.double().abs(), R + 1)).all())
    k2 = torch.full((M,), SENTINEL, device=DEV)
    ops.gemm_tn(ad, bd, out=o2, colsums=(k2,), colsum_accumulate=False)
    assert torch.equal(o2, out)
    assert bool(((k2.cpu().double() - cs).abs() <= sum_bound(csmag, R)).all())


def test_gemm_tn_strided_operands():
    from dvg_amd import ops
    R, M, N = dr.GEMM_TN_STRIDED
    a, b = params.normal(575, R, M), params.normal(576, R, N)
    ref, mag, cs, csmag = dr.gemm_tn_ref(a, b)
    (a_big, ad), (b_big, bd) = column_slice(a, M + 6, POISON), column_slice(b, N + 8, POISON)
    big, out = column_slice(torch.full((M, N), SENTINEL), N + 4, SENTINEL)
    k0 = torch.full((M,), SENTINEL, device=DEV)
    ops.gemm_tn(ad, bd, out=out, colsums=(k0,), colsum_accumulate=False)
    e = dr.elem_err(out, ref, mag)
    print(f"\ngemm_tn strided ({R}, {M}, {N}): e_hip {e:.2e} bound {dr.gamma(R):.2e}")
    assert e <= dr.gamma(dr.gemm_tn_depth(R)) and untouched(big, N)
    assert bool(((k0.cpu().double() - cs).abs() <= sum_bound(csmag, R)).all())
    big2, out2 = column_slice(torch.full((M, N), SENTINEL), N + 4, SENTINEL)
    ops.gemm_tn(ad, bd, out=out2)
    assert torch.equal(big2, big)


# ---- the decoder stem ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("KP,K,M,N,period", dr.STEM_CASES)
def test_stem_gemm(KP, K, M, N, period):
    from dvg_amd import ops
    vec, w = dr.stem_inputs(KP, K, M, N)
    ref, mag = dr.gemm_nt_ref(vec, w)
    wt = torch.zeros(KP, N)
    wt[:K] = w.t()                                    # rows K .. KP - 1 zero: the kernel's contract
    wtd = wt.to(DEV)
    vec_big, vd = column_slice(vec, K + 6, POISON)
    sc, sh = 1 + 0.1 * params.normal(9600 + M, period), 0.1 * params.normal(9601 + M, period)

    def run(s, t, act):
        big, out = column_slice(torch.full((M, N), SENTINEL), N + 64, SENTINEL)
        assert ops.stem_gemm(vd, wtd, K, s, t, out, period=period, act=act, slope=0.2) is out
        assert untouched(big, N)
        return big, out
    big, u = run(None, None, ops.ACT_NONE)
    d = dr.stem_depth(KP)
    e = dr.elem_err(u, ref, mag)
    print(f"\nstem ({KP}, {K}, {M}, {N}): d {d} bound {dr.gamma(d):.2e} e_hip {e:.2e} e32 {dr.elem_err(vec @ w.t(), ref, mag):.2e}")
    assert e <= dr.gamma(d), (e, dr.gamma(d))
    assert torch.equal(run(None, None, ops.ACT_NONE)[0], big)
    _, y = run(*dev(sc, sh), ops.ACT_LRELU)
    eref, emag = dr.epilogue_ref(u, sc, sh, period, dr.ACT_LRELU, 0.2)
    allow = dr.epilogue_allowance(eref, emag, dr.ACT_LRELU)
    assert bool(((y.cpu().double() - eref).abs() <= allow).all())


# ---- the LSTM forward cells ---------------------------------------------------------------------------------------------------
def raw_lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh, h_out, c_out, gates):
    from dvg_amd._lib import check, lib
    B, H = h.shape
    check(lib().dvg_lstm_cell(x.data_ptr(), h.data_ptr(), c.data_ptr(), w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(),
                              b_hh.data_ptr(), h_out.data_ptr(), c_out.data_ptr(), None if gates is None else gates.data_ptr(),
                              B, H, torch.cuda.current_stream().cuda_stream), "lstm_cell")


def row_slices(B, widths):
    """Per width, (a (3B, width) buffer of sentinels, its middle B rows)."""
    bigs = [torch.full((3 * B, wd), SENTINEL, device=DEV) for wd in widths]
    return bigs, [b[B:2 * B] for b in bigs]


def rows_untouched(bigs, B):
    return all(bool((b[:B] == SENTINEL).all()) and bool((b[2 * B:] == SENTINEL).all()) for b in bigs)


def hold_cell(label, got, kind, key):
    fig, bars = dr.cell_figures(kind, key), dr.cell_bars(kind, key)
    line, bad = [], []
    for o, ref in fig["ref"].items():
        assert bool(torch.isfinite(got[o]).all()), (label, o)
        e = dr.block_err(got[o], ref)
        line.append(f"{o} {e:.2e}/{fig['e32'][o]:.2e}/{bars[o]:.2e}" + (f" (ordered {fig['e_ord'][o]:.2e})" if "e_ord" in fig else ""))
        if not e <= bars[o]:
            bad.append((o, e, bars[o]))
    print(f"\n{label} {key} (e_hip/e32/bar; smallest plant {min(fig['plants'].values()):.2e}): " + "  ".join(line))
    assert not bad, (label, key, bad)


@pytest.mark.parametrize("key", dr.cell_keys("cell"), ids=str)
def test_lstm_cell_and_pre_against_fp64(key):
    from dvg_amd import ops
    B, H = dr.SAT_CASE if key == "sat" else key
    cpu = dr.cell_inputs(B, H, sat=key == "sat")
    x, h, c, w_ih, w_hh, b_ih, b_hh = dev(*cpu)
    bigs, (ho, co, go) = row_slices(B, (H, H, 4 * H))
    raw_lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh, ho, co, go)
    assert rows_untouched(bigs, B)
    hold_cell("lstm_cell", {"h": ho, "c": co, **dr.gate_slices(go)}, "cell", key)
    h2, c2, g2 = ops.lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh, want_gates=True)
    assert torch.equal(h2, ho) and torch.equal(c2, co) and torch.equal(g2, go)               # two calls
    h3, c3 = ops.lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh)
    assert torch.equal(h3, ho) and torch.equal(c3, co)                                       # want_gates=False
    # the `pre` form: its operand computed in fp64 and rounded once
    c64 = [t.double() for t in cpu]
    pre = (c64[0] @ c64[3].t() + c64[5] + c64[6]).float().to(DEV)
    bigs, (hp, cp, gp) = row_slices(B, (H, H, 4 * H))
    ops.lstm_cell_pre(pre, h, c, w_hh, hp, cp, gp)
    assert rows_untouched(bigs, B)
    hold_cell("lstm_cell_pre", {"h": hp, "c": cp, **dr.gate_slices(gp)}, "pre", key)
    bigs2, (hq, cq, gq) = row_slices(B, (H, H, 4 * H))
    ops.lstm_cell_pre(pre, h, c, w_hh, hq, cq, gq)
    assert all(torch.equal(u, v) for u, v in zip(bigs, bigs2))
    bigs3, (hr, cr, _) = row_slices(B, (H, H, 4 * H))
    ops.lstm_cell_pre(pre, h, c, w_hh, hr, cr, None)
    assert torch.equal(hr, hp) and torch.equal(cr, cp)


@pytest.mark.parametrize("key", dr.CELL_X_CASES, ids=str)
def test_lstm_cell_x_against_fp64(key):
    from dvg_amd import ops
    B, H, Kx, Kxp, ldx = key
    cpu = dr.cell_x_inputs(B, H, Kx)
    x, h, c, w_e, b_e, w_ih, w_hh, b_ih, b_hh = cpu
    wx, bias = dr.fold_x(w_e, b_e, w_ih, b_ih, b_hh, Kxp)
    x_big = torch.full((B, ldx), POISON, device=DEV)       # a stray read beyond Kx would show up
    x_big[:, :Kx] = x.to(DEV)
    xd = x_big[:, :Kx]
    hd, cd, wxd, whd, bd = dev(h, c, wx, w_hh, bias)
    h2, c2 = ops.lstm_cell_x(xd, hd, cd, wxd, whd, bd)
    hold_cell("lstm_cell_x", {"h": h2, "c": c2}, "x", key)
    h3, c3 = ops.lstm_cell_x(xd, hd, cd, wxd, whd, bd)
    assert torch.equal(h3, h2) and torch.equal(c3, c2)
    # into slices of larger buffers
    from dvg_amd._lib import check, lib
    bigs, (ho, co) = row_slices(B, (H, H))
    check(lib().dvg_lstm_cell_x(xd.data_ptr(), ldx, Kx, hd.data_ptr(), cd.data_ptr(), wxd.data_ptr(), Kxp, whd.data_ptr(),
                                bd.data_ptr(), ho.data_ptr(), co.data_ptr(), B, H, torch.cuda.current_stream().cuda_stream), "x")
    assert torch.equal(ho, h2) and torch.equal(co, c2) and rows_untouched(bigs, B)


# ---- the LSTM backward kernels ------------------------------------------------------------------------------------------------
def hold_bwd(label, got, key):
    fig, bars = dr.bwd_figures(*key), dr.bwd_bars(*key)
    line, bad = [], []
    for o, e32 in fig["e32"].items():
        e = dr.block_err(got[o], fig["ref"][o], 8, 4)
        line.append(f"{o} {e:.2e}/{e32:.2e}/{bars[o]:.2e}")
        if not e <= bars[o]:
            bad.append((o, e, bars[o]))
    print(f"\n{label} {key} (e_hip/e32/bar; smallest plant {min(fig['plants'].values()):.2e}): " + "  ".join(line))
    assert not bad, (label, key, bad)


@pytest.mark.parametrize("B,H", dr.GATES_BWD_CASES)
def test_lstm_gates_bwd_against_fp64(B, H):
    from dvg_amd import ops
    dh, _, dc, gates, c_prev, c_new, _ = dev(*dr.bwd_inputs(B, H))
    for use_dh, use_dc in ((True, False), (False, True), (True, True)):
        dG, dcp = ops.lstm_gates_bwd(dh if use_dh else None, dc if use_dc else None, gates, c_prev, c_new)
        hold_bwd("lstm_gates_bwd", {**{"d" + k: v for k, v in dr.gate_slices(dG).items()}, "dc_prev": dcp},
                 (B, H, use_dh, False, use_dc, True, False))
        again = ops.lstm_gates_bwd(dh if use_dh else None, dc if use_dc else None, gates, c_prev, c_new)
        assert torch.equal(again[0], dG) and torch.equal(again[1], dcp)


@pytest.mark.parametrize("B", dr.CELL_BWD_BATCHES)
def test_lstm_cell_bwd_against_fp64(B):
    from dvg_amd import ops
    H = 256
    dh_a, dh_b, dc, gates, c_prev, c_new, w_hh = dev(*dr.bwd_inputs(B, H))
    gates0, c_new0 = dev(*dr.bwd_inputs_zero_state(B, H))
    w_hh_t = w_hh.t().contiguous()
    w64 = w_hh.double().cpu()
    for name, use_b, use_dc, use_cp, want_dhp in dr.CELL_BWD_COMBOS:
        g, cn = (gates, c_new) if use_cp else (gates0, c_new0)

        def run(cp):
            bigs, (dG, dcp, dhp) = row_slices(B, (4 * H, H, H))
            ops.lstm_cell_bwd(dh_a, dh_b if use_b else None, dc if use_dc else None, g, cp, cn, w_hh_t, dG, dcp,
                              dhp if want_dhp else None)
            assert rows_untouched(bigs, B)
            return bigs, dG, dcp, dhp
        bigs, dG, dcp, dhp = run(c_prev if use_cp else None)
        hold_bwd(f"lstm_cell_bwd {name}", {**{"d" + k: v for k, v in dr.gate_slices(dG).items()}, "dc_prev": dcp},
                 (B, H, True, use_b, use_dc, use_cp, want_dhp))
        if want_dhp:      # the product, from the kernel's own dG
            ref, mag = dG.double().cpu() @ w64, dG.double().cpu().abs() @ w64.abs()
            e, bound = dr.elem_err(dhp, ref, mag), dr.gamma(dr.LSTM_BWD_DEPTH)
            print(f"lstm_cell_bwd {name} B={B} dh_prev: e_hip {e:.2e} bound {bound:.2e} "
                  f"e32 {dr.elem_err(dG.cpu() @ w_hh.cpu(), ref, mag):.2e}")
            assert e <= bound, (name, e, bound)
        else:
            assert bool((bigs[2] == SENTINEL).all())
        assert all(torch.equal(u, v) for u, v in zip(run(c_prev if use_cp else None)[0], bigs))          # two calls
        if not use_cp:    # NULL c_prev == explicit zeros, bit for bit
            assert all(torch.equal(u, v) for u, v in zip(run(torch.zeros_like(c_prev))[0], bigs))


# ---- rejections: return codes checked before any launch ---------------------------------------------------------------
def test_rejections_before_any_launch():
    from dvg_amd._lib import lib
    L = lib()
    buf = torch.zeros(1 << 20, device=DEV)
    p = [buf.data_ptr() + 4 * 65536 * i for i in range(12)]      # distinct, 16-byte aligned, inside the buffer
    for H in (96, 100):
        assert L.dvg_lstm_cell(*p[:9], None, 4, H, None) == ERR_SHAPE
        assert L.dvg_lstm_cell_pre(*p[:6], None, 4, H, None) == ERR_SHAPE
        assert L.dvg_lstm_cell_x(p[0], 90, 90, p[1], p[2], p[3], 92, p[4], p[5], p[6], p[7], 4, H, None) == ERR_SHAPE
    for H in (128, 512):
        assert L.dvg_lstm_cell_bwd(*p[:10], 4, H, None) == ERR_SHAPE
    for kx, ldx, kxp in ((89, 90, 92), (130, 130, 132), (90, 89, 92), (90, 91, 92), (90, 90, 88), (90, 90, 90)):
        assert L.dvg_lstm_cell_x(p[0], ldx, kx, p[1], p[2], p[3], kxp, p[4], p[5], p[6], p[7], 4, 64, None) == ERR_SHAPE, (kx, ldx, kxp)
    # in-place state updates
    assert L.dvg_lstm_cell(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[1], p[8], None, 4, 64, None) == ERR_SHAPE     # h_out == h
    assert L.dvg_lstm_cell(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[2], None, 4, 64, None) == ERR_SHAPE     # c_out == c
    assert L.dvg_lstm_cell_pre(p[0], p[1], p[2], p[3], p[1], p[5], None, 4, 64, None) == ERR_SHAPE
    assert L.dvg_lstm_cell_x(p[0], 90, 90, p[1], p[2], p[3], 92, p[4], p[5], p[1], p[7], 4, 64, None) == ERR_SHAPE
    # alignment
    assert L.dvg_lstm_cell(p[0] + 4, *p[1:9], None, 4, 64, None) == ERR_ALIGN
    assert L.dvg_lstm_cell(p[0], p[1] + 4, *p[2:9], None, 4, 64, None) == ERR_ALIGN
    assert L.dvg_lstm_cell_x(p[0] + 4, 90, 90, p[1], p[2], p[3], 92, p[4], p[5], p[6], p[7], 4, 64, None) == ERR_ALIGN
    assert L.dvg_lstm_cell_bwd(p[0] + 4, *p[1:10], 4, 256, None) == ERR_ALIGN
    # gemm_nt: split K without a workspace, bad period; gemm_tn: a second column-sum sink without the first
    assert L.dvg_gemm_nt_bias_act(p[0], p[1], None, None, p[2], None, 8, 8, 512, 512, 8, 8, 2, 0, 0.0, 0, None) == ERR_NULL
    assert L.dvg_gemm_nt_bias_act(p[0], p[1], None, None, p[2], None, 8, 8, 512, 512, 8, 3, 1, 0, 0.0, 0, None) == ERR_SHAPE
    assert L.dvg_gemm_nt_bias_act(p[0], p[1], None, None, p[2], None, 8, 8, 512, 500, 8, 8, 1, 0, 0.0, 0, None) == ERR_SHAPE
    assert L.dvg_gemm_tn(p[0], p[1], p[2], None, p[3], 8, 8, 8, 8, 8, 8, 0, 0, None) == ERR_NULL
    assert L.dvg_stem_gemm(p[0], 90, p[1], 112, None, None, p[2], 32, 4, 32, 90, 32, 0, 0.0, None) == ERR_SHAPE    # KP
    torch.cuda.synchronize()
    assert bool((buf == 0).all())                      # nothing ran


def test_lstm_wrappers_validate_their_buffers():
    """ops.lstm_cell_pre / ops.lstm_cell_bwd refuse wrong shapes on the host side (a (B, 3H) `pre` used to be read out of bounds);
    nothing is launched."""
    from dvg_amd import ops
    B, H = 4, 64
    z = lambda *s: torch.zeros(*s, device=DEV)                                                # noqa: E731
    pre, h, c, w_hh, ho, co, go = z(B, 4 * H), z(B, H), z(B, H), z(4 * H, H), z(B, H), z(B, H), z(B, 4 * H)
    bad_calls = [(z(B, 3 * H), h, c, w_hh, ho, co, go), (z(B, 8 * H)[:, :4 * H], h, c, w_hh, ho, co, go),
                 (pre, h, z(B + 1, H), w_hh, ho, co, go), (pre, h, c, z(4 * H, H + 4), ho, co, go),
                 (pre, h, c, w_hh, z(B, 2 * H)[:, :H], co, go), (pre, h, c, w_hh, ho, z(B, H + 4), go),
                 (pre, h, c, w_hh, ho, co, z(B, 3 * H)), (pre.cpu(), h, c, w_hh, ho, co, go), (pre.double(), h, c, w_hh, ho, co, go)]
    for args in bad_calls:
        with pytest.raises(RuntimeError):
            ops.lstm_cell_pre(*args)
    assert bool((ho == 0).all()) and bool((go == 0).all())
    H = 256
    dh, gates, cn, wt, dG, dcp, dhp = z(B, H), z(B, 4 * H), z(B, H), z(H, 4 * H), z(B, 4 * H), z(B, H), z(B, H)
    good = dict(dh_a=dh, dh_b=None, dc=None, gates=gates, c_prev=None, c_new=cn, w_hh_t=wt, dG=dG, dc_prev=dcp, dh_prev=dhp)
    for k, v in (("dh_a", z(B, H + 4)), ("dh_b", z(B + 1, H)), ("dc", z(B, 2 * H)[:, :H]), ("gates", z(B, 3 * H)),
                 ("c_prev", z(B + 1, H)), ("w_hh_t", z(4 * H, H)), ("dG", z(B, 3 * H)), ("dc_prev", z(B, 2 * H)[:, :H]),
                 ("dh_prev", z(B, H + 4)), ("gates", gates.cpu()), ("dh_a", None)):
        with pytest.raises(RuntimeError):
            ops.lstm_cell_bwd(**{**good, k: v})
    assert bool((dG == 0).all()) and bool((dhp == 0).all())
