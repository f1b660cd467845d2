"""CPU: the references, bounds, bars and planted defects of tests/winograd_ref.py hold what the GPU tests
(tests/test_gpu_winograd_stages.py, tests/test_gpu_wino_wgrad.py) rely on - the packed-row codec is exact, the vectorised
transform references agree with explicit loops over the tiles, a plain fp32 evaluation of every transform lies within its derived
bound, every case reaches the dispatch edge it was chosen for (dvg_gemm_batched_plan, dvg_winograd_transform_width,
dvg_winograd_wgrad_splits), and each bar passes its yardstick and rejects every planted defect
(docs/DESIGN_NOTES_winograd_tests.md)."""
import pytest
import torch

from oracle import params
from tests import winograd_ref as wr
from tests.backward_ref import YARDSTICK_RATIO
from tests.forward_ref import ENERGY, LATENCY


def _lib():
    from dvg_amd import _lib
    return _lib.lib()


def _x3():
    return _lib().dvg_mfma_mode() == 1


# ---- packed rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [16, 24])
@pytest.mark.parametrize("cout,cin", [(64, 16), (64, 48), (128, 16), (128, 48)])
def test_packed_rows_round_trip_bit_for_bit(cout, cin, row):
    u = params.normal(9600 + cout + cin, 3, cin, cout)
    packed = wr.pack_rows(u, row)
    assert packed.shape == (3, cout // 64, cin // 16, 64, row) and packed.dtype == torch.float32
    back = wr.unpack_rows(packed, 3, cin, cout, row)
    assert torch.equal(back.view(torch.int32), u.view(torch.int32))


def test_packed_rows_layout_from_the_writers_index_formula():
    """wrow_store_pair, spelled out per element: row ((xi cb_n + cb) chunks + chunk) 64 + co % 64, plane j at bf16 slots
    [16 j, 16 j + 16), value k at slot ((k >> 3) ^ ((co % 64 >> 3) & 1)) 8 + k % 8."""
    cin, cout = 32, 128
    u = params.normal(9650, 2, cin, cout)
    bits = wr.pack_rows(u, 24).reshape(-1, 24).view(torch.int16).reshape(-1, 48)
    h = u.bfloat16()
    for xi, ci, co in [(0, 0, 0), (1, 5, 8), (0, 17, 77), (1, 31, 127), (1, 8, 72), (0, 15, 15)]:
        row = ((xi * (cout // 64) + co // 64) * (cin // 16) + ci // 16) * 64 + co % 64
        k = ci % 16
        slot = (((k >> 3) ^ ((co % 64 >> 3) & 1)) << 3) + (k & 7)
        assert bits[row, slot] == h[xi, ci, co].view(torch.int16), (xi, ci, co)
    plain = wr.pack_rows(u, 16).reshape(-1, 16)
    assert plain[((1 * 2 + 1) * 2 + 1) * 64 + 63, 15] == u[1, 31, 127]


# ---- the transform references against explicit loops -----------------------------------------------------------------------
@pytest.mark.parametrize("m,up", [(2, False), (4, False), (4, True)])
def test_input_reference_tile_order_halo_and_layout(m, up):
    """2 images, a non-square map, 4 channels: the unfold-based reference equals the loop written from the kernel's index
    formulas, so a layout mistake in the reference cannot cancel against the same mistake in the code that reads it."""
    x = params.normal(9610 + m + up, 2, 4 if up else 8, 6 if up else 12, 4)
    v, bound = wr.input_ref(x, m, up)
    loop = wr.input_ref_loop(x, m, up)
    assert v.shape == loop.shape and float((v - loop).abs().max()) <= 1e-13
    assert bool((bound > 0).any())


def test_output_and_dy_references_against_explicit_loops():
    n, h, w, c = 2, 8, 12, 4
    for m in (2, 4):
        e, t = m + 2, n * (h // m) * (w // m)
        mm = params.normal(9620 + m, e * e, t, c)
        y, _ = wr.output_ref(mm, n, h, w, m)
        for i, ty, tx in [(0, 0, 0), (1, h // m - 1, w // m - 1), (1, 0, 1)]:
            q = mm[:, (i * (h // m) + ty) * (w // m) + tx].double().reshape(e, e, c)
            o = torch.einsum("pa,abc,qb->pqc", wr.AT[m], q, wr.AT[m])
            assert float((y[i, m * ty:m * ty + m, m * tx:m * tx + m] - o).abs().max()) <= 1e-13
    dy = params.normal(9625, n, h, w, c)
    dm, _ = wr.dy_ref(dy)
    for i, ty, tx in [(0, 0, 0), (1, 1, 2)]:
        d = dy[i, 4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4].double()
        o = torch.einsum("ap,pqc,bq->abc", wr.A4, d, wr.A4)
        assert float((dm[:, (i * 2 + ty) * 3 + tx] - o.reshape(36, c)).abs().max()) <= 1e-13


def test_transform_pairs_are_adjoint_and_the_whole_is_a_convolution():
    """A^T [(G g G^T) . (B^T d B)] A is the 3 x 3 convolution, and dy_ref / reduce_ref are its adjoints: the references compose
    to torch's fp64 conv2d and to its weight gradient."""
    import torch.nn.functional as F
    n, h, w, cin, cout = 2, 8, 12, 4, 4
    x, wt, dy = params.normal(9630, n, h, w, cin), params.normal(9631, cout, cin, 3, 3), params.normal(9632, n, h, w, cout)
    for m in (2, 4):
        u, _ = wr.weight_ref(wt, m)
        v, _ = wr.input_ref(x, m)
        y, _ = wr.output_ref(torch.einsum("ptc,pco->pto", v, u), n, h, w, m)
        ref = F.conv2d(x.double().permute(0, 3, 1, 2), wt.double(), None, 1, 1).permute(0, 2, 3, 1)
        assert float((y - ref).abs().max()) <= 1e-12
    dm, _ = wr.dy_ref(dy)
    v, _ = wr.input_ref(x, 4)
    part = torch.einsum("pto,ptc->poc", dm, v).reshape(1, 36, cout, cin)
    dg, _ = wr.reduce_ref(part)
    xx = x.double().permute(0, 3, 1, 2)
    w0 = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    (F.conv2d(xx, w0, None, 1, 1) * dy.double().permute(0, 3, 1, 2)).sum().backward()
    assert float((dg - w0.grad.permute(2, 3, 0, 1).reshape(9, cout, cin)).abs().max()) <= 1e-11


# ---- a plain fp32 evaluation lies within every derived bound -----------------------------------------------------------------
def _fp32_two_sided(t1, x, t2):
    """Two 1-D passes in fp32 with fp32 matrices: every product and every sum rounds, which is at least as many roundings as
    the kernels' hand-written passes make wherever a matrix row has a non-trivial entry - not a proof of the count, a check
    that the bound has the right order of magnitude and no missing factor."""
    a = torch.einsum("ia,...ab->...ib", t1.float(), x.float())
    return torch.einsum("...ib,jb->...ij", a, t2.float())


def test_bounds_hold_for_plain_fp32_and_reject_a_wrong_matrix_entry():
    x = params.normal(9640, 3, 8, 12, 20)
    for m in (2, 4):
        v, bound = wr.input_ref(x, m)
        p = wr._patches(x, m, False)
        v32 = _fp32_two_sided(wr.BT[m], p, wr.BT[m]).permute(2, 3, 0, 1).reshape(v.shape)
        ex, ratio = wr.excess(v32, v, bound)
        print(f"input m={m}: fp32 / bound {ratio:.2f}")
        assert ex <= 0
        bad = wr.BT[m].clone()
        bad[1, 2] *= 1 + 2.0 ** -18          # one entry off by 4e-6
        vb = torch.einsum("ia,...ab,jb->...ij", bad, p, wr.BT[m]).permute(2, 3, 0, 1).reshape(v.shape)
        assert wr.excess(vb, v, bound)[0] > 0
    wt = params.normal(9641, 8, 16, 3, 3)
    for m in (2, 4):
        u, bound = wr.weight_ref(wt, m)
        u32 = _fp32_two_sided(wr.G[m], wt, wr.G[m]).permute(2, 3, 1, 0).reshape(u.shape)
        ex, ratio = wr.excess(u32, u, bound)
        print(f"weight m={m}: fp32 / bound {ratio:.2f}")
        assert ex <= 0


# ---- the width query --------------------------------------------------------------------------------------------------------
def test_transform_width_query_states_the_rule():
    """tiles * C / 4 >= 1024 * 256 -> 4, else tiles * C / 2 >= 1024 * 256 -> 2, else 1: the shapes the GPU tests run the wider
    forms at are the smallest that reach them."""
    lib = _lib()
    for tiles, c, want in [(2048, 256, 2), (2047, 256, 1), (4096, 256, 4), (4095, 256, 2), (8192, 128, 4), (8191, 128, 2),
                           (1, 4, 1), (1 << 20, 4, 4), (3 * 6, 20, 1)]:
        assert lib.dvg_winograd_transform_width(tiles, c) == want, (tiles, c)
    assert lib.dvg_winograd_transform_width(0, 64) == 0 and lib.dvg_winograd_transform_width(64, 6) == 0
    for (n, h, w, c), width in wr.WIDE_SHAPES:
        assert lib.dvg_winograd_transform_width(n * (h // 4) * (w // 4), c) == width, (n, h, w, c)


# ---- the batched GEMM -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wr.GEMM_NAMES)
def test_gemm_cases_reach_the_edge_they_were_chosen_for(name):
    """Every case's (tile width, Cout blocks per workgroup, images per pipeline) against dvg_gemm_batched_plan, so that a
    retuned threshold fails here instead of silently un-covering an edge; for the threshold cases also that the next smaller
    launch does NOT take the variant (the case is the smallest that does)."""
    lib, case = _lib(), wr.GEMM_BY_NAME[name]
    plan = wr.gemm_plan(lib, case)
    assert plan == wr.expected_plan(case, _x3()), (name, plan)
    assert lib.dvg_tile_policy() == LATENCY
    if not _x3():
        return
    nb, h, w, cin, cout = case["shape"]
    smaller = dict(case, shape=(nb, h - 8, w, cin, cout))
    if name in ("ni2", "ni3", "rows128-k64", "nt2", "nt2-o256"):
        assert wr.gemm_plan(lib, smaller) == (8, 1, 1), (name, wr.gemm_plan(lib, smaller))
    if name in ("nt2", "nt2-o256"):
        assert wr.gemm_plan(lib, dict(case, policy=LATENCY)) == (8, 1, 1)


def test_gemm_plan_rejects_what_the_launcher_rejects():
    import ctypes
    lib = _lib()
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    r = [ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)]
    assert lib.dvg_gemm_batched_plan(1, 8, 8, 64, 64, *r) == 0 and (a.value, b.value, c.value) == (8, 1, 1)
    assert lib.dvg_gemm_batched_plan(1, 8, 8, 48, 64, *r) == -1          # Cin % 64
    assert lib.dvg_gemm_batched_plan(1, 8, 12, 64, 64, *r) == -1         # W % 8
    assert lib.dvg_gemm_batched_plan(1, 8, 8, 64, 96, *r) == -1          # Cout % 64
    assert lib.dvg_gemm_batched_plan(1, 8, 8, 64, 64, None, None, None) == -1


@pytest.mark.parametrize("name", wr.GEMM_NAMES)
def test_gemm_bar_passes_the_yardstick_and_rejects_every_planted_defect(name):
    x3 = _x3()
    case = wr.GEMM_BY_NAME[name]
    plan = wr.expected_plan(case, x3)
    f, b = wr.gemm_figures(name, x3), wr.gemm_bar(name, x3)
    print(f"{name} plan {plan}: e32 {f['e32']:.2e} e_emu {f.get('e_emu', float('nan')):.2e} e_plane_x {f['e_plane_x']:.2e} "
          f"e_plane_u {f['e_plane_u']:.2e} worst {wr.gemm_worst(x3):.2e} bar {b:.2e}")
    # the cap is a condition, not a clamp
    assert max(wr.yardstick_ratio(x3) * f["e_y"], wr.gemm_worst(x3)) <= 0.5 * f["e_plane"], (name, f["e_y"], f["e_plane"])
    assert f["e_y"] <= b
    x, u = wr.gemm_inputs(name)
    ref = wr.gemm_ref(x, u)
    applied = []
    for kind in wr.GEMM_PLANTS:
        try:
            y = wr.gemm_plant(kind, x, u, plan, x3)
        except ValueError:
            continue
        e = wr.gemm_err(y, ref, plan)
        applied.append(kind)
        assert e > b, (name, kind, e, b)
    assert {"plane_x", "plane_u", "slab"} <= set(applied)
    assert ("wrap" in applied) == (plan[2] > 1) and ("half" in applied) == (plan[1] == 2)


def test_gemm_blockwise_error_sees_one_bad_block_and_nan():
    ref = wr.gemm_ref(*wr.gemm_inputs("three-stages"))
    a = ref.clone()
    a[2, 0:8, 8:16, 64:128] *= 1 + 1e-4
    blocks = wr.gemm_blocks(a, ref, (8, 1, 1))
    assert blocks.shape == (3, 1, 2, 2) and int((blocks > 0).sum()) == 1 and float(blocks[2, 0, 1, 1]) > 5e-5
    a[0, 0, 0, 0] = float("nan")
    assert wr.gemm_err(a, ref, (8, 1, 1)) == float("inf")


# ---- the Winograd-form weight gradient --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wr.WGEMM_NAMES)
def test_wgrad_gemm_cases_have_the_plan_they_were_chosen_for(name):
    """ww_plan restated in Python gives every case its (stages per block, stages per workgroup, workgroups, slabs), and the
    library's dvg_winograd_wgrad_splits agrees on S."""
    c = wr.WGEMM_BY_NAME[name]
    pl = wr.ww_plan(c["tp"], c["cin"], c["cout"])
    assert (pl["nst"], pl["q"], pl["wgs"], pl["S"]) == c["plan"], (name, pl)
    assert _lib().dvg_winograd_wgrad_splits(c["tp"], c["cin"], c["cout"]) == pl["S"]
    if name == "whole-blocks":
        assert set(pl["segs"]) == {1} and pl["q"] == 4 * pl["nst"]
    if name == "cut-blocks":
        assert set(pl["segs"]) == {1, 2}          # the uncut blocks are the ones whose slab 1 is zero-filled
    if name == "short-tail":
        assert pl["total"] == 4896 and pl["short"] == 4 and max(pl["segs"]) == 5
    if name.startswith("items"):
        per_item = c["t_item"] // 32          # a workgroup's q stages start inside one item and end inside another
        assert per_item < pl["q"]


@pytest.mark.parametrize("name", wr.WGEMM_NAMES)
def test_wgrad_gemm_bar_passes_fp32_and_rejects_every_planted_defect(name):
    from tests.backward_ref import blockwise_err
    x3 = _x3()
    f, b = wr.wgemm_figures(name), wr.wgemm_bar(name, x3)
    print(f"{name}: e32 {f['e32']:.2e} e_plane {f['e_plane']:.2e} worst {wr.wgemm_worst():.2e} bar {b:.2e}")
    assert max(wr.yardstick_ratio(x3) * f["e32"], wr.wgemm_worst()) <= 0.5 * f["e_plane"], (name, f)
    assert f["e32"] <= b
    ref = wr.wgemm_ref(*wr.wgemm_inputs(name))
    applied = []
    for kind in wr.WGEMM_PLANTS:
        try:
            p = wr.wgemm_plant(kind, name)
        except ValueError:
            continue
        applied.append(kind)
        assert blockwise_err(p, ref) > b, (name, kind)
    assert {"plane", "pos"} <= set(applied)
    assert ("segment" in applied) == (wr.WGEMM_BY_NAME[name]["plan"][3] > 1) and ("item" in applied) == name.startswith("items")


def test_reduce_reference_bound_holds_for_plain_fp32():
    part = params.normal(9660, 3, 36, 4, 12)
    ref, bound = wr.reduce_ref(part)
    t = part.float().sum(0).reshape(6, 6, 4, 12).permute(2, 3, 0, 1)
    got = _fp32_two_sided(wr.GT4, t, wr.GT4).permute(2, 3, 0, 1).reshape(9, 4, 12)
    ex, ratio = wr.excess(got, ref, bound)
    print(f"reduce: fp32 / bound {ratio:.2f}")
    assert ex <= 0


# ---- the forward end to end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(wr.FWD_E2E)), ids=wr.FWD_E2E_IDS)
def test_forward_end_to_end_bar_rejects_a_lost_plane(k):
    """The fp32 Winograd form passes its own bar, a lost plane of V or of U in the GEMM - seen through the output transform -
    fails it, and the cap never bites; the shapes are ones ops.winograd_ok admits with exactly 128 tiles."""
    from dvg_amd.ops.winograd import winograd_ok
    m, n, h, cin, cout, _, _ = wr.FWD_E2E[k]
    assert winograd_ok(n, cin, h, h, cout, m) and n * (h // m) ** 2 == 128
    f, b = wr.fwd_e2e_figures(k), wr.fwd_e2e_bar(k)
    print(f"{wr.FWD_E2E_IDS[k]}: e32 {f['e32']:.2e} e_plane_v {f['e_plane_v']:.2e} e_plane_u {f['e_plane_u']:.2e} "
          f"worst {wr.fwd_e2e_worst(m):.2e} bar {b:.2e}")
    assert max(YARDSTICK_RATIO * f["e32"], wr.fwd_e2e_worst(m)) <= 0.5 * f["e_plane"], (k, f)
    assert f["e32"] <= b < f["e_plane"]


def test_forward_end_to_end_error_is_per_gemm_tile():
    ref = wr.fwd_e2e_ref(2)
    a = ref.clone()
    a[0, 0:4, 0:4, :64] *= 1 + 1e-3          # Winograd tile 0 of image 0 at m = 4: one block
    assert wr.fwd_e2e_err(a, ref, 4) > 1e-4
    a = ref.clone()
    a[0, 0, 0, 0] = float("nan")
    assert wr.fwd_e2e_err(a, ref, 4) == float("inf")


# ---- the weight gradient end to end -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(wr.WGRAD_E2E)), ids=wr.WGRAD_E2E_IDS)
def test_wgrad_end_to_end_bar_passes_fp32_and_rejects_lost_planes_and_wrapper_defects(k):
    """The fp32 Winograd form passes its own bar; a lost plane of dM or of V - the operands wino_wgrad_gemm_x3_kernel splits -
    seen through G^T . G fails it and the cap never bites; so do an item's V at the wrong tile offset and padding rows that
    are not zero.  d out itself rounded to 16 bits is NOT separable from the fp32 form end to end (the notes' finding): printed."""
    from tests.backward_ref import MODE_CONV3, blockwise_err, wgrad_ref
    n, h, cin, cout, items, _ = wr.WGRAD_E2E[k]
    f, b = wr.wgrad_e2e_figures(k), wr.wgrad_e2e_bar(k)
    print(f"{wr.WGRAD_E2E_IDS[k]}: e32 {f['e32']:.2e} e_plane_v {f['e_plane_v']:.2e} e_plane_dm {f['e_plane_dm']:.2e} "
          f"(d out to 16 bits {f['e_plane_dout']:.2e}) worst {wr.wgrad_e2e_worst():.2e} bar {b:.2e}")
    assert max(YARDSTICK_RATIO * f["e32"], wr.wgrad_e2e_worst()) <= 0.5 * f["e_plane"], (k, f)
    assert f["e32"] <= b < f["e_plane"]
    xs, dus = wr.wgrad_e2e_inputs(k)
    ref = wgrad_ref(MODE_CONV3, xs, None, dus)
    t = n * (h // 4) ** 2
    applied = []
    for kind in wr.WGRAD_E2E_PLANTS:
        try:
            p = wr.wgrad_winograd_form(xs, dus, torch.float64, plant=kind)
        except ValueError:
            continue
        applied.append(kind)
        assert blockwise_err(p, ref) > b, (k, kind)
    assert ("t_off" in applied) == (items > 1) and ("pad" in applied) == ((items * t) % 64 != 0)
    slabs = _lib().dvg_winograd_wgrad_splits(-(-items * t // 64) * 64, cin, cout)
    assert slabs == wr.ww_plan(-(-items * t // 64) * 64, cin, cout)["S"] and (slabs > 2) == (n == 9)
