"""Every stage of the Winograd forward (dvg_amd/csrc/winograd.hip and the batched GEMM mode of conv_igemm2.hip) against an fp64
reference of THAT STAGE ALONE on the kernel's own inputs, at the smallest shapes that reach each code path: the packed weight
rows, the weight / input / d(out) / output transforms within rounding bounds derived from their code (nothing measured), the
F(4x4) transforms' f32x2 and f32x4 forms, and dvg_gemm_batched_k16 workgroup tile by workgroup tile under the bar of
docs/DESIGN_NOTES_winograd_tests.md at every tile and pipeline variant.  tests/test_winograd_ref_host.py shows on the CPU that
the references are laid out as the kernels lay their tensors out, that the bar rejects every planted defect and that each case
still reaches the dispatch edge it was chosen for."""
import pytest
import torch

from oracle import params
from tests import winograd_ref as wr
from tests.common import dev

pytestmark = pytest.mark.gpu

_ops, _lib, _call, _nan, _untouched, _report = wr.gpu_ops, wr.gpu_lib, wr.gpu_call, wr.nan_filled, wr.untouched, wr.report


def _row():
    return int(_lib().dvg_packed_row_floats())


# ---- packed rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", [16, 48])
def test_unpack_rows_decodes_what_pack_igemm_weight_writes(cin):
    """The decoder against a kernel that does not belong to the family under test: at Cout = 64 the 1 x 1 layout
    [Cin/16][Cout/64][1][64][row] of pack_k16_kernel IS [1][Cout/64][Cin/16][64][row]."""
    w = params.normal(9800 + cin, 64, cin, 1, 1)
    packed = _ops().pack_igemm_weight(w.to(dev()))
    u = wr.unpack_rows(packed, 1, cin, 64, _row())
    assert torch.equal(u[0].view(torch.int32), w[:, :, 0, 0].t().contiguous().view(torch.int32))


# ---- the weight transform ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout,cin", [(64, 16), (128, 48)])
@pytest.mark.parametrize("m", [2, 4])
def test_weight_transform(m, cout, cin):
    """U = G g G^T within gamma_(2 k) |G| |g| |G|^T, and the corners that are copies: F(4x4) position (5, 5) is g[2][2] bit for
    bit (rows of exact zeros there are the failure wrow_owner_note describes) and (0, 0) is g[0][0] / 16 exactly; F(2x2)
    positions (0, 0) and (3, 3) are g[0][0] and g[2][2]."""
    w = params.normal(9810 + m + cout, cout, cin, 3, 3)
    packed = _ops().winograd_weight(w.to(dev()), m)
    torch.cuda.synchronize()
    e = (m + 2) ** 2
    u = wr.unpack_rows(packed, e, cin, cout, _row())
    ref, bound = wr.weight_ref(w, m)
    _report(f"weight m={m} {cout}x{cin}", u, ref, bound)
    g00, g22 = w[:, :, 0, 0].t().contiguous(), w[:, :, 2, 2].t().contiguous()
    assert torch.equal(u[e - 1].view(torch.int32), g22.view(torch.int32))
    assert torch.equal(u[0], g00 / 16 if m == 4 else g00)


# ---- the input transform ----------------------------------------------------------------------------------------------------
INPUT_CASES = [(2, (1, 2, 2, 4), False), (2, (2, 6, 10, 12), False), (4, (1, 4, 4, 4), False), (4, (3, 8, 12, 20), False),
               (4, (2, 4, 4, 8), True), (4, (1, 4, 8, 12), True)]


@pytest.mark.parametrize("m,shape,up", INPUT_CASES, ids=[f"m{m}-{'x'.join(map(str, s))}{'-up' if u else ''}" for m, s, u in INPUT_CASES])
def test_input_transform(m, shape, up):
    """V = B^T d B of x (stored shape; read through the x2 upsampling when `up`) within gamma_(2 k) |B^T| |d| |B|."""
    n, hs, ws, c = shape
    h, w = (2 * hs, 2 * ws) if up else (hs, ws)
    x = params.normal(9820 + sum(shape), *shape)
    ref, bound = wr.input_ref(x, m, up)
    v = _nan(*ref.shape)
    if m == 4:
        assert _lib().dvg_winograd_transform_width(n * (h // 4) * (w // 4), c) == 1
    _call(_lib().dvg_winograd_input, x.to(dev()), v, n, h, w, c, m, int(up))
    _report(f"input m={m} {shape} up={up}", v, ref, bound)


@pytest.mark.parametrize("items", [2, 3])
def test_wgrad_operands_at_tile_offsets(items):
    """dvg_winograd_wgrad_operands writes item i's tiles at t_off = i t of buffers that hold t_total tiles per position: every
    row of [t_off, t_off + t) within bound, every other row untouched (Tt and t_off addressing of winograd4_input_kernel and
    winograd4_dy_kernel); x = NULL and dy = NULL each skip their operand."""
    n, h, w, cin, cout = 1, 8, 12, 8, 12
    t = n * (h // 4) * (w // 4)
    t_total = -(-items * t // 64) * 64
    v, dm = _nan(36, t_total, cin), _nan(36, t_total, cout)
    for i in range(items):
        x, dy = params.normal(9830 + i, n, h, w, cin), params.normal(9840 + i, n, h, w, cout)
        before_v, before_dm = v[:, :i * t].clone(), dm[:, :i * t].clone()
        _call(_lib().dvg_winograd_wgrad_operands, x.to(dev()), dy.to(dev()), v, dm, n, h, w, cin, cout, t_total, i * t)
        (vr, vb), (dr, db) = wr.input_ref(x, 4), wr.dy_ref(dy)
        _report(f"operands item {i} V", v[:, i * t:(i + 1) * t], vr, vb)
        _report(f"operands item {i} dM", dm[:, i * t:(i + 1) * t], dr, db)
        assert bool(_untouched(v[:, (i + 1) * t:]).all()) and bool(_untouched(dm[:, (i + 1) * t:]).all())
        assert torch.equal(v[:, :i * t], before_v) and torch.equal(dm[:, :i * t], before_dm)      # the earlier items' rows stay
    x, dy = params.normal(9830, n, h, w, cin).to(dev()), params.normal(9840, n, h, w, cout).to(dev())
    v2, dm2 = _nan(36, t_total, cin), _nan(36, t_total, cout)
    _call(_lib().dvg_winograd_wgrad_operands, None, dy, v2, dm2, n, h, w, cin, cout, t_total, 0)
    assert bool(_untouched(v2).all()) and torch.equal(dm2[:, :t], dm[:, :t])
    v3, dm3 = _nan(36, t_total, cin), _nan(36, t_total, cout)
    _call(_lib().dvg_winograd_wgrad_operands, x, None, v3, dm3, n, h, w, cin, cout, t_total, 0)
    assert bool(_untouched(dm3).all()) and torch.equal(v3[:, :t], v[:, :t])


# ---- the output transform ---------------------------------------------------------------------------------------------------
def _epilogue(c, seed, random):
    if not random:
        return None, None
    return 1.0 + 0.1 * params.normal(seed, c), 0.1 * params.normal(seed + 1, c)


def _output(mm, n, h, w, c, m, sc, sh, act, addend=None, pool=False, y_from=0):
    """One dvg_winograd_output call on the device; (y or None, pooled y or None), both NaN-prefilled."""
    d = lambda t: None if t is None else t.to(dev())      # noqa: E731
    y = _nan(n - y_from, h, w, c) if y_from < n else None
    yp = _nan(n, h // 2, w // 2, c) if pool else None
    _call(_lib().dvg_winograd_output, d(mm), d(sc), d(sh), y, yp, n, h, w, c, act, 0.2, m, d(addend), y_from)
    return y, yp


@pytest.mark.parametrize("random", [False, True], ids=["unit", "scaled"])
@pytest.mark.parametrize("act", [0, 1, 2, 3], ids=["none", "lrelu", "tanh", "sigmoid"])
@pytest.mark.parametrize("shape", [(1, 4, 4, 4), (3, 8, 12, 20)], ids=["1x4x4x4", "3x8x12x20"])
@pytest.mark.parametrize("m", [2, 4])
def test_output_transform_on_a_synthetic_m(m, shape, act, random):
    """y = act(A^T M A scale + shift) on M from params.normal within output_ref's bound; scale / shift NULL (what return_v
    passes) and random; with the F(4x4) addend."""
    n, h, w, c = shape
    t = n * (h // m) * (w // m)
    mm = params.normal(9850 + m + h, (m + 2) ** 2, t, c)
    sc, sh = _epilogue(c, 9860 + m, random)
    y, _ = _output(mm, n, h, w, c, m, sc, sh, act)
    ref, bound = wr.output_ref(mm, n, h, w, m, sc, sh, act)
    _report(f"output m={m} {shape} act={act} scaled={random}", y, ref, bound)
    if m == 4:
        add = params.normal(9870 + h, n, h, w, c)
        y, _ = _output(mm, n, h, w, c, m, sc, sh, act, addend=add)
        ref, bound = wr.output_ref(mm, n, h, w, m, sc, sh, act, addend=add)
        _report(f"output m=4 {shape} act={act} scaled={random} addend", y, ref, bound)


@pytest.mark.parametrize("shape", [(1, 4, 4, 4), (3, 8, 12, 20)], ids=["1x4x4x4", "3x8x12x20"])
@pytest.mark.parametrize("m", [2, 4])
def test_output_transform_pooled_and_y_from(m, shape):
    """The pooled output is the max-pool of the stored map bit for bit, and y holds exactly the images [y_from, N) (NULL at
    y_from == N)."""
    n, h, w, c = shape
    mm = params.normal(9880 + m + h, (m + 2) ** 2, n * (h // m) * (w // m), c)
    sc, sh = _epilogue(c, 9890 + m, True)
    ref, bound = wr.output_ref(mm, n, h, w, m, sc, sh, wr.ACT_LRELU)
    full, full_p = _output(mm, n, h, w, c, m, sc, sh, wr.ACT_LRELU, pool=True)
    _report(f"output+pool m={m} {shape}", full, ref, bound)
    assert torch.equal(full_p, wr.max_pool_nhwc(full))
    for y_from in sorted({1, n}):
        y, yp = _output(mm, n, h, w, c, m, sc, sh, wr.ACT_LRELU, pool=True, y_from=y_from)
        assert torch.equal(yp, full_p)
        assert (y is None) == (y_from == n)
        if y is not None:
            assert torch.equal(y, full[y_from:])


# ---- the wider forms --------------------------------------------------------------------------------------------------------
def _chunked(fn_ref, src, got, n, tiles_per_image, what, step=8):
    """fn_ref on `step` images at a time against the matching tile range of `got` (P, T, C): the fp64 reference of the whole
    tensor is never held."""
    worst = 0.0
    for i in range(0, n, step):
        ref, bound = fn_ref(src[i:i + step])
        ex, ratio = wr.excess(got[:, i * tiles_per_image:(i + step) * tiles_per_image].cpu(), ref, bound)
        assert ex <= 0.0, (what, i, ex, ratio)
        worst = max(worst, ratio)
    print(f"{what}: measured / bound {worst:.3f}")


@pytest.mark.parametrize("shape,width", wr.WIDE_SHAPES, ids=["f32x2", "f32x4"])
def test_wide_input_and_dy_transforms(shape, width):
    """The smallest launches of the f32x2 and f32x4 forms of winograd4_input_kernel and winograd4_dy_kernel."""
    n, h, w, c = shape
    tpi = (h // 4) * (w // 4)
    assert _lib().dvg_winograd_transform_width(n * tpi, c) == width
    x = params.normal(9900 + width, *shape)
    xd = x.to(dev())
    v = _nan(36, n * tpi, c)
    _call(_lib().dvg_winograd_input, xd, v, n, h, w, c, 4, 0)
    _chunked(lambda s: wr.input_ref(s, 4), x, v, n, tpi, f"input width {width}")
    v2, dm = _nan(36, n * tpi, c), _nan(36, n * tpi, c)
    _call(_lib().dvg_winograd_wgrad_operands, xd, xd, v2, dm, n, h, w, c, c, n * tpi, 0)
    assert torch.equal(v2, v)
    _chunked(wr.dy_ref, x, dm, n, tpi, f"dy width {width}")


@pytest.mark.parametrize("shape,width", wr.WIDE_SHAPES, ids=["f32x2", "f32x4"])
def test_wide_output_transform(shape, width):
    """The f32x2 and f32x4 forms of winograd4_output_kernel, with and without the pooled output."""
    n, h, w, c = shape
    tpi = (h // 4) * (w // 4)
    assert _lib().dvg_winograd_transform_width(n * tpi, c) == width
    mm = params.normal(9910 + width, 36, n * tpi, c)
    sc, sh = _epilogue(c, 9920, True)
    y, _ = _output(mm, n, h, w, c, 4, sc, sh, wr.ACT_LRELU)
    y2, yp = _output(mm, n, h, w, c, 4, sc, sh, wr.ACT_LRELU, pool=True, y_from=n - 8)
    assert torch.equal(y2, y[n - 8:]) and torch.equal(yp, wr.max_pool_nhwc(y))
    y, worst = y.cpu(), 0.0
    for i in range(0, n, 8):
        ref, bound = wr.output_ref(mm[:, i * tpi:(i + 8) * tpi], 8, h, w, 4, sc, sh, wr.ACT_LRELU)
        ex, ratio = wr.excess(y[i:i + 8], ref, bound)
        assert ex <= 0.0, (i, ex, ratio)
        worst = max(worst, ratio)
    print(f"output width {width}: measured / bound {worst:.3f}")


# ---- the batched GEMM -------------------------------------------------------------------------------------------------------
def _x3():
    return _lib().dvg_mfma_mode() == 1


def _skip_unless_built(case):
    if not _x3() and case["plan"] != (8, 1, 1):
        pytest.skip(f"{case['name']}: the f32-MFMA build has no {case['plan']} variant (bf16-triple build only)")


def _gemm_operands(name):
    x, u = wr.gemm_inputs(name)
    return x.to(dev()), wr.pack_rows(u, _row()).to(dev())


def _gemm(name):
    """One dvg_gemm_batched_k16 launch of the case under its policy (restored afterwards); the plan is asserted first."""
    ops, lib, case = _ops(), _lib(), wr.GEMM_BY_NAME[name]
    nb, h, w, cin, cout = case["shape"]
    xd, wd = _gemm_operands(name)
    y = _nan(nb, h, w, cout)
    with ops.tile_policy(case["policy"] == wr.ENERGY):
        plan = wr.gemm_plan(lib, case)
        assert plan == wr.expected_plan(case, _x3()), (name, plan)
        _call(lib.dvg_gemm_batched_k16, xd, wd, y, nb, h, w, cin, cout)
    return y, plan


@pytest.mark.parametrize("name", wr.GEMM_NAMES)
def test_batched_gemm_against_fp64_tile_by_tile(name):
    case = wr.GEMM_BY_NAME[name]
    _skip_unless_built(case)
    x3 = _x3()
    f, b = wr.gemm_figures(name, x3), wr.gemm_bar(name, x3)
    y, plan = _gemm(name)
    assert _lib().dvg_tile_policy() == wr.LATENCY
    e_hip = wr.gemm_err(y.cpu(), wr.gemm_ref(*wr.gemm_inputs(name)), plan)
    print(f"{name} {case['shape']} plan {plan}: e_hip {e_hip:.2e} e32 {f['e32']:.2e} e_y {f['e_y']:.2e} "
          f"e_plane {f['e_plane']:.2e} bar {b:.2e}")
    assert e_hip <= b, (name, e_hip, b)


def test_batched_gemm_is_deterministic():
    a, _ = _gemm("three-stages")
    b, _ = _gemm("three-stages")
    assert torch.equal(a, b)


# ---- the hand-over kernels, called directly on a synthetic M ------------------------------------------------------------------
def _unfused(mm, n, h, c, sc, sh, mode, addend=None):
    """dvg_winograd_output (+ pool) followed by dvg_winograd_input (through the upsampling for "up"): (V', y) on the device."""
    y, yp = _output(mm, n, h, h, c, 4, sc, sh, wr.ACT_LRELU, addend=addend, pool=mode == "pool")
    z, hz = (yp, h // 2) if mode == "pool" else (y, 2 * h if mode == "up" else h)
    v = _nan(36, n * (hz // 4) ** 2, c)
    _call(_lib().dvg_winograd_input, z, v, n, hz, hz, c, 4, int(mode == "up"))
    return v, y


def _handover_inputs(n, h, c, seed, addend=False):
    mm = params.normal(seed, 36, n * (h // 4) ** 2, c)
    sc, sh = _epilogue(c, seed + 1, True)
    return mm, sc, sh, (params.normal(seed + 3, n, h, h, c) if addend else None)


def _check_handover(what, v, mm, n, h, sc, sh, mode, addend=None, step=128):
    """v (36, T', C) against handover_ref, `step` images at a time."""
    tpi, tpo = (h // 4) ** 2, ((h // 2 if mode == "pool" else (2 * h if mode == "up" else h)) // 4) ** 2
    v, worst = v.cpu(), 0.0
    for i in range(0, n, step):
        k = min(step, n - i)
        ref, bound, _, _ = wr.handover_ref(mm[:, i * tpi:(i + k) * tpi], k, h, sc, sh, wr.ACT_LRELU, mode,
                                           None if addend is None else addend[i:i + k])
        ex, ratio = wr.excess(v[:, i * tpo:(i + k) * tpo], ref, bound)
        assert ex <= 0.0, (what, i, ex, ratio)
        worst = max(worst, ratio)
    print(f"{what}: measured / bound {worst:.3f}")


@pytest.mark.parametrize("addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("c", [64, 128])
@pytest.mark.parametrize("h", [8, 16, 32])
def test_output_input_handover(h, c, n, addend):
    """dvg_winograd_output_input against the fp64 composition within the composed bound, and bit for bit against the two
    launches it replaces."""
    mm, sc, sh, add = _handover_inputs(n, h, c, 9930 + h + c + n, addend)
    d = lambda t: None if t is None else t.to(dev())      # noqa: E731
    v = _nan(36, n * (h // 4) ** 2, c)
    _call(_lib().dvg_winograd_output_input, d(mm), d(sc), d(sh), v, n, h, h, c, wr.ACT_LRELU, 0.2, d(add))
    _check_handover(f"output_input h={h} c={c} n={n} addend={addend}", v, mm, n, h, sc, sh, "same", add)
    assert torch.equal(v, _unfused(mm, n, h, c, sc, sh, "same", add)[0])


def test_output_input_handover_16x16_wide_form():
    """16 x 16 maps from N * C/64 >= 1024 on take the <16, 64, f32x2> form (the cases above the <16, 32, float> one)."""
    n, h, c = 1024, 16, 64
    assert n * (c // 64) >= 1024 > 3 * (128 // 64)
    mm, sc, sh, _ = _handover_inputs(n, h, c, 9940)
    v = _nan(36, n * 16, c)
    _call(_lib().dvg_winograd_output_input, mm.to(dev()), sc.to(dev()), sh.to(dev()), v, n, h, h, c, wr.ACT_LRELU, 0.2, None)
    _check_handover("output_input 16x16 n=1024", v, mm, n, h, sc, sh, "same")
    assert torch.equal(v, _unfused(mm, n, h, c, sc, sh, "same")[0])


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h", [16, 32])
def test_output_pool_input_handover(h, n):
    """dvg_winograd_output_pool_input: V' of the pooled map and the skip tensor y, each within its bound and bit-equal to the
    unfused launches; y holds exactly the images [y_from, N)."""
    c = 64
    mm, sc, sh, _ = _handover_inputs(n, h, c, 9950 + h + n)
    md, sd, hd = mm.to(dev()), sc.to(dev()), sh.to(dev())
    v_pair, y_pair = _unfused(mm, n, h, c, sc, sh, "pool")
    _, _, y_ref, y_bound = wr.handover_ref(mm, n, h, sc, sh, wr.ACT_LRELU, "pool")
    for y_from in sorted({0, 1, n}):
        v = _nan(36, n * (h // 8) ** 2, c)
        y = _nan(n - y_from, h, h, c) if y_from < n else None
        _call(_lib().dvg_winograd_output_pool_input, md, sd, hd, y, v, n, h, h, c, wr.ACT_LRELU, 0.2, y_from)
        _check_handover(f"output_pool_input h={h} n={n} y_from={y_from}", v, mm, n, h, sc, sh, "pool")
        assert torch.equal(v, v_pair)
        if y is not None:
            assert torch.equal(y, y_pair[y_from:])
            _report(f"output_pool_input y h={h} n={n} y_from={y_from}", y, y_ref[y_from:], y_bound[y_from:])


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("c", [64, 128])
def test_output_up_input_handover(c, n):
    h = 8
    mm, sc, sh, _ = _handover_inputs(n, h, c, 9970 + c + n)
    v = _nan(36, n * 16, c)
    _call(_lib().dvg_winograd_output_up_input, mm.to(dev()), sc.to(dev()), sh.to(dev()), v, n, h, h, c, wr.ACT_LRELU, 0.2)
    _check_handover(f"output_up_input c={c} n={n}", v, mm, n, h, sc, sh, "up")
    assert torch.equal(v, _unfused(mm, n, h, c, sc, sh, "up")[0])


@pytest.mark.parametrize("M,K", [(64, 90), (50, 90), (3, 128)])
def test_stem_up_input_against_the_fp64_composition(M, K):
    """dvg_stem_up_winograd_input at the shapes of tests/test_gpu_winograd.py's bit-equality check (M no multiple of 8, both KP)
    against fp64: the stem's dot product runs as two chains of KP / 2 FMAs each plus their sum - at most KP / 2 + 1 roundings,
    gamma_(KP/2+1) sum |v| |w| -, then the epilogue and the input transform through the upsampling."""
    c = 64
    kp = 96 if K <= 96 else 128
    vec = params.normal(9980 + M, M, K, scale=0.5).tanh()
    w = params.normal(9981 + M, K, c, 4, 4, scale=0.05)                      # ConvTranspose2d(K, C, 4, 1, 0).weight
    wt = torch.zeros(kp, 16 * c)
    wt[:K] = w.permute(0, 2, 3, 1).reshape(K, 16 * c)
    sc, sh = _epilogue(c, 9982, True)
    wv = _ops().stem_up_winograd_input(vec.to(dev()), wt.to(dev()), K, sc.to(dev()), sh.to(dev()), c)
    torch.cuda.synchronize()
    pre = torch.einsum("mk,kchw->mhwc", vec.double(), w.double())
    pre_err = torch.einsum("mk,kchw->mhwc", vec.double().abs(), w.double().abs()) * wr.gamma(kp // 2 + 1)
    y, y_err = wr.epilogue(pre, pre_err, sc, sh, wr.ACT_LRELU)
    ref, bound = wr.input_ref(y, 4, True, y_err)
    _report(f"stem_up_input M={M} K={K}", wv.v, ref, bound)


# ---- the forward end to end, small and tile-wise ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(wr.FWD_E2E)), ids=wr.FWD_E2E_IDS)
def test_forward_end_to_end_tile_by_tile(k):
    """ops.conv3x3_winograd's raw result (no scale, shift or activation) at the smallest shapes winograd_ok admits against
    torch's fp64 conv2d, per GEMM workgroup tile, under 1.5 x the fp32 Winograd form's own error (floored at the worst case of
    the same m, capped at half a lost plane); the pooled output is the max-pool of the stored one."""
    ops = _ops()
    m, n, h, cin, cout, pool, up = wr.FWD_E2E[k]
    x, w, add = wr.fwd_e2e_inputs(k)
    d = lambda t: t.to(dev()).permute(0, 3, 1, 2)      # noqa: E731
    u = ops.winograd_weight(w.to(dev()), m)
    out = ops.conv3x3_winograd(d(x), u, None, None, act=ops.ACT_NONE, pool=pool, upsample=up, addend=None if add is None else d(add))
    torch.cuda.synchronize()
    y, yp = out if pool else (out, None)
    y = y.permute(0, 2, 3, 1)
    f, b = wr.fwd_e2e_figures(k), wr.fwd_e2e_bar(k)
    e_hip = wr.fwd_e2e_err(y, wr.fwd_e2e_ref(k), m)
    print(f"{wr.FWD_E2E_IDS[k]}: e_hip {e_hip:.2e} e32 {f['e32']:.2e} e_plane {f['e_plane']:.2e} bar {b:.2e}")
    assert e_hip <= b, (k, e_hip, b)
    if pool:
        assert torch.equal(yp.permute(0, 2, 3, 1), wr.max_pool_nhwc(y))
