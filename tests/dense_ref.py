"""fp64 statements, in torch on the CPU, of what the dense kernels compute (dvg_amd/csrc/dense.hip, dvg_lstm_gates_bwd of
backward.hip): the NT / TN products with their epilogue, the decoder stem, the three LSTM forward cells and the two LSTM
backward kernels - written from the formulas, not from the kernels - the measures they are read with, references that carry a
KNOWN defect, and the cases the host and GPU tests share (tests/test_dense_ref_host.py, tests/test_gpu_dense.py;
docs/DESIGN_NOTES_dense_tests.md has the table).

Two measures:
  products     e = max |got - ref| / mag element by element, mag = the element's sum of |terms|; the bar is gamma(d), DERIVED
               from the kernel's own summation tree (product_depth below states d per kernel with its derivation);
  cell outputs max |got - ref| over a wave block / max(max |ref| in the block, 1e-3), maximised over the blocks; the bar is
               backward_ref.bar on torch's fp32 evaluation of the same reference and the smallest planted defect.
"""
import functools
import math

import torch

from oracle import params
from tests.backward_ref import U32, bar, ulp32

ACT_NONE, ACT_LRELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3
ACTS = (ACT_NONE, ACT_LRELU, ACT_TANH, ACT_SIGMOID)
GEMM_TN_MAX_ROWS = 512      # ops.GEMM_TN_MAX_ROWS (asserted by the GPU test)


def gamma(d):
    """gamma_d = d u / (1 - d u): |fp32 result of a chain of d rounded operations - exact| <= gamma_d * sum |terms|
    (backward_ref.sum_bound is the same formula with d = n - 1)."""
    k = d * U32
    return k / (1.0 - k)


def _d(t):
    return t.detach().double().cpu()


def _nan_to_inf(e):
    return float("inf") if e != e else float(e)


# ---- products ---------------------------------------------------------------------------------------------------------
def gemm_nt_ref(a, w):
    """(a w^T, |a| |w|^T): the raw product and each element's sum of |terms|."""
    a, w = _d(a), _d(w)
    return a @ w.t(), a.abs() @ w.abs().t()


def gemm_tn_ref(a, b):
    """(a^T b, |a|^T |b|, column sums of a, column sums of |a|)."""
    a, b = _d(a), _d(b)
    return a.t() @ b, a.abs().t() @ b.abs(), a.sum(0), a.abs().sum(0)


def elem_err(got, ref, mag):
    """max over the elements of |got - ref| / mag (mag == 0: an empty sum, which must come out exactly)."""
    got, ref, mag = _d(got), _d(ref), _d(mag)
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    diff = (got - ref).abs()
    e = torch.where(mag > 0, diff / mag.clamp_min(1e-300), torch.where(diff == 0, diff, torch.full_like(diff, math.inf)))
    return _nan_to_inf(float(e.max()))


def _act64(v, act, slope):
    if act == ACT_LRELU:
        return torch.where(v > 0, v, v * float(torch.tensor(slope, dtype=torch.float32)))   # the slope is an fp32 argument
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    return v


def epilogue_ref(u, scale, shift, period, act, slope=0.0, base=None, defect=None):
    """(act(u * scale[n % period] + shift[n % period]) (+ base), |u scale| + |shift|) from a raw product u (M, N); scale / shift
    None: 1 / 0.  defect "period": scale and shift indexed by n clamped to the period; "no_accumulate": base left out."""
    u = _d(u)
    n = u.shape[1]
    if defect not in (None,) + EPILOGUE_DEFECTS:
        raise ValueError(defect)
    if defect == "period" and (period == n or (scale is None and shift is None)):
        raise ValueError("nothing to clamp")
    if defect == "no_accumulate" and base is None:
        raise ValueError("no base to leave out")
    idx = torch.arange(n).clamp_max(period - 1) if defect == "period" else torch.arange(n) % period
    sc = torch.ones(n, dtype=torch.float64) if scale is None else _d(scale)[idx]
    sh = torch.zeros(n, dtype=torch.float64) if shift is None else _d(shift)[idx]
    y = _act64(u * sc + sh, act, slope)
    if base is not None and defect != "no_accumulate":
        y = y + _d(base)
    return y, (u * sc).abs() + sh.abs()


ACT_LIPSCHITZ = {ACT_NONE: 1.0, ACT_LRELU: 1.0, ACT_TANH: 1.0, ACT_SIGMOID: 0.25}


def epilogue_allowance(ref, mag, act, base=None, act_ulps=0.0):
    """What the fp32 epilogue may differ by from epilogue_ref evaluated on the kernel's own raw u: v = u * sc + sf is a product
    and a sum, LeakyReLU's v * slope a third rounding (and a v that changes sign between fp32 and fp64 moves the result by at
    most the error of v): 3 u32 (|u sc| + |sh|); tanh / sigmoid map that input error with a slope of at most 1 / 0.25 and add
    the device function's own `act_ulps` ulps of the activation's result; the accumulate add rounds once more: u32 |result|."""
    ref, mag = _d(ref), _d(mag)
    allow = 3 * U32 * mag * ACT_LIPSCHITZ[act]
    if act in (ACT_TANH, ACT_SIGMOID):
        allow = allow + act_ulps * ulp32(ref if base is None else ref - _d(base))
    if base is not None:
        allow = allow + U32 * ref.abs()
    return allow


def torch_act_ulps(v32, act):
    """Error of torch-CPU fp32 tanh / sigmoid on the fp32 inputs v32 against fp64, in ulps of the result (the maximum)."""
    f = torch.tanh if act == ACT_TANH else torch.sigmoid
    ref = f(v32.double())
    return float(((f(v32).double() - ref).abs() / ulp32(ref)).max())


def act_ulps_allowed(v32, act):
    """Twice torch's own error on the same inputs, at least 2 ulp (a device function that is correctly one ulp less accurate)."""
    return max(2.0 * torch_act_ulps(v32, act), 2.0)


def ceil_div(a, b):
    return -(-a // b)


def dispatch(M, N, K, splitk=1, lda=None, a_off=0, w_off=0):
    """dvg_gemm_nt_bias_act's dispatch recomputed: (kernel, splits it ends with, kper).  a_off / w_off: the operand's base
    pointer is that many floats past a 16-byte boundary."""
    lda = K if lda is None else lda
    kper = ceil_div(ceil_div(K, splitk), 32) * 32
    vec = K % 4 == 0 and w_off % 4 == 0
    vec_a = K % 4 == 0 and lda % 4 == 0 and a_off % 4 == 0
    if M <= 1024 and N <= 2048:
        if vec and vec_a:
            kper = ceil_div(ceil_div(K, splitk), 256) * 256
            return "dot_vec", ceil_div(K, kper), kper
        return "dot_scalar", ceil_div(K, kper), kper
    return ("tile_vec" if vec and vec_a else "tile_scalar"), ceil_div(K, kper), kper


def product_depth(kernel, K, splits, kper):
    """d: the longest chain of rounded operations between a product and the stored raw value, read off the kernel.
      dot_vec     a lane runs 4 FMAs per 256-wide slice of its split (a split holds at most min(kper, K) terms), the butterfly
                  adds 6 times, the reduce kernel adds the S partials with S - 1 roundings (0 + p is exact);
      dot_scalar  2 FMAs per 128-wide trip, + 6, + (S - 1);
      tile_*      one thread, one FMA per k of its split: min(kper, K), + (S - 1);
    """
    span = min(kper, K)
    if kernel == "dot_vec":
        return 4 * ceil_div(span, 256) + 6 + (splits - 1)
    if kernel == "dot_scalar":
        return 2 * ceil_div(span, 128) + 6 + (splits - 1)
    if kernel.startswith("tile"):
        return span + (splits - 1)
    raise ValueError(kernel)


def gemm_tn_depth(R):
    """gemm_tn: one thread, one FMA per row: R (the rows past R in the last chunk of 32 are zeros: exact).  The long-sum fallback
    (R > GEMM_TN_MAX_ROWS: transposes + the NT dot kernel) has a shorter tree and is held to the same R."""
    return R


def stem_depth(KP):
    """stem: two chains of KP / 2 FMAs (s0, s1), + their sum."""
    return KP // 2 + 1


LSTM_BWD_DEPTH = 16 + 6     # lstm_cell_bwd's dh_prev: 16 FMAs per lane (4 gates x 4 units), two plain exchanges + 4 butterfly adds

PRODUCT_DEFECTS = ("k_last", "lane_slice", "row_clamp", "col_clamp", "split_tail")
EPILOGUE_DEFECTS = ("period", "no_accumulate")


def plant_product(kind, a, w, kper=None, splits=1):
    """An fp64 product like gemm_nt_ref's that carries a known defect (module table in the design notes); ValueError where
    the defect does not apply."""
    a, w = _d(a).clone(), _d(w)
    M, K = a.shape
    N = w.shape[0]
    if kind == "k_last":
        a[:, K - 1] = 0
        return a @ w.t()
    if kind == "lane_slice":
        if K < 256:
            raise ValueError("no lane 63 slice below K = 256")
        a[:, (torch.arange(K) % 256) >= 252] = 0
        return a @ w.t()
    if kind == "split_tail":
        if splits < 2:
            raise ValueError("no split")
        a[:, (splits - 1) * kper:] = 0
        return a @ w.t()
    ref = a @ w.t()
    if kind == "row_clamp":
        if M % 8 < 2:
            raise ValueError("no partial row block with more than one row")
        ref[8 * (M // 8):] = ref[M - 1]
        return ref
    if kind == "col_clamp":
        if N % 8 < 2:
            raise ValueError("no partial column block with more than one column")
        ref[:, 8 * (N // 8):] = ref[:, N - 1:N]
        return ref
    raise ValueError(kind)


# ---- the gemm_nt cases -------------------------------------------------------------------------------------------------
# kernel / splits: what dvg_gemm_nt_bias_act must reach and end with (test_dense_ref_host asserts them against dispatch()).
def _g(M, N, K, splitk, kernel, splits, *, lda=None, ldo=None, a_off=0, w_off=0, accumulate=(False,), tag="", why=""):
    name = f"{M}x{N}x{K}" + (f"-s{splitk}" if splitk > 1 else "") + (f"-{tag}" if tag else "")
    return dict(name=name, M=M, N=N, K=K, splitk=splitk, kernel=kernel, splits=splits, lda=lda, ldo=ldo, a_off=a_off,
                w_off=w_off, accumulate=accumulate, why=why)


GEMM_CASES = [
    _g(1, 1, 4, 1, "dot_vec", 1, why="smallest"),
    _g(9, 9, 260, 1, "dot_vec", 1, why="row and column tails; second slice with one live lane"),
    _g(5, 256, 256, 1, "dot_vec", 1, why="one full slice"),
    _g(64, 90, 8192, 64, "dot_vec", 32, why="64 requested -> 32; unrolled reduce only"),
    _g(7, 33, 2816, 11, "dot_vec", 11, why="reduce: one unrolled trip + tail of 3"),
    _g(8, 8, 520, 3, "dot_vec", 3, why="last split of 8 terms"),
    _g(8, 16, 512, 5, "dot_vec", 2, why="5 requested -> 2, workspace sized for 5"),
    _g(6, 40, 128, 1, "dot_vec", 1, lda=136, ldo=48, accumulate=(False, True), tag="strided",
       why="a and out are column slices; sentinels"),
    _g(1, 1, 1, 1, "dot_scalar", 1, why="smallest"),
    _g(5, 256, 90, 1, "dot_scalar", 1, why="the latent width"),
    _g(9, 17, 129, 1, "dot_scalar", 1, why="second trip with one live lane"),
    _g(130, 33, 1001, 4, "dot_scalar", 4, why="scalar split K, last split of 233"),
    _g(8, 8, 64, 1, "dot_scalar", 1, a_off=1, tag="a+4B", why="a at a 4-byte offset: vec_a = 0"),
    _g(8, 8, 64, 1, "dot_scalar", 1, w_off=1, tag="w+4B", why="w at a 4-byte offset: vec = 0"),
    _g(1025, 8, 8, 1, "tile_vec", 1, why="M tail of one row"),
    _g(3, 2049, 36, 1, "tile_vec", 1, why="vector loads, 4-wide K tail in the second step"),
    _g(64, 2112, 90, 1, "tile_scalar", 1, why="scalar loads: the head's data-gradient shape in small"),
    _g(2, 2112, 200, 3, "tile_vec", 3, why="splits of 96 / 96 / 8"),
    _g(1100, 70, 256, 1, "tile_vec", 1, ldo=72, accumulate=(True,), tag="acc", why="accumulate into a strided out, M tail"),
    _g(130, 2049, 8, 2, "tile_vec", 1, why="2 requested -> 1: K = 8 fits one 32-deep split (no reduce launch)"),
    _g(130, 2049, 40, 2, "tile_vec", 2, why="the reduce kernel's grid-stride loop: M N > 4096 * 64, splits of 32 / 8"),
]
GEMM_BY_NAME = {c["name"]: c for c in GEMM_CASES}
GEMM_NAMES = [c["name"] for c in GEMM_CASES]
assert len(GEMM_BY_NAME) == len(GEMM_CASES)
# one case per kernel (and the reduce kernel) for the epilogue, with a period that divides N properly
EPILOGUE_CASES = {"5x256x256": 64, "5x256x90": 64, "64x2112x90": 64, "7x33x2816-s11": 11}


def gemm_inputs(case):
    """(a (M, K) scaled by 1 / sqrt(K), w (N, K)) from params.normal (full significands), fp32 on the CPU."""
    k = GEMM_CASES.index(case)
    a = params.normal(9000 + 10 * k, case["M"], case["K"], scale=1 / math.sqrt(case["K"]))
    return a, params.normal(9001 + 10 * k, case["N"], case["K"])


def case_dispatch(case):
    return dispatch(case["M"], case["N"], case["K"], case["splitk"], case["lda"], case["a_off"], case["w_off"])


def case_depth(case):
    kernel, splits, kper = case_dispatch(case)
    return product_depth(kernel, case["K"], splits, kper)


# ---- gemm_tn and the stem ----------------------------------------------------------------------------------------------
GEMM_TN_CASES = [(176, 1024, 256), (60, 90, 256), (176, 256, 90), (1, 7, 5), (33, 31, 65), (600, 64, 36), (40, 36, 68)]
GEMM_TN_STRIDED = (33, 90, 256)        # with lda / ldb / ldo wider than the widths, and sentinels
STEM_CASES = [(96, 90, 1, 32, 32), (96, 90, 65, 96, 32), (128, 128, 100, 64, 64), (128, 100, 64, 96, 32)]   # KP, K, M, N, period


def stem_inputs(KP, K, M, N):
    """(vec (M, K), w (N, K)): the stem's product is gemm_nt_ref(vec, w); the kernel reads w transposed and zero-padded."""
    return params.normal(9500 + KP + M, M, K, scale=1 / math.sqrt(K)), params.normal(9501 + KP + M, N, K)


# ---- the LSTM cells ----------------------------------------------------------------------------------------------------
FORWARD_DEFECTS = ("gate_order", "k_tail", "slice2", "bias_once", "row_clamp", "c_stale", "x_tail")
BACKWARD_DEFECTS = ("no_dc", "f_prev", "tanh_c", "no_dh_b", "whh_plain", "null_cprev")


def _last_block(B):
    """First row of the last 8-row block; ValueError where that block holds one row (a clamp cannot show)."""
    r0 = 8 * ((B - 1) // 8)
    if B - r0 < 2:
        raise ValueError("the last row block holds one row")
    return r0


def lstm_cell_ref(x, h, c, w_ih, w_hh, b_ih, b_hh, defect=None, x_half=None):
    """One nn.LSTMCell step, gate order i, f, g, o: dict(h, c, gates (B, 4H), pre, mag = the pre-activations' sum of |terms|).
    The dtype follows the operands (fp64: the reference; fp32: the yardstick).  x_half: W_ih x + b_ih + b_hh given (the `pre`
    form; x, w_ih and the biases are then unused)."""
    H = h.shape[1]
    B = h.shape[0]
    hh, whh = h, w_hh
    if defect == "k_tail":
        hh = h.clone()
        hh[:, H - 4:] = 0
    if defect == "slice2":
        if H <= 256:
            raise ValueError("one 256-wide slice only")
        hh = h.clone()
        hh[:, 256:] = 0
    if x_half is None:
        xx = x
        if defect == "slice2":
            xx = x.clone()
            xx[:, 256:] = 0
        xs = xx @ w_ih.t() + b_ih + (0 if defect == "bias_once" else b_hh)
        mag = xx.abs() @ w_ih.abs().t() + b_ih.abs() + b_hh.abs()
    else:
        if defect == "bias_once":
            raise ValueError("the pre form has no bias of its own")
        xs, mag = x_half, x_half.abs()
    pre = xs + hh @ whh.t()
    mag = mag + hh.abs() @ whh.abs().t()
    if defect == "row_clamp":
        r0 = _last_block(B)
        if B % 8 == 0:
            raise ValueError("no partial row block")
        pre = pre.clone()
        pre[r0:] = pre[B - 1]
    p = [pre[:, k * H:(k + 1) * H] for k in range(4)]
    if defect == "gate_order":
        p[2], p[3] = p[3], p[2]
    i, f, g, o = torch.sigmoid(p[0]), torch.sigmoid(p[1]), torch.tanh(p[2]), torch.sigmoid(p[3])
    cc = c
    if defect == "c_stale":
        r0 = _last_block(B)
        cc = c.clone()
        cc[r0:] = c[B - 1]
    if defect == "row_clamp":
        cc = c.clone()
        cc[r0:] = c[B - 1]
    c2 = f * cc + i * g
    h2 = o * torch.tanh(c2)
    if defect not in (None,) + FORWARD_DEFECTS or defect == "x_tail":
        raise ValueError(defect)
    return {"h": h2, "c": c2, "gates": torch.cat([i, f, g, o], 1), "pre": pre, "mag": mag}


def _r32(t):
    return t.float().double()


def lstm_cell_ordered(x, h, c, w_ih, w_hh, b_ih, b_hh):
    """fp32 arithmetic in lstm_cell_kernel's OWN order (the emulation the design notes explain the saturated case with): lane l
    of a wave owns k = 4 l .. 4 l + 3 of every 256-wide slice and runs ONE chain through them - four FMAs on x, four on h, per
    slice - the 64 lanes' partial sums meet in a halving tree (lanes l and l ^ 32, then ^ 16 ... ^ 1), the two biases are added
    to each other and then to the sum; c' = fma(f, c, i g), h' = o tanh(c').  Every FMA is the exact product (48 bits: exact in
    fp64) added in fp64 and rounded to fp32; tanh / sigmoid are torch's fp32 functions."""
    x, h, c, w_ih, w_hh, b_ih, b_hh = (_d(t) for t in (x, h, c, w_ih, w_hh, b_ih, b_hh))
    B, H = h.shape
    s = torch.zeros(B, 4 * H, 64, dtype=torch.float64)
    for k0 in range(0, H, 256):
        lanes = min(64, (H - k0) // 4)
        for a, w in ((x, w_ih), (h, w_hh)):
            for e in range(4):
                ks = k0 + 4 * torch.arange(lanes) + e
                s[:, :, :lanes] = _r32(a[:, None, ks] * w[None, :, ks] + s[:, :, :lanes])
    n = 64
    while n > 1:
        n //= 2
        s = _r32(s[:, :, :n] + s[:, :, n:2 * n])
    pre = _r32(s[:, :, 0] + _r32(b_ih + b_hh)).float()
    i, f, g, o = (torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]),
                  torch.sigmoid(pre[:, 3 * H:]))
    c2 = _r32(f.double() * c + _r32(i.double() * g.double())).float()
    h2 = o * torch.tanh(c2)
    return {"h": h2, "c": c2, "gates": torch.cat([i, f, g, o], 1), "pre": pre}


def lstm_cell_x_ref(x, h, c, w_e, b_e, w_ih, w_hh, b_ih, b_hh, defect=None):
    """The first cell of a step on the UNFOLDED operands: embed = W_e x + b_e, then the cell."""
    if defect == "x_tail":
        x = x.clone()
        x[:, -2:] = 0
        defect = None
    return lstm_cell_ref(x @ w_e.t() + b_e, h, c, w_ih, w_hh, b_ih, b_hh, defect)


def fold_x(w_e, b_e, w_ih, b_ih, b_hh, kxp):
    """(W_x = W_ih W_e zero-padded to (4H, kxp), bias = W_ih b_e + b_ih + b_hh): folded in fp64, rounded to fp32 ONCE."""
    wx = _d(w_ih) @ _d(w_e)
    out = torch.zeros(wx.shape[0], kxp, dtype=torch.float64)
    out[:, :wx.shape[1]] = wx
    return out.float(), (_d(w_ih) @ _d(b_e) + _d(b_ih) + _d(b_hh)).float()


def lstm_gates_bwd_ref(dh, dc, gates, c_prev, c_new, defect=None):
    """(dG (B, 4H) in the order i, f, g, o, dc_prev) from d h', d c' (None: zero), the saved activated gates, c (None: the zero
    state) and c':  d c = dc + dh o (1 - tanh^2 c'),  dG = [d c g i (1 - i), d c c f (1 - f), d c i (1 - g^2), dh tanh(c') o (1 - o)],
    dc_prev = d c f."""
    H = c_new.shape[1]
    i, f, g, o = (gates[:, k * H:(k + 1) * H] for k in range(4))
    zero = torch.zeros_like(c_new)
    if defect == "tanh_c" and dh is None:
        raise ValueError("without dh, tanh(c') enters nowhere")
    dh = zero if dh is None else dh
    if defect == "no_dc":
        if dc is None:
            raise ValueError("no dc to ignore")
        dc = None
    dc = zero if dc is None else dc
    if defect == "null_cprev":
        if c_prev is not None:
            raise ValueError("c_prev is given")
        c_prev = c_new
    c_prev = zero if c_prev is None else c_prev
    tc = torch.tanh(c_new)
    dcv = dc + dh * o * ((1 - c_new * c_new) if defect == "tanh_c" else (1 - tc * tc))
    df = dcv * (c_new if defect == "f_prev" else c_prev) * f * (1 - f)
    dG = torch.cat([dcv * g * i * (1 - i), df, dcv * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
    if defect not in (None, "no_dc", "null_cprev", "tanh_c", "f_prev"):
        raise ValueError(defect)
    return dG, dcv * f


def lstm_cell_bwd_ref(dh_a, dh_b, dc, gates, c_prev, c_new, w_hh, defect=None):
    """dvg_lstm_cell_bwd: lstm_gates_bwd_ref on dh = dh_a + dh_b (either None) plus dh_prev = dG W_hh (w_hh: (4H, H));
    (dG, dc_prev, dh_prev, |dG| |W_hh|)."""
    if defect == "no_dh_b":
        if dh_b is None or dh_a is None:
            raise ValueError("no dh_b to ignore")
        dh_b = None
    dh = dh_a if dh_b is None else (dh_b if dh_a is None else dh_a + dh_b)
    inner = None if defect in ("no_dh_b", "whh_plain") else defect
    dG, dcp = lstm_gates_bwd_ref(dh, dc, gates, c_prev, c_new, inner)
    # "whh_plain": the transposed buffer (H, 4H) indexed as if it were W_hh (4H, H)
    m = w_hh.t().contiguous().reshape(w_hh.shape) if defect == "whh_plain" else w_hh
    return dG, dcp, dG @ m, dG.abs() @ w_hh.abs()


def block_err(got, ref, rows=8, cols=2):
    """max over the (rows x cols) blocks of max |got - ref| / max(max |ref| in the block, 1e-3): what one wave writes (8 batch rows
    x 2 hidden units of the forward cells, 8 x 4 of the elementwise backward).  NaN / inf comes back as inf."""
    got, ref = _d(got), _d(ref)
    assert got.shape == ref.shape and ref.dim() == 2, (got.shape, ref.shape)
    b, n = ref.shape
    pb, pn = -b % rows, -n % cols
    diff = torch.nn.functional.pad((got - ref).abs(), (0, pn, 0, pb))
    mag = torch.nn.functional.pad(ref.abs(), (0, pn, 0, pb))
    shape = ((b + pb) // rows, rows, (n + pn) // cols, cols)
    e = (diff.reshape(shape).amax((1, 3)) / mag.reshape(shape).amax((1, 3)).clamp_min(1e-3)).max()
    return _nan_to_inf(float(e))


def gate_slices(t):
    """{"gate_i": ..., ...} of a (B, 4H) tensor."""
    H = t.shape[1] // 4
    return {"gate_" + n: t[:, k * H:(k + 1) * H] for k, n in enumerate("ifgo")}


# ---- forward cell cases ------------------------------------------------------------------------------------------------
CELL_CASES = [(1, 64), (5, 64), (8, 64), (33, 128), (40, 64), (21, 256), (64, 256), (9, 512)]
SAT_CASE = (10, 64)                     # rows 1 and 9: pre-activations pushed to +-40 and +-100 by scaling x (by 24 and 64)
CELL_X_CASES = [(5, 256, 90, 92, 90), (33, 64, 128, 128, 128), (9, 128, 2, 4, 2), (21, 256, 90, 92, 100)]   # B, H, Kx, Kxp, ldx
GATES_BWD_CASES = [(1, 64), (21, 256), (5, 100)]
CELL_BWD_BATCHES = [1, 8, 21, 64]       # H = 256
CELL_BWD_COMBOS = [("b+dc", True, True, True, True), ("a+dc", False, True, True, True), ("b,c0", True, False, False, True),
                   ("a,nodhp", False, False, True, False)]    # name, dh_b, dc, c_prev given, dh_prev wanted
CELL_OUTPUTS = ("h", "c", "gate_i", "gate_f", "gate_g", "gate_o")


def cell_inputs(B, H, seed=9700, sat=False):
    """(x, h, c, w_ih, w_hh, b_ih, b_hh), fp32 on the CPU."""
    s = seed + 7 * B + H
    x, h, c = (params.normal(s + i, B, H, scale=0.5) for i in range(3))
    w_ih, w_hh = (params.normal(s + 3 + i, 4 * H, H, scale=1 / math.sqrt(H)) for i in range(2))
    b_ih, b_hh = (params.normal(s + 5 + i, 4 * H, scale=0.1) for i in range(2))
    if sat:
        x[1] *= 24.0
        x[B - 1] *= 64.0
    return x, h, c, w_ih, w_hh, b_ih, b_hh


def cell_x_inputs(B, H, Kx):
    """(x (B, Kx), h, c, w_e (H, Kx), b_e, w_ih, w_hh, b_ih, b_hh)."""
    s = 9800 + 7 * B + H + Kx
    x = params.normal(s, B, Kx, scale=0.5)
    _, h, c, w_ih, w_hh, b_ih, b_hh = cell_inputs(B, H, seed=9850)
    return x, h, c, params.normal(s + 1, H, Kx, scale=1 / math.sqrt(Kx)), params.normal(s + 2, H, scale=0.1), w_ih, w_hh, b_ih, b_hh


def _outputs(r, with_gates=True):
    out = {"h": r["h"], "c": r["c"]}
    if with_gates:
        out.update(gate_slices(r["gates"]))
    return out


def _errs(res, ref, rows=8, cols=2):
    return {k: block_err(res[k], ref[k], rows, cols) for k in ref}


def _applicable(fn, defects):
    out = {}
    for d in defects:
        try:
            out[d] = fn(d)
        except ValueError:
            pass
    return out


@functools.lru_cache(maxsize=None)
def cell_figures(kind, key):
    """{"ref": outputs of the fp64 reference, "e32": per output, the block error of the same reference in torch fp32, "plants":
    {defect: its largest block error over the outputs}} of one forward-cell case; kind "cell" (key (B, H) or "sat"), "pre" (the
    same cases through the `pre` form) or "x" (key: the CELL_X_CASES tuple).  Shared; not to be modified."""
    if kind == "x":
        B, H, Kx, _, _ = key
        ops32 = cell_x_inputs(B, H, Kx)
        fn, defects, gates = lstm_cell_x_ref, FORWARD_DEFECTS, False
        run = lambda ops, d: fn(*ops, defect=d)                                               # noqa: E731
    else:
        B, H = SAT_CASE if key == "sat" else key
        ops32 = cell_inputs(B, H, sat=key == "sat")
        defects, gates = tuple(d for d in FORWARD_DEFECTS if d != "x_tail"), True
        if kind == "pre":
            def run(ops, d):
                x, h, c, w_ih, w_hh, b_ih, b_hh = ops
                return lstm_cell_ref(None, h, c, None, w_hh, None, None, d, x_half=x @ w_ih.t() + b_ih + b_hh)
        else:
            run = lambda ops, d: lstm_cell_ref(*ops, defect=d)                                # noqa: E731
    ops64 = tuple(t.double() for t in ops32)
    ref = _outputs(run(ops64, None), gates)
    e32 = _errs(_outputs(run(ops32, None), gates), ref)
    plants = _applicable(lambda d: max(_errs(_outputs(run(ops64, d), gates), ref).values()), defects)
    fig = {"ref": ref, "e32": e32, "e_y": e32, "plants": plants}
    if (kind, key) in ORDERED_INFO:
        fig["e_ord"] = _errs(_outputs(lstm_cell_ordered(*ops32), gates), ref)
    return fig


# Where the error of fp32 arithmetic in the kernel's own order (lstm_cell_ordered) is computed and printed beside the kernel's:
# the saturated case of dvg_lstm_cell, whose pre-activations of magnitude 40 ... 100 make the ORDER of the additions, not their
# number, the error (design notes, "The saturated case").  For information: the yardstick e_y is torch's fp32 at every case.
ORDERED_INFO = {("cell", "sat")}


def cell_keys(kind):
    return list(CELL_X_CASES) if kind == "x" else list(CELL_CASES) + ["sat"]


@functools.lru_cache(maxsize=None)
def cell_worst_e32(kind):
    figs = [cell_figures(kind, k) for k in cell_keys(kind)]
    return {o: max(f["e_y"][o] for f in figs) for o in figs[0]["e_y"]}


def cell_bars(kind, key):
    """{output: bar}: backward_ref.bar on the output's own yardstick figures and the case's smallest planted defect."""
    f = cell_figures(kind, key)
    worst, plant = cell_worst_e32(kind), min(f["plants"].values())
    return {o: bar(f["e_y"][o], worst[o], plant) for o in f["e_y"]}


# ---- backward cases ----------------------------------------------------------------------------------------------------
def bwd_inputs(B, H, seed=9900):
    """(dh_a, dh_b, dc, gates32, c_prev, c_new32, w_hh): the gates and c' are the fp64 forward cell's, rounded to fp32 - the
    values the kernels read."""
    x, h, c, w_ih, w_hh, b_ih, b_hh = cell_inputs(B, H, seed=seed)
    fwd = lstm_cell_ref(*(t.double() for t in (x, h, c, w_ih, w_hh, b_ih, b_hh)))
    s = seed + 50 + 7 * B + H
    dh_a, dh_b, dc = (params.normal(s + i, B, H) for i in range(3))
    return dh_a, dh_b, dc, fwd["gates"].float(), c, fwd["c"].float(), w_hh


def _bwd_outputs(dG, dcp):
    out = {"d" + k: v for k, v in gate_slices(dG).items()}
    out["dc_prev"] = dcp
    return out


@functools.lru_cache(maxsize=None)
def bwd_figures(B, H, use_a, use_b, use_dc, use_cprev, with_dhp):
    """As cell_figures for the backward kernels (8 x 4 blocks) at one operand combination; with_dhp: dvg_lstm_cell_bwd's
    dh_prev is part of the outputs (the planted defects see it; its own measure is the products')."""
    dh_a, dh_b, dc, gates, c_prev, c_new, w_hh = bwd_inputs(B, H)
    if not use_cprev:      # the zero initial state: c' = i g
        gates, c_new = bwd_inputs_zero_state(B, H)

    def run(dt, d):
        t = lambda v, on=True: v.to(dt) if on else None                                        # noqa: E731
        dG, dcp, dhp, _ = lstm_cell_bwd_ref(t(dh_a, use_a), t(dh_b, use_b), t(dc, use_dc), t(gates), t(c_prev, use_cprev),
                                            t(c_new), t(w_hh), d)
        out = _bwd_outputs(dG, dcp)
        if with_dhp:
            out["dh_prev"] = dhp
        elif d == "whh_plain":
            raise ValueError("no dh_prev")
        return out
    ref = run(torch.float64, None)
    e32 = _errs(run(torch.float32, None), ref, 8, 4)
    e32.pop("dh_prev", None)
    plants = _applicable(lambda d: max(_errs(run(torch.float64, d), ref, 8, 4).values()), BACKWARD_DEFECTS)
    return {"ref": ref, "e32": e32, "e_y": e32, "plants": plants}


def bwd_inputs_zero_state(B, H):
    """(gates32, c_new32) of the forward cell from c = 0."""
    x, h, c, w_ih, w_hh, b_ih, b_hh = cell_inputs(B, H, seed=9900)
    fwd = lstm_cell_ref(*(t.double() for t in (x, h, torch.zeros_like(c), w_ih, w_hh, b_ih, b_hh)))
    return fwd["gates"].float(), fwd["c"].float()


def bwd_case_list():
    """Every (B, H, use_a, use_b, use_dc, use_cprev, with_dhp) the GPU tests run: the lstm_gates_bwd cases (dh only, dc only, both) and
    the lstm_cell_bwd combinations."""
    out = [(B, H, a, False, dc, True, False) for B, H in GATES_BWD_CASES
           for a, dc in ((True, False), (False, True), (True, True))]
    out += [(B, 256, True, ub, udc, ucp, dhp) for B in CELL_BWD_BATCHES for _, ub, udc, ucp, dhp in CELL_BWD_COMBOS]
    return out


@functools.lru_cache(maxsize=None)
def bwd_worst_e32():
    figs = [bwd_figures(*k) for k in bwd_case_list()]
    return {o: max(f["e32"][o] for f in figs) for o in figs[0]["e32"]}


def bwd_bars(*key):
    f = bwd_figures(*key)
    worst, plant = bwd_worst_e32(), min(f["plants"].values())
    return {o: bar(f["e32"][o], worst[o], plant) for o in f["e32"]}
