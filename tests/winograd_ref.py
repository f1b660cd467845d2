"""fp64 references of every stage of the Winograd forward and weight gradient (dvg_amd/csrc/winograd.hip, the batched GEMM
mode of conv_igemm2.hip, wino_wgrad.hip), written from the mathematics in plain torch on the CPU: the transforms with their
derived rounding bounds, the packed weight rows in Python, the batched GEMM and the Winograd-form weight-gradient GEMM with
block-wise comparisons, references that carry a KNOWN defect, the emulation of the GEMM's summation order, and the cases the
host and GPU tests share (tests/test_winograd_ref_host.py, tests/test_gpu_winograd_stages.py, tests/test_gpu_wino_wgrad.py;
docs/DESIGN_NOTES_winograd_tests.md).  The Winograd counterpart of tests/forward_ref.py and tests/backward_ref.py.

Layouts (all on the CPU): activations NHWC (N, H, W, C); transformed tensors (P, T, C) with P = (m + 2)^2 positions xi = a (m + 2)
+ b and T tiles t = (n H/m + ty) W/m + tx; the Winograd-domain weight U (P, Cin, Cout); packed weight rows
[P][Cout/64][Cin/16][64][row]."""
import functools

import torch
import torch.nn.functional as F

from oracle import params
from tests.backward_ref import U32, YARDSTICK_RATIO, bar, round16
from tests.forward_ref import ENERGY, LATENCY, PLANE_PAIRS, bf16_planes

# ---- the matrices (Lavin & Gray, "Fast algorithms for convolutional neural networks", F(2x2,3x3) and F(4x4,3x3)) ----------------
_T = functools.partial(torch.tensor, dtype=torch.float64)
BT = {2: _T([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]),
      4: _T([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
             [0, 4, 0, -5, 0, 1]])}
G = {2: _T([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]),
     4: _T([[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]]) / 24}
AT = {2: _T([[1, 1, 1, 0], [0, 1, -1, -1]]),
      4: _T([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]])}
A4 = AT[4].t().contiguous()             # d(out) -> dM = A dY A^T (winograd4_dy_kernel)
GT4 = G[4].t().contiguous()             # sum of P -> dg = G^T P G (wino_wgrad_reduce_kernel)

# Roundings per output of ONE 1-D pass of each transform, counted from the kernels' code (docs/DESIGN_NOTES_winograd_tests.md has
# the expression behind every figure).  A multiplication by a power of two is exact, a constant that fp32 does not hold (1/6,
# 1/12, 1/24) counts one rounding for its own error, FMA contraction only removes roundings.
K_PASS = {"input2": 1, "input4": 3, "output2": 2, "output4": 3, "dy4": 2, "weight2": 2, "weight4": 4, "reduce4": 5}
ACT_NONE, ACT_LRELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3
ACT_ULPS = 8          # tanhf / expf and the division: a few fp32 ulps of an output that is at most 1 in magnitude


# ((N, H, W, C), channels per thread): the smallest launches of the F(4x4) transforms' wider forms, tiles * C = 2^19 and 2^20
WIDE_SHAPES = [((32, 32, 32, 256), 2), ((64, 32, 32, 256), 4)]


def gamma(k):
    """gamma_k = k u / (1 - k u): the relative error of k consecutive fp32 roundings."""
    return k * U32 / (1.0 - k * U32)


def two_sided(t1, x, t2):
    """(t1 X t2^T, |t1| |X| |t2|^T) over the last two dimensions of x, in fp64."""
    x = x.double()
    return (torch.einsum("ia,...ab,jb->...ij", t1, x, t2), torch.einsum("ia,...ab,jb->...ij", t1.abs(), x.abs(), t2.abs()))


# ---- what the GPU tests share: direct calls of the library's entry points into NaN-prefilled buffers ---------------------------
NAN_BITS = 0x7FC00123          # a quiet NaN with a payload: what an element nobody wrote still holds


def gpu_ops():
    from dvg_amd import ops
    return ops


def gpu_lib():
    from dvg_amd import _lib
    return _lib.lib()


def gpu_call(fn, *args):
    """fn(*args, stream) through the C ABI - tensors and None as pointers - checked and synchronised."""
    from dvg_amd import _lib
    ops = gpu_ops()
    _lib.check(fn(*[ops._p(a) if (a is None or torch.is_tensor(a)) else a for a in args], ops._stream()), fn.__name__)
    torch.cuda.synchronize()


def nan_filled(*shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device="cuda:0").view(torch.float32)


def untouched(t):
    return t.view(torch.int32) == NAN_BITS


def report(what, a, ref, bound):
    """Print measured / bound and assert that `a` lies within `bound` of `ref` everywhere."""
    ex, ratio = excess(a, ref, bound)
    print(f"{what}: measured / bound {ratio:.3f}")
    assert ex <= 0.0, (what, ex, ratio)


# ---- packed weight rows ---------------------------------------------------------------------------------------------------
def _swizzle(row):
    """index [co % 64][k] -> position inside a 16-value plane: the two 8-value halves are swapped where (co % 64) & 8
    (dvg_common.h: wrow_store_pair)."""
    co, k = torch.arange(64).view(64, 1), torch.arange(16).view(1, 16)
    return ((((k >> 3) ^ ((co >> 3) & 1)) << 3) + (k & 7)) if row == 24 else k.expand(64, 16)


def pack_rows(u, row):
    """U (P, Cin, Cout) fp32 -> the packed rows [P][Cout/64][Cin/16][64][row] as dvg_winograd_weight writes them: row = 16 plain
    floats (the f32-MFMA build) or row = 24: three planes h, m, l of 16 bf16 each (the bf16-triple build)."""
    p, cin, cout = u.shape
    assert cin % 16 == 0 and cout % 64 == 0 and row in (16, 24), (u.shape, row)
    w = u.float().reshape(p, cin // 16, 16, cout // 64, 64).permute(0, 3, 1, 4, 2).contiguous()      # [P][cb][chunk][co][k]
    if row == 16:
        return w
    pos = _swizzle(24).expand(w.shape)
    planes = [torch.zeros_like(w, dtype=torch.bfloat16).scatter_(4, pos, pl.to(torch.bfloat16)) for pl in bf16_planes(w)]
    return torch.stack(planes, 4).contiguous().view(torch.int16).reshape(*w.shape[:4], 48).view(torch.float32)


def unpack_rows(packed, p, cin, cout, row):
    """The inverse of pack_rows on a tensor of p * cin * cout / 16 rows in the packed order: U (P, Cin, Cout) fp32, exactly (the
    three planes of a value sum to it)."""
    shape = (p, cout // 64, cin // 16, 64)
    if row == 16:
        w = packed.detach().cpu().float().reshape(*shape, 16)
    else:
        planes = packed.detach().cpu().contiguous().reshape(*shape, 24).view(torch.int16).reshape(*shape, 3, 16).view(torch.bfloat16)
        pos = _swizzle(24).expand(*shape, 16)
        w = sum(planes[..., j, :].double().gather(4, pos) for j in range(3)).float()
    return w.permute(0, 2, 4, 1, 3).reshape(p, cin, cout).contiguous()


# ---- the transforms -------------------------------------------------------------------------------------------------------
def weight_ref(w, m):
    """(U, bound): U (P, Cin, Cout) = G g G^T of a Conv2d weight (Cout, Cin, 3, 3) in fp64 and the elementwise bound of the fp32
    kernel's error."""
    u, mag = two_sided(G[m], w, G[m])                     # (Cout, Cin, m + 2, m + 2)
    k = K_PASS[f"weight{m}"]
    f = lambda t: t.permute(2, 3, 1, 0).reshape((m + 2) ** 2, w.shape[1], w.shape[0])      # noqa: E731
    return f(u), f(mag) * gamma(2 * k)


def _patches(x, m, upsample):
    """x NHWC (N, Hs, Ws, C) -> the (m + 2) x (m + 2) input patches (T, C, m + 2, m + 2) of the m x m output tiles of the map
    (upsampled x2 first when `upsample`), zero padding 1, tiles in the order t = (n Ht + ty) Wt + tx."""
    x = x.double().permute(0, 3, 1, 2)
    if upsample:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    n, c = x.shape[:2]
    p = F.pad(x, (1, 1, 1, 1)).unfold(2, m + 2, m).unfold(3, m + 2, m)        # (N, C, Ht, Wt, a, b)
    return p.permute(0, 2, 3, 1, 4, 5).reshape(-1, c, m + 2, m + 2)


def input_ref(x, m, upsample=False, x_err=None):
    """(V, bound): V (P, T, C) = B^T d B of x NHWC in fp64 (dvg_winograd_input).  x_err: elementwise bound of the error the
    kernel's own x carries against this x (a hand-over kernel transforms what it computed itself): the transform of the
    kernel's x is within gamma (|B^T| (|x| + x_err) |B|) of its exact transform, which is within |B^T| x_err |B| of V."""
    v, mag = two_sided(BT[m], _patches(x, m, upsample), BT[m])
    f = lambda t: t.permute(2, 3, 0, 1).reshape((m + 2) ** 2, t.shape[0], t.shape[1])      # noqa: E731
    g = gamma(2 * K_PASS[f"input{m}"])
    if x_err is None:
        return f(v), f(mag) * g
    prop = two_sided(BT[m], _patches(x_err, m, upsample), BT[m])[1]
    return f(v), f(mag) * g + f(prop) * (1 + g)


def input_ref_loop(x, m, upsample=False):
    """input_ref's V by an explicit loop over the tiles, written from the index formulas of winograd_input_kernel /
    winograd4_input_kernel: the check of input_ref's tile order, halo and layout (small shapes only)."""
    n, hs, ws, c = x.shape
    up = int(upsample)
    h, w = hs << up, ws << up
    ht, wt, e = h // m, w // m, m + 2
    v = torch.zeros(e * e, n * ht * wt, c, dtype=torch.float64)
    for i in range(n):
        for ty in range(ht):
            for tx in range(wt):
                d = torch.zeros(e, e, c, dtype=torch.float64)
                for a in range(e):
                    for b in range(e):
                        yy, xx = m * ty - 1 + a, m * tx - 1 + b
                        if 0 <= yy < h and 0 <= xx < w:
                            d[a, b] = x[i, yy >> up, xx >> up].double()
                o = torch.einsum("ia,abc,jb->ijc", BT[m], d, BT[m])
                v[:, (i * ht + ty) * wt + tx] = o.reshape(e * e, c)
    return v


def dy_ref(dy):
    """(dM, bound): dM (36, T, C) = A dY A^T per 4 x 4 tile of d(out) NHWC (winograd4_dy_kernel)."""
    n, h, w, c = dy.shape
    t = dy.double().reshape(n, h // 4, 4, w // 4, 4, c).permute(0, 1, 3, 5, 2, 4).reshape(-1, c, 4, 4)
    v, mag = two_sided(A4, t, A4)
    f = lambda z: z.permute(2, 3, 0, 1).reshape(36, z.shape[0], c)      # noqa: E731
    return f(v), f(mag) * gamma(2 * K_PASS["dy4"])


def _untile(o, n, h, w, m):
    """(T, C, m, m) per-tile results -> NHWC (N, H, W, C)."""
    c = o.shape[1]
    return o.reshape(n, h // m, w // m, c, m, m).permute(0, 1, 4, 2, 5, 3).reshape(n, h, w, c)


def activation(v, act, slope):
    if act == ACT_LRELU:
        return torch.where(v > 0, v, v * slope)
    return torch.tanh(v) if act == ACT_TANH else (torch.sigmoid(v) if act == ACT_SIGMOID else v)


def output_ref(mm, n, h, w, m, scale=None, shift=None, act=ACT_NONE, slope=0.2, addend=None):
    """(y, bound): y NHWC = act((A^T M A + addend) scale + shift) of M (P, T, C) in fp64 (dvg_winograd_output) and the bound of
    the fp32 kernel's error: gamma_(2 k) |A^T| |M| |A| of the transform, one rounding of the addend's sum, the epilogue's
    2 u (|v sc| + |sh|) (3 u with LeakyReLU, which also covers a sign of v that differs between fp32 and fp64:
    tests/test_gpu_forward_igemm.py), and ACT_ULPS for tanh / sigmoid, both of which are 1-Lipschitz."""
    e, c = m + 2, mm.shape[2]
    q = mm.double().reshape(e, e, -1, c).permute(2, 3, 0, 1)          # (T, C, a, b)
    o, mag = two_sided(AT[m], q, AT[m])
    o, err = _untile(o, n, h, w, m), _untile(mag, n, h, w, m) * gamma(2 * K_PASS[f"output{m}"])
    if addend is not None:
        o = o + addend.double()
        err = err + U32 * (o.abs() + err)
    return epilogue(o, err, scale, shift, act, slope)


def epilogue(o, err, scale, shift, act, slope=0.2):
    """(act(o scale + shift), bound) over the last (channel) dimension, for a raw o the kernel holds within err."""
    c = o.shape[-1]
    sc = torch.ones(c, dtype=torch.float64) if scale is None else scale.double()
    sh = torch.zeros(c, dtype=torch.float64) if shift is None else shift.double()
    v = o * sc + sh
    slope = float(torch.tensor(slope, dtype=torch.float32))          # the kernel's slope is an fp32 argument
    if scale is not None or shift is not None or act != ACT_NONE:
        err = err * sc.abs() * (1 + 3 * U32) + (3 if act == ACT_LRELU else 2) * U32 * ((o * sc).abs() + sh.abs())
    if act in (ACT_TANH, ACT_SIGMOID):
        err = err + ACT_ULPS * U32
    return activation(v, act, slope), err


def max_pool_nhwc(y):
    n, h, w, c = y.shape
    return y.reshape(n, h // 2, 2, w // 2, 2, c).amax((2, 4))


def handover_ref(mm, n, h, scale, shift, act, mode, addend=None):
    """The hand-over kernels' composition in fp64 for M (36, T, C) of an h x h F(4x4) layer: y = the output transform with its
    epilogue, then mode "same": V' = the input transform of y; "pool": of maxpool2x2(y) (|max a - max b| <= max |a - b|: the
    pooled map is within the window's largest bound); "up": of y read through the x2 upsampling.  (V', bound of V', y, bound
    of y)."""
    y, y_err = output_ref(mm, n, h, h, 4, scale, shift, act, addend=addend)
    z, z_err = (max_pool_nhwc(y), max_pool_nhwc(y_err)) if mode == "pool" else (y, y_err)
    v, v_err = input_ref(z, 4, mode == "up", z_err)
    return v, v_err, y, y_err


def reduce_ref(part):
    """(packed, bound): packed (9, Cout, Cin) = G^T (sum_s P[s]) G of part (S, 36, Cout, Cin) (wino_wgrad_reduce_kernel: the S
    slabs added in order from zero, then the two passes)."""
    s = part.shape[0]
    tot, tot_abs = part.double().sum(0), part.double().abs().sum(0)
    f = lambda t: t.reshape(6, 6, *t.shape[1:]).permute(2, 3, 0, 1)      # noqa: E731
    d, mag = two_sided(GT4, f(tot), GT4)
    sum_err = two_sided(GT4, f(tot_abs), GT4)[1] * gamma(max(s - 1, 0))
    g = lambda t: t.permute(2, 3, 0, 1).reshape(9, *t.shape[:2])        # noqa: E731
    k = K_PASS["reduce4"]
    return g(d), g(mag * gamma(2 * k) + sum_err * (1 + gamma(2 * k)))


def excess(a, ref, bound):
    """(max (|a - ref| - bound), max |a - ref| / bound): <= 0 / <= 1 where `a` is within the bound; a NaN in `a` gives inf."""
    d = (a.detach().double().cpu() - ref).abs()
    if not bool(torch.isfinite(d).all()):
        return float("inf"), float("inf")
    return float((d - bound).max()), float((d / bound.clamp_min(1e-300)).max())


# ---- the batched GEMM (dvg_gemm_batched_k16) ----------------------------------------------------------------------------------
# (NB, H, W, Cin, Cout), the policy, and what dvg_gemm_batched_plan must answer on the bf16-triple build (tile_w, nt, ni) and on
# the f32-MFMA build (which has the 64-row tile with ni = 1 only): tests/test_winograd_ref_host.py asserts both.
def _gcase(name, shape, policy, plan, why, plan_f32=(8, 1, 1)):
    return dict(name=name, shape=shape, policy=policy, plan=plan, plan_f32=plan_f32, why=why)


GEMM_CASES = [
    _gcase("one-wg", (1, 8, 8, 64, 64), LATENCY, (8, 1, 1), "one workgroup, one stage: the pipeline's prologue is its last stage"),
    _gcase("three-stages", (3, 8, 16, 192, 128), LATENCY, (8, 1, 1), "64-row tile, three stages, two Cout blocks"),
    _gcase("eight-stages", (2, 16, 8, 512, 64), LATENCY, (8, 1, 1), "64-row tile, eight stages"),
    _gcase("ni2", (2, 3072, 16, 128, 64), LATENCY, (8, 1, 2), "2 x 768 workgroup slots: two images in one pipeline"),
    _gcase("ni3", (3, 3072, 16, 128, 64), LATENCY, (8, 1, 3), "3 x 768 workgroup slots: three images in one pipeline"),
    _gcase("rows128-k64", (4, 3072, 16, 64, 128), LATENCY, (16, 1, 1), "3072 workgroups of the 128-row tile: two stages of K = 32"),
    _gcase("rows128-k192", (4, 3072, 16, 192, 128), LATENCY, (16, 1, 1), "the 128-row tile, six stages"),
    _gcase("nt2", (4, 512, 16, 128, 128), ENERGY, (16, 2, 1), "256 workgroups of the 128 x 128 tile, one Cout block"),
    _gcase("nt2-o256", (2, 512, 16, 128, 256), ENERGY, (16, 2, 1), "256 workgroups of the 128 x 128 tile, two Cout blocks"),
    _gcase("energy-o192", (4, 512, 16, 128, 192), ENERGY, (8, 1, 2),
           "Cout % 128 != 0: the 128 x 128 tile is not offered - the 64-row tile, whose 1536 workgroups pair the four images up"),
]
GEMM_BY_NAME = {c["name"]: c for c in GEMM_CASES}
GEMM_NAMES = [c["name"] for c in GEMM_CASES]
EMU_BLOCKS = 48           # pixel tiles the emulation of the summation order is evaluated on (all of them where a case has fewer)


def gemm_plan(lib, case):
    """(tile_w, nt, ni) of the case from dvg_gemm_batched_plan under the case's policy; the policy is restored."""
    import ctypes
    tw, nt, ni = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    old = lib.dvg_tile_policy()
    lib.dvg_set_tile_policy(case["policy"])
    try:
        rc = lib.dvg_gemm_batched_plan(*case["shape"], ctypes.byref(tw), ctypes.byref(nt), ctypes.byref(ni))
    finally:
        lib.dvg_set_tile_policy(old)
    assert rc == 0, (case["name"], rc)
    return tw.value, nt.value, ni.value


def expected_plan(case, x3):
    return case["plan"] if x3 else case["plan_f32"]


def stage_k(plan, x3):
    """Channels one pipeline stage consumes: 64 on the 64-row tile, 32 on the bf16-triple build's 128-row and 128 x 128 tiles
    (conv_igemm2.hip: DVG_GEMM_GT, DVG_GEMM128_GT, NT = 2 -> 2 slabs)."""
    return 64 if plan[0] == 8 or not x3 else 32


def plane_pairs(plan):
    """The order of the six bf16 MFMAs of one 16-channel slab: the LEAN fragment schedule of the 128-row and 128 x 128 tiles
    issues (l,h) (h,l) (m,m) (m,h) (h,m) (h,h), the 64-row tile forward_ref.PLANE_PAIRS."""
    return ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)) if plan[0] == 16 else PLANE_PAIRS


def gemm_inputs(name):
    """(x (NB, H, W, Cin), U (NB, Cin, Cout)) fp32 from params.normal: full significands, U scaled to unit-variance outputs."""
    nb, h, w, cin, cout = GEMM_BY_NAME[name]["shape"]
    k = GEMM_NAMES.index(name)
    return params.normal(9700 + 10 * k, nb, h, w, cin), params.normal(9701 + 10 * k, nb, cin, cout, scale=cin ** -0.5)


def gemm_ref(x, u, dtype=torch.float64):
    nb, h, w, cin = x.shape
    return torch.bmm(x.reshape(nb, h * w, cin).to(dtype), u.to(dtype)).reshape(nb, h, w, -1)


def gemm_blocks(a, ref, plan):
    """(NB, H/8, W/tw, Cout/bn) block-wise max |a - ref| / max |ref|: a block is what one workgroup writes - one image, an
    8 x tile_w pixel tile, 64 nt output channels.  NaN / inf in `a` come back as inf."""
    tw, nt, _ = plan
    a, ref = a.detach().double().cpu(), ref.double()
    nb, h, w, cout = ref.shape
    bn = 64 * nt
    assert a.shape == ref.shape and h % 8 == 0 and w % tw == 0 and cout % bn == 0, (a.shape, ref.shape, plan)
    shape = (nb, h // 8, 8, w // tw, tw, cout // bn, bn)
    d = (a - ref).abs().reshape(shape).amax((2, 4, 6))
    e = d / ref.abs().reshape(shape).amax((2, 4, 6)).clamp_min(1e-300)
    return torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)


def gemm_err(a, ref, plan):
    return float(gemm_blocks(a, ref, plan).max())


GEMM_PLANTS = ("plane_x", "plane_u", "slab", "wrap", "half", "image")


def gemm_plant(kind, x, u, plan, x3=True):
    """An fp64 result like gemm_ref's that carries a known defect (ValueError where the case has no such edge):
      "plane_x" / "plane_u": the operand rounded to 16 significant bits (a lost low bf16 plane);
      "slab":   the last 16-channel slab dropped;
      "wrap":   in a run of ni > 1 images the last stage of image i is multiplied with image i + 1's weights;
      "half":   in a 128 x 128 block the upper 64 output channels read the lower 64's weights;
      "image":  image b reads image 0's weights."""
    nb, cin = x.shape[0], x.shape[3]
    tw, nt, ni = plan
    if kind == "plane_x":
        return gemm_ref(round16(x), u)
    if kind == "plane_u":
        return gemm_ref(x, round16(u))
    if kind == "slab":
        u2 = u.clone()
        u2[:, -16:] = 0
        return gemm_ref(x, u2)
    if kind == "wrap":
        if ni < 2:
            raise ValueError("one image per pipeline")
        ks = stage_k(plan, x3)
        y = gemm_ref(x, u).clone()
        for b in range(nb):
            if b % ni != ni - 1:
                y[b] = gemm_ref(x[b:b + 1, ..., :cin - ks], u[b:b + 1, :cin - ks])[0] + \
                    gemm_ref(x[b:b + 1, ..., cin - ks:], u[b + 1:b + 2, cin - ks:])[0]
        return y
    if kind == "half":
        if nt != 2:
            raise ValueError("no 128-wide Cout block")
        u2 = u.clone().reshape(nb, cin, -1, 2, 64)
        u2[:, :, :, 1] = u2[:, :, :, 0]
        return gemm_ref(x, u2.reshape(u.shape))
    if kind == "image":
        if nb < 2:
            raise ValueError("one image")
        return gemm_ref(x, u[:1].expand_as(u))
    raise ValueError(kind)


def emu_tiles(h, w, tw):
    """The pixel tiles (ty, tx) of an image the emulation runs on: all of them up to EMU_BLOCKS, else EMU_BLOCKS spread evenly
    with the first and the last among them."""
    tiles = [(ty, tx) for ty in range(h // 8) for tx in range(w // tw)]
    if len(tiles) <= EMU_BLOCKS:
        return tiles
    idx = sorted({round(i * (len(tiles) - 1) / (EMU_BLOCKS - 1)) for i in range(EMU_BLOCKS)})
    return [tiles[i] for i in idx]


def gemm_ordered(x, u, pairs):
    """The product in the bf16-triple kernel's summation order, for x (NB, pixels, Cin): ONE fp32 accumulator per output walked
    through the 16-channel slabs in order; per slab six MFMAs on the operands' bf16 planes in the order `pairs`, each adding
    its 16 exact products in two steps (k 0-7, k 8-15) with the accumulator rounded after each
    (forward_ref.ordered_fp32_ref(per_mfma=True) has the evidence for that model)."""
    xp, up = bf16_planes(x), bf16_planes(u)
    acc = torch.zeros(x.shape[0], x.shape[1], u.shape[2], dtype=torch.float32)
    for s in range(x.shape[2] // 16):
        for pa, pb in pairs:
            for k0 in (16 * s, 16 * s + 8):
                acc = (acc.double() + torch.bmm(xp[pa][:, :, k0:k0 + 8], up[pb][:, k0:k0 + 8])).float()
    return acc


@functools.lru_cache(maxsize=None)
def gemm_figures(name, x3=True):
    """{"e32", "e_emu", "e_y", "e_plane_x", "e_plane_u", "e_plane"} of the case at the plan of the build: torch's fp32
    error, the emulation's (on emu_tiles), the yardstick - the emulation on the bf16-triple build, torch's fp32 on the f32-MFMA
    build - and the lost planes, all block-wise against fp64 (floats only: the large cases' tensors are not kept)."""
    case = GEMM_BY_NAME[name]
    plan = expected_plan(case, x3)
    x, u = gemm_inputs(name)
    ref = gemm_ref(x, u)
    f = {"e32": gemm_err(gemm_ref(x, u, torch.float32), ref, plan)}
    for kind in ("plane_x", "plane_u"):
        f["e_" + kind] = gemm_err(gemm_plant(kind, x, u, plan, x3), ref, plan)
    f["e_plane"] = min(f["e_plane_x"], f["e_plane_u"])
    if x3:
        nb, h, w, cin, _ = case["shape"]
        tw = plan[0]
        tiles = emu_tiles(h, w, tw)
        pick = lambda t: torch.stack([t[:, 8 * ty:8 * ty + 8, tw * tx:tw * tx + tw] for ty, tx in tiles], 1)      # noqa: E731
        xs = pick(x).reshape(nb, -1, cin)                                   # (NB, tiles * 8 * tw, Cin)
        emu = gemm_ordered(xs, u, plane_pairs(plan)).reshape(nb, len(tiles) * 8, tw, -1)
        f["e_emu"] = gemm_err(emu, pick(ref).reshape(emu.shape), plan)
    f["e_y"] = f["e_emu"] if x3 else f["e32"]
    return f


@functools.lru_cache(maxsize=None)
def gemm_worst(x3=True):
    return max(gemm_figures(n, x3)["e_y"] for n in GEMM_NAMES)


# The yardstick's ratio.  bf16-triple build: tests.backward_ref's 1.5 - the yardstick IS the kernel's summation order (batched GEMM)
# or the kernel passes torch's own (weight gradient).  f32-MFMA build: the yardstick is torch's blocked fp32 product while the
# kernels walk ONE fp32 accumulator through all of K, two k per MFMA - measured 1.7 ... 2.3 x torch at the longest chains; the
# rule of docs/DESIGN_NOTES_backward_tests.md for that situation: ratio 4 with the summation order as the reason, under the cap.
def yardstick_ratio(x3):
    return YARDSTICK_RATIO if x3 else 4.0


def ratio_bar(e_y, worst, e_plane, x3):
    return bar(e_y, worst, e_plane) if x3 else min(max(yardstick_ratio(x3) * e_y, worst), 0.5 * e_plane)


def gemm_bar(name, x3=True):
    f = gemm_figures(name, x3)
    return ratio_bar(f["e_y"], gemm_worst(x3), f["e_plane"], x3)


# ---- the Winograd-form weight gradient (wino_wgrad.hip) -----------------------------------------------------------------------
def ww_plan(tp, cin, cout):
    """wino_wgrad.hip's ww_plan and the kernel's segment arithmetic, restated: stages of 32 tiles, 36 * Cin/128 * Cout/128 output
    blocks of nst stages each in ONE sequence, one round of at most 512 workgroups of q >= 8 consecutive stages; block b is cut
    into segs[b] segments, S = the most segments any block has."""
    nst = tp // 32
    blocks = 36 * (cin // 128) * (cout // 128)
    total = blocks * nst
    wgs = 512
    if wgs * 8 > total:
        wgs = -(-total // 8)
    q = -(-total // wgs)
    wgs = -(-total // q)
    segs = [(b * nst + nst - 1) // q - b * nst // q + 1 for b in range(blocks)]
    return dict(nst=nst, blocks=blocks, total=total, q=q, wgs=wgs, segs=segs, S=max(segs), short=wgs * q - total)


def _wcase(name, tp, cin, cout, plan, why, t_item=None, t_real=None):
    return dict(name=name, tp=tp, cin=cin, cout=cout, plan=plan, why=why, t_item=t_item or tp, t_real=t_real or tp)


# plan: (nst, q, workgroups, S) as ww_plan gives them (asserted on the host, S against dvg_winograd_wgrad_splits too)
WGEMM_CASES = [
    _wcase("whole-blocks", 64, 128, 128, (2, 8, 9, 1), "a workgroup runs four whole blocks: the block-to-block hand-off", t_real=40),
    _wcase("cut-blocks", 192, 128, 128, (6, 8, 27, 2), "blocks cut across workgroups; uncut blocks zero-fill slab 1", t_real=170),
    _wcase("short-tail", 1088, 256, 256, (34, 10, 490, 5), "490 workgroups, the last 4 stages short; up to 5 segments per block",
           t_real=1070),
    _wcase("items3x64", 192, 128, 128, (6, 8, 27, 2), "three V buffers of 64 tiles: a workgroup crosses item boundaries", t_item=64),
    _wcase("items2x128", 256, 128, 128, (8, 8, 36, 1), "two V buffers of 128 tiles: the boundary in the middle of every block",
           t_item=128),
]
WGEMM_BY_NAME = {c["name"]: c for c in WGEMM_CASES}
WGEMM_NAMES = [c["name"] for c in WGEMM_CASES]


def wgemm_inputs(name):
    """(dM (36, Tp, Cout), [V_i (36, t_item, Cin)]) fp32 from params.normal; the rows from t_real on are zero padding."""
    c = WGEMM_BY_NAME[name]
    k = WGEMM_NAMES.index(name)
    dm, v = params.normal(9750 + 10 * k, 36, c["tp"], c["cout"]), params.normal(9751 + 10 * k, 36, c["tp"], c["cin"])
    dm[:, c["t_real"]:] = 0
    v[:, c["t_real"]:] = 0
    return dm, [v[:, i:i + c["t_item"]].contiguous() for i in range(0, c["tp"], c["t_item"])]


def wgemm_ref(dm, vs, dtype=torch.float64):
    """P (36, Cout, Cin) = sum_t dM[xi][t][co] V[xi][t][ci]."""
    return torch.bmm(dm.to(dtype).transpose(1, 2), torch.cat(list(vs), 1).to(dtype))


WGEMM_PLANTS = ("plane", "segment", "item", "tail", "pos")


def wgemm_plant(kind, name):
    """An fp64 P like wgemm_ref's that carries a known defect (ValueError where the case has no such edge):
      "plane":   dM rounded to 16 significant bits;
      "segment": the second segment of the first block that is cut is dropped;
      "item":    the stages of item 1 read item 0's V;
      "tail":    the padding rows hold data, not zeros;
      "pos":     two positions swapped."""
    c = WGEMM_BY_NAME[name]
    dm, vs = wgemm_inputs(name)
    if kind == "plane":
        return wgemm_ref(round16(dm), vs)
    if kind == "segment":
        pl = ww_plan(c["tp"], c["cin"], c["cout"])
        cut = [b for b, s in enumerate(pl["segs"]) if s > 1]
        if not cut:
            raise ValueError("no block is cut")
        b = cut[0]
        first_w = b * pl["nst"] // pl["q"]
        s0 = (first_w + 1) * pl["q"] - b * pl["nst"]              # the second segment's first stage inside the block
        s1 = min(pl["nst"], s0 + pl["q"])
        nbj, nbi = c["cin"] // 128, c["cout"] // 128
        bj, bi, xi = b % nbj, (b // nbj) % nbi, b // (nbj * nbi)
        ref = wgemm_ref(dm, vs).clone()
        rows = slice(32 * s0, 32 * s1)
        v = torch.cat(vs, 1)
        ref[xi, 128 * bi:128 * bi + 128, 128 * bj:128 * bj + 128] -= \
            dm[xi, rows, 128 * bi:128 * bi + 128].double().t() @ v[xi, rows, 128 * bj:128 * bj + 128].double()
        return ref
    if kind == "item":
        if len(vs) < 2:
            raise ValueError("one V buffer")
        return wgemm_ref(dm, [vs[0], vs[0]] + list(vs[2:]))
    if kind == "tail":
        if c["t_real"] == c["tp"]:
            raise ValueError("no padding rows")
        dm2, v2 = dm.clone(), torch.cat(vs, 1)
        dm2[:, c["t_real"]:] = params.normal(9799, 36, c["tp"] - c["t_real"], c["cout"])
        v2[:, c["t_real"]:] = params.normal(9798, 36, c["tp"] - c["t_real"], c["cin"])
        return wgemm_ref(dm2, [v2])
    if kind == "pos":
        ref = wgemm_ref(dm, vs).clone()
        ref[[7, 8]] = ref[[8, 7]]
        return ref
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def wgemm_figures(name):
    """{"e32", "e_plane"}: torch's fp32 product and the lost planes (dM rounded, V rounded: the smaller), block-wise
    (backward_ref.blockwise_err: position x 64 x 64 block, a wave's quarter of the workgroup's block) against fp64."""
    from tests.backward_ref import blockwise_err
    dm, vs = wgemm_inputs(name)
    ref = wgemm_ref(dm, vs)
    e_dm = blockwise_err(wgemm_ref(round16(dm), vs), ref)
    e_v = blockwise_err(wgemm_ref(dm, [round16(v) for v in vs]), ref)
    return {"e32": blockwise_err(wgemm_ref(dm, vs, torch.float32), ref), "e_plane": min(e_dm, e_v)}


@functools.lru_cache(maxsize=None)
def wgemm_worst():
    return max(wgemm_figures(n)["e32"] for n in WGEMM_NAMES)


def wgemm_bar(name, x3=True):
    f = wgemm_figures(name)
    return ratio_bar(f["e32"], wgemm_worst(), f["e_plane"], x3)


# ---- the forward end to end (ops.conv3x3_winograd), small and tile-wise -------------------------------------------------------
# (m, N, H = W of the output, Cin, Cout, pool, upsample with addend): the smallest shapes ops.winograd_ok admits (128 tiles)
FWD_E2E = [(2, 2, 16, 64, 64, False, False), (2, 8, 8, 128, 64, True, False), (4, 8, 16, 64, 64, False, False),
           (4, 32, 8, 64, 128, True, False), (4, 2, 32, 128, 64, False, False), (4, 8, 16, 64, 64, False, True)]
FWD_E2E_IDS = [f"m{m}-n{n}-h{h}-c{ci}-o{co}" + ("-pool" if p else "") + ("-up-add" if u else "") for m, n, h, ci, co, p, u in FWD_E2E]


def fwd_e2e_inputs(k):
    """(x NHWC - stored at half the side when the case upsamples -, w (Cout, Cin, 3, 3) scaled to unit-variance outputs, addend
    NHWC or None) of case k."""
    m, n, h, cin, cout, _, up = FWD_E2E[k]
    hs = h // 2 if up else h
    return (params.normal(9990 + 10 * k, n, hs, hs, cin), params.normal(9991 + 10 * k, cout, cin, 3, 3, scale=(9 * cin) ** -0.5),
            params.normal(9992 + 10 * k, n, h, h, cout) if up else None)


def fwd_winograd_form(k, dtype, lost=None):
    """The raw convolution of case k NHWC (N, H, W, Cout) computed in Winograd form - U = G g G^T, V = B^T d B, M = V U per
    position, A^T M A, + addend - in `dtype` with the matrices rounded to it (float32: the yardstick).  lost = "v" / "u" (with
    float64): that operand as fp32 rounded to 16 significant bits, the rest exact - a lost low bf16 plane in the GEMM."""
    m, n, h, cin, cout, _, up = FWD_E2E[k]
    x, w, add = fwd_e2e_inputs(k)
    bt, g, at = BT[m].to(dtype), G[m].to(dtype), AT[m].to(dtype)
    v = torch.einsum("ia,tcab,jb->ijtc", bt, _patches(x, m, up).to(dtype), bt)
    u = torch.einsum("ia,ocab,jb->ijco", g, w.to(dtype), g)
    if lost == "v":
        v = round16(v.float()).to(dtype)
    if lost == "u":
        u = round16(u.float()).to(dtype)
    y = torch.einsum("pa,abto,qb->topq", at, torch.einsum("ijtc,ijco->ijto", v, u), at)
    y = _untile(y, n, h, h, m)
    return y if add is None else y + add.to(dtype)


def fwd_e2e_err(a, ref, m):
    """max over every (GEMM workgroup tile, 64-wide Cout block) of max |a - ref| / max |ref| inside it, a and ref NHWC: the tiles
    t = 16 r + c enter the batched GEMM as pixel (r, c) of a (T / 16) x 16 image, and the 64-row workgroup tile takes 8 x 8 of
    them - the output pixels of those 64 Winograd tiles form one block."""
    a, ref = a.detach().double().cpu(), ref.double()
    n, h, w, c = ref.shape
    f = lambda z: z.reshape(n, h // m, m, w // m, m, c).permute(0, 1, 3, 5, 2, 4).reshape(-1, 16, c // 64, 64 * m * m)   # noqa: E731
    t = n * (h // m) * (w // m)
    g = lambda z: f(z).reshape(t // 128, 8, 2, 8, c // 64, 64 * m * m).amax((1, 3, 5))      # noqa: E731
    e = g((a - ref).abs()) / g(ref.abs()).clamp_min(1e-300)
    e = e.max()
    return float("inf") if torch.isnan(e) else float(e)


@functools.lru_cache(maxsize=None)
def fwd_e2e_figures(k):
    """{"e32", "e_plane_v", "e_plane_u", "e_plane"} of case k against torch's fp64 conv2d, tile-wise."""
    m, n, h, cin, cout, _, up = FWD_E2E[k]
    ref = fwd_e2e_ref(k)
    assert fwd_e2e_err(fwd_winograd_form(k, torch.float64), ref, m) < 1e-12
    f = {"e32": fwd_e2e_err(fwd_winograd_form(k, torch.float32), ref, m),
         "e_plane_v": fwd_e2e_err(fwd_winograd_form(k, torch.float64, "v"), ref, m),
         "e_plane_u": fwd_e2e_err(fwd_winograd_form(k, torch.float64, "u"), ref, m)}
    f["e_plane"] = min(f["e_plane_v"], f["e_plane_u"])
    return f


def fwd_e2e_ref(k):
    """The raw convolution (+ addend) of case k by torch's conv2d in fp64, NHWC."""
    up = FWD_E2E[k][6]
    x, w, add = fwd_e2e_inputs(k)
    xx = x.double().permute(0, 3, 1, 2)
    if up:
        xx = F.interpolate(xx, scale_factor=2, mode="nearest")
    y = F.conv2d(xx, w.double(), None, 1, 1).permute(0, 2, 3, 1)
    return y if add is None else y + add.double()


@functools.lru_cache(maxsize=None)
def fwd_e2e_worst(m):
    return max(fwd_e2e_figures(k)["e32"] for k in range(len(FWD_E2E)) if FWD_E2E[k][0] == m)


def fwd_e2e_bar(k):
    f = fwd_e2e_figures(k)
    return bar(f["e32"], fwd_e2e_worst(FWD_E2E[k][0]), f["e_plane"])


# ---- the weight gradient end to end (ops.winograd_wgrad_partial_multi) ---------------------------------------------------------
# (N, H = W, Cin, Cout, items, the saved-V path): 8 tiles padded to 64; 3 x 12 tiles packed at t_off 0 / 12 / 24 and padded to 64;
# 2 x 32 tiles, no padding; 64 tiles; two items whose saved V buffers (t % 64 == 0) are read in place; and 576 tiles, whose
# blocks are cut into up to 3 segments - the one case with S > 2, where the wrapper sums the slabs with dvg_reduce_partials first
WGRAD_E2E = [(2, 8, 128, 128, 1, False), (3, 8, 128, 256, 3, False), (2, 16, 256, 128, 2, False), (1, 32, 128, 128, 1, False),
             (1, 32, 128, 128, 2, True), (9, 32, 128, 128, 1, False)]
WGRAD_E2E_IDS = [f"n{n}-h{h}-c{ci}-o{co}-x{it}" + ("-vs" if vs else "") for n, h, ci, co, it, vs in WGRAD_E2E]
WGRAD_E2E_PLANTS = ("t_off", "pad")


def wgrad_e2e_inputs(k):
    """([x_i], [d out_i]) NCHW fp32 of case k; d out scaled so that the gradient's entries are of order one."""
    n, h, cin, cout, items, _ = WGRAD_E2E[k]
    return ([params.normal(9900 + 20 * k + i, n, cin, h, h) for i in range(items)],
            [params.normal(9910 + 20 * k + i, n, cout, h, h, scale=(items * n * h * h) ** -0.5) for i in range(items)])


def wgrad_winograd_form(xs, dus, dtype, lost=None, plant=None):
    """The packed (9, Cout, Cin) gradient computed as ops.winograd_wgrad_partial_multi computes it, in `dtype` with the matrices
    rounded to it (float32: the yardstick): V = B^T d B and dM = A dY A^T of item i at the rows [i t, (i + 1) t) of buffers of
    Tp = items * t rounded up to 64 tiles whose padding rows are zero, P = sum over the rows of dM V per position, G^T P G.
      lost = "v" / "dm" (with float64): that buffer as fp32 rounded to 16 significant bits - a lost low bf16 plane of the
             operand the product kernel splits;
      plant = "t_off": the last item's V written at the FIRST item's offset (its own rows stay zero; ValueError with one item);
              "pad":   the padding rows of both buffers hold data, not zeros (ValueError where Tp == items * t)."""
    bt, a, gt = BT[4].to(dtype), A4.to(dtype), GT4.to(dtype)
    items, (n, cout, h, w) = len(xs), dus[0].shape
    t = n * (h // 4) * (w // 4)
    tp = -(-items * t // 64) * 64
    v = torch.zeros(36, tp, xs[0].shape[1], dtype=dtype)
    dm = torch.zeros(36, tp, cout, dtype=dtype)
    if plant == "pad":
        if tp == items * t:
            raise ValueError("no padding rows")
        v[:, items * t:] = params.normal(9997, 36, tp - items * t, v.shape[2]).to(dtype)
        dm[:, items * t:] = params.normal(9998, 36, tp - items * t, cout, scale=float(dus[0].std())).to(dtype)
    if plant == "t_off" and items < 2:
        raise ValueError("one item")
    for i, (x, du) in enumerate(zip(xs, dus)):
        vi = torch.einsum("ia,tcab,jb->ijtc", bt, _patches(x.permute(0, 2, 3, 1), 4, False).to(dtype), bt).reshape(36, t, -1)
        d = du.to(dtype).reshape(n, cout, h // 4, 4, w // 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(-1, cout, 4, 4)
        dm[:, i * t:(i + 1) * t] = torch.einsum("ia,tcab,jb->ijtc", a, d, a).reshape(36, t, cout)
        off = 0 if (plant == "t_off" and i == items - 1) else i * t
        v[:, off:off + t] = vi
    if lost == "v":
        v = round16(v.float()).to(dtype)
    if lost == "dm":
        dm = round16(dm.float()).to(dtype)
    p = torch.bmm(dm.transpose(1, 2), v).reshape(6, 6, cout, -1)
    return torch.einsum("ia,aboc,jb->ijoc", gt, p, gt).reshape(9, cout, -1)


@functools.lru_cache(maxsize=None)
def wgrad_e2e_figures(k):
    """{"e32": the fp32 Winograd form, "e_plane_v" / "e_plane_dm": a lost plane of the product's operands, "e_plane": the smaller,
    "e_plane_dout": d out itself rounded to 16 bits (a figure of the notes, not the cap)} block-wise against
    backward_ref.wgrad_ref(MODE_CONV3) in fp64."""
    from tests.backward_ref import MODE_CONV3, blockwise_err, wgrad_ref
    xs, dus = wgrad_e2e_inputs(k)
    ref = wgrad_ref(MODE_CONV3, xs, None, dus)
    assert blockwise_err(wgrad_winograd_form(xs, dus, torch.float64), ref) < 1e-12
    f = {"e32": blockwise_err(wgrad_winograd_form(xs, dus, torch.float32), ref),
         "e_plane_v": blockwise_err(wgrad_winograd_form(xs, dus, torch.float64, lost="v"), ref),
         "e_plane_dm": blockwise_err(wgrad_winograd_form(xs, dus, torch.float64, lost="dm"), ref),
         "e_plane_dout": blockwise_err(wgrad_ref(MODE_CONV3, xs, None, [round16(d) for d in dus]), ref)}
    f["e_plane"] = min(f["e_plane_v"], f["e_plane_dm"])
    return f


@functools.lru_cache(maxsize=None)
def wgrad_e2e_worst():
    return max(wgrad_e2e_figures(k)["e32"] for k in range(len(WGRAD_E2E)))


def wgrad_e2e_bar(k):
    f = wgrad_e2e_figures(k)
    return bar(f["e32"], wgrad_e2e_worst(), f["e_plane"])
