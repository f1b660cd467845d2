"""fp64 references of the convolutions' backward kernels, written from the mathematics in plain torch on the CPU, the
block-wise comparison they are read with, references that carry a KNOWN defect, and the cases the host and GPU tests share
(tests/test_backward_ref_host.py, tests/test_gpu_wgrad.py; docs/DESIGN_NOTES_backward_tests.md).

Packed slab layout (wgrad_finish_kernel in dvg_amd/csrc/backward.hip): slab[tap = a * KW + b][co][ci] is
  kind 0 (Conv2d weight (Cout, Cin, KH, KW)):           dW[co][ci][a][b]
  kind 1 (ConvTranspose2d weight (Cin, Cout, KH, KW)):  dW[ci][co][KH-1-a][KW-1-b]     (taps flipped)
MODE_CONV3 and MODE_CONV4S2 are of kind 0, MODE_CONVT4S2 of kind 1."""
import functools

import torch
import torch.nn.functional as F

from oracle import params

MODE_CONV3, MODE_CONV4S2, MODE_CONVT4S2 = 0, 1, 2
MODE_NAME = {MODE_CONV3: "conv3", MODE_CONV4S2: "conv4s2", MODE_CONVT4S2: "convT4s2"}
KSIZE = {MODE_CONV3: 3, MODE_CONV4S2: 4, MODE_CONVT4S2: 4}
U32 = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)


# ---- the dense convolutions' weight gradient -------------------------------------------------------------------------------
def conv_input(x, skip, upsample):
    """cat([upsample(x), skip]) along the channels: what the conv of a block reads."""
    inp = F.interpolate(x, scale_factor=2, mode="nearest") if upsample else x
    return inp if skip is None else torch.cat([inp, skip], 1)


def conv_forward(mode, inp, w):
    if mode == MODE_CONV3:
        return F.conv2d(inp, w, None, 1, 1)
    if mode == MODE_CONV4S2:
        return F.conv2d(inp, w, None, 2, 1)
    return F.conv_transpose2d(inp, w, None, 2, 1)


def weight_shape(mode, cin, cout):
    k = KSIZE[mode]
    return (cin, cout, k, k) if mode == MODE_CONVT4S2 else (cout, cin, k, k)


def pack_slab(mode, dw):
    """The nn-layout weight gradient as the packed (taps, Cout, Cin) slab (module docstring)."""
    k = KSIZE[mode]
    if mode == MODE_CONVT4S2:      # (Cin, Cout, kh, kw), taps flipped
        return dw.flip(2, 3).permute(2, 3, 1, 0).reshape(k * k, dw.shape[1], dw.shape[0])
    return dw.permute(2, 3, 0, 1).reshape(k * k, dw.shape[0], dw.shape[1])


def wgrad_ref(mode, xs, skips, dus, upsample=False, dtype=torch.float64):
    """Packed (taps, Cout, Cin) weight gradient summed over the items (x, skip, d out), by autograd through F.conv2d /
    F.conv_transpose2d on cat([upsample(x), skip]) in `dtype`: float64 is the reference, float32 the yardstick (what plain
    fp32 arithmetic costs at this shape)."""
    cin = xs[0].shape[1] + (0 if skips is None else skips[0].shape[1])
    w = torch.zeros(weight_shape(mode, cin, dus[0].shape[1]), dtype=dtype, requires_grad=True)
    total = None
    for i, (x, du) in enumerate(zip(xs, dus)):
        inp = conv_input(x.to(dtype), None if skips is None else skips[i].to(dtype), upsample)
        t = (conv_forward(mode, inp, w) * du.to(dtype)).sum()
        total = t if total is None else total + t
    total.backward()
    return pack_slab(mode, w.grad)


def blockwise_err(a, ref, tile=64):
    """max over every (tap, 64-wide co tile, 64-wide ci tile) of max |a - ref| / max |ref| WITHIN that block: an error confined
    to one tap or one tile is measured against that block's own magnitude, not diluted by the whole tensor's maximum."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape and a.dim() == 3, (a.shape, ref.shape)
    t, co, ci = ref.shape
    pco, pci = -co % tile, -ci % tile
    diff = F.pad((a - ref).abs(), (0, pci, 0, pco))
    mag = F.pad(ref.abs(), (0, pci, 0, pco))
    # a NaN / inf in `a` must not vanish in a max: amax propagates NaN, and inf / x = inf
    shape = (t, (co + pco) // tile, tile, (ci + pci) // tile, tile)
    d = diff.reshape(shape).amax((2, 4))
    m = mag.reshape(shape).amax((2, 4)).clamp_min(1e-300)
    e = (d / m).max()
    return float("inf") if torch.isnan(e) else float(e)


def round16(t):
    """fp32 values rounded (to nearest) to 16 significant bits: what is left of an operand whose low bf16 plane is lost (the
    h and m planes of a bf16 triple hold 8 significant bits each)."""
    i = t.detach().float().contiguous().view(torch.int32)
    return ((i + 0x80) & ~0xFF).view(torch.float32)


PLANTS = ("plane", "pixel", "tap", "tail")


def plant(kind, mode, xs, skips, dus, upsample=False, *, ti=1, taps=(0, 1)):
    """An fp64 slab like wgrad_ref's that carries a known defect:
      "plane": d out rounded to 16 significant bits (a lost low bf16 plane of one operand);
      "pixel": the last output pixel of the last image of the last item dropped;
      "tap":   the slabs of two taps swapped;
      "tail":  the images beyond N - N % ti dropped (a kernel that forgets the partly filled last tile of `ti` images);
               ValueError where N % ti == 0: there is no such tile."""
    if kind == "plane":
        return wgrad_ref(mode, xs, skips, [round16(d) for d in dus], upsample)
    if kind == "pixel":
        last = dus[-1].clone()
        last[-1, :, -1, -1] = 0
        return wgrad_ref(mode, xs, skips, list(dus[:-1]) + [last], upsample)
    if kind == "tap":
        ref = wgrad_ref(mode, xs, skips, dus, upsample).clone()
        ref[list(taps)] = ref[list(taps)[::-1]]
        return ref
    if kind == "tail":
        n = xs[0].shape[0]
        keep = n - n % ti
        if keep == n:
            raise ValueError("no image tail")
        if keep == 0:
            return torch.zeros_like(wgrad_ref(mode, xs, skips, dus, upsample))
        return wgrad_ref(mode, [x[:keep] for x in xs], None if skips is None else [s[:keep] for s in skips],
                         [d[:keep] for d in dus], upsample)
    raise ValueError(kind)


YARDSTICK_RATIO = 1.5     # tests.common.yardstick's ratio


def bar(e32_case, e32_worst_kind, e_plane_case):
    """The largest block-wise error a kernel may show at one case: 1.5 x the fp32 yardstick's own error there, but at least the
    yardstick's worst error over the kind's cases (so a case where torch's fp32 lands unusually close does not fail a correct
    kernel), and never more than half the error of a lost bf16 plane - that cap is a condition: the bar must reject one."""
    return min(max(YARDSTICK_RATIO * e32_case, e32_worst_kind), 0.5 * e_plane_case)


# ---- the cases (docs/DESIGN_NOTES_backward_tests.md has the table) -----------------------------------------------------
# n, h: images and the side of the grid named in the mode's case list (MODE_CONV3: the conv's grid - x enters at half of it
# when `up`; MODE_CONV4S2 / MODE_CONVT4S2: the input grid); tile: the (TI, TH, TW) wgrad_tile picks; splits: the K-split count;
# split_tail: the last split owns fewer tiles than the others; straddle: one split's tiles come from two items.
def _case(mode, n, h, c1, c2, cout, tile, splits, *, up=False, items=1, split_tail=False, straddle=False, why=""):
    name = f"{MODE_NAME[mode]}-n{n}-h{h}-c{c1}+{c2}-o{cout}" + ("-up" if up else "") + (f"-x{items}" if items > 1 else "")
    return dict(name=name, mode=mode, n=n, h=h, c1=c1, c2=c2, cout=cout, up=up, items=items, tile=tile, splits=splits,
                split_tail=split_tail, straddle=straddle, why=why)


WGRAD_CASES = [
    _case(MODE_CONV3, 3, 8, 64, 0, 64, (1, 8, 8), 3, why="baseline"),
    _case(MODE_CONV3, 2, 16, 64, 64, 64, (1, 8, 8), 8, up=True, why="x half read at half resolution, skip at full"),
    _case(MODE_CONV3, 1, 8, 64, 192, 128, (1, 8, 8), 1, why="the ci tile that first crosses from x into skip"),
    _case(MODE_CONV3, 9, 8, 512, 0, 512, (1, 8, 8), 5, split_tail=True, why="9 tiles over 5 splits, the last owns one"),
    _case(MODE_CONV3, 5, 8, 512, 0, 512, (1, 8, 8), 8, items=3, split_tail=True, straddle=True,
          why="15 tiles, two per split: a split straddles items 0 and 1"),
    _case(MODE_CONV4S2, 3, 8, 64, 0, 128, (2, 4, 4), 2, why="output grid 4x4, TI = 2, odd N"),
    _case(MODE_CONV4S2, 1, 8, 128, 0, 64, (2, 4, 4), 1, why="a single image in a two-image tile"),
    _case(MODE_CONV4S2, 2, 16, 64, 0, 64, (1, 4, 8), 4, why="tile 1x4x8"),
    _case(MODE_CONV4S2, 2, 32, 64, 0, 128, (1, 4, 8), 32, items=2, why="both tap groups, two items"),
    _case(MODE_CONVT4S2, 5, 4, 128, 0, 64, (4, 4, 4), 2, why="TI = 4: tail of 1"),
    _case(MODE_CONVT4S2, 2, 4, 64, 64, 64, (4, 4, 4), 1, why="TI = 4: tail of 2, concat"),
    _case(MODE_CONVT4S2, 1, 4, 64, 0, 64, (4, 4, 4), 1, why="TI = 4: a single image"),
    _case(MODE_CONVT4S2, 4, 4, 64, 0, 64, (4, 4, 4), 1, why="TI = 4: the exact fit"),
    _case(MODE_CONVT4S2, 3, 8, 64, 64, 128, (1, 8, 8), 3, why="tile 1x8x8 with concat"),
    _case(MODE_CONVT4S2, 7, 4, 64, 0, 64, (4, 4, 4), 6, items=3, why="item boundary after a partly filled 4-image tile"),
]
CASE_BY_NAME = {c["name"]: c for c in WGRAD_CASES}
CASE_NAMES = [c["name"] for c in WGRAD_CASES]
assert len(CASE_BY_NAME) == len(WGRAD_CASES)


def wgrad_inputs(case):
    """(xs, skips, dus): the case's operands, NCHW fp32 on the CPU, from params.normal (full 24-bit significands)."""
    k = WGRAD_CASES.index(case)
    n, h, c1, c2, cout, mode = case["n"], case["h"], case["c1"], case["c2"], case["cout"], case["mode"]
    hx = h // 2 if case["up"] else h
    ho = {MODE_CONV3: h, MODE_CONV4S2: h // 2, MODE_CONVT4S2: 2 * h}[mode]
    xs, skips, dus = [], [], []
    for i in range(case["items"]):
        seed = 7000 + 100 * k + 10 * i
        xs.append(params.normal(seed, n, c1, hx, hx))
        skips.append(params.normal(seed + 1, n, c2, h, h) if c2 else None)
        dus.append(params.normal(seed + 2, n, cout, ho, ho))
    return xs, (skips if c2 else None), dus


@functools.lru_cache(maxsize=None)
def case_figures(name):
    """{"ref": the fp64 slab, "e32": the fp32 yardstick's block-wise error, "e_plane": that of the planted lost plane}, computed
    once per case and shared (the tensors are not to be modified)."""
    case = CASE_BY_NAME[name]
    xs, skips, dus = wgrad_inputs(case)
    ref = wgrad_ref(case["mode"], xs, skips, dus, case["up"])
    e32 = blockwise_err(wgrad_ref(case["mode"], xs, skips, dus, case["up"], dtype=torch.float32), ref)
    e_plane = blockwise_err(plant("plane", case["mode"], xs, skips, dus, case["up"]), ref)
    return {"ref": ref, "e32": e32, "e_plane": e_plane}


@functools.lru_cache(maxsize=None)
def kind_worst_e32(mode):
    return max(case_figures(c["name"])["e32"] for c in WGRAD_CASES if c["mode"] == mode)


def case_bar(name):
    f = case_figures(name)
    return bar(f["e32"], kind_worst_e32(CASE_BY_NAME[name]["mode"]), f["e_plane"])


# ---- plain fp64 references of the small kernels -----------------------------------------------------------------------
def sum_bound(terms_abs_sum, n):
    """|fp32 sum of n terms in ANY order - exact sum| <= gamma_(n-1) * sum |v|, gamma_k = k u / (1 - k u) (every one of the n - 1
    additions rounds a partial sum that is at most sum |v| in magnitude)."""
    k = max(n - 1, 0) * U32
    return terms_abs_sum * (k / (1.0 - k))


def upsample2x_bwd_ref(dxu):
    """Adjoint of the nearest x2 upsampling: dx[n][c][y][x] = the sum of the 2x2 block of dxu (NCHW); (dx, sum of |terms|)."""
    n, c, h2, w2 = dxu.shape
    v = dxu.double().reshape(n, c, h2 // 2, 2, w2 // 2, 2)
    return v.sum((3, 5)), v.abs().sum((3, 5))


def group_sum_ref(src, gmap, blocks):
    """dst[b] = sum over the groups g with gmap[g] == b of src[g]; src: (groups * block, ...); (dst, sum of |terms|, terms per
    block)."""
    g = len(gmap)
    s = src.double().reshape((g, src.shape[0] // g) + tuple(src.shape[1:]))
    out = torch.zeros((blocks,) + tuple(s.shape[1:]), dtype=torch.float64)
    mag = torch.zeros_like(out)
    for i, b in enumerate(gmap):
        out[b] += s[i]
        mag[b] += s[i].abs()
    shape = (blocks * s.shape[1],) + tuple(src.shape[1:])
    return out.reshape(shape), mag.reshape(shape), [list(gmap).count(b) for b in range(blocks)]


def k4_unpack(dk4p):
    """dK4 (Cout, C1, 4, 4) from its packed transposed-conv slab (16, Cout, C1): tap (3 - r) * 4 + (3 - s) holds dK4[..][r][s]."""
    _, cout, c1 = dk4p.shape
    return dk4p.reshape(4, 4, cout, c1).flip(0, 1).permute(2, 3, 0, 1)


def k4_of_w3(w):
    """K4 = W (*) ones(2x2), (Cout, C1, 4, 4): nearest x2 upsampling then a 3x3 conv (pad 1) is the stride-2 transposed conv with
    this kernel; per axis, tap t of the 3x3 kernel lands on taps 2 - t and 3 - t of the 4-tap one."""
    k4 = torch.zeros(w.shape[:2] + (4, 4), dtype=torch.float64)
    for ty in range(3):
        for tx in range(3):
            k4[:, :, 2 - ty:4 - ty, 2 - tx:4 - tx] += w.double()[:, :, ty:ty + 1, tx:tx + 1]
    return k4


def k4_to_w3_ref(dk4p):
    """dW3 (Cout, C1, 3, 3) = the 2x2 window sums of dK4 - the adjoint of k4_of_w3; (dW3, sum of |terms|)."""
    dk4 = k4_unpack(dk4p.double())
    out = torch.zeros(dk4.shape[:2] + (3, 3), dtype=torch.float64)
    mag = torch.zeros_like(out)
    for ty in range(3):
        for tx in range(3):
            win = dk4[:, :, 2 - ty:4 - ty, 2 - tx:4 - tx]
            out[:, :, ty, tx] = win.sum((2, 3))
            mag[:, :, ty, tx] = win.abs().sum((2, 3))
    return out, mag


ACT_NONE, ACT_LRELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3


def act_bwd_ref(dy, y, act, slope=0.2):
    """dy * act'(pre-activation) with the derivative evaluated from the OUTPUT y, as the kernels do, in fp64."""
    dy, y = dy.double(), y.double()
    if act == ACT_LRELU:
        # the kernel's slope is an fp32 argument
        return dy * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, float(torch.tensor(slope, dtype=torch.float32))))
    if act == ACT_TANH:
        return dy * (1 - y * y)
    if act == ACT_SIGMOID:
        return dy * (y * (1 - y))
    return dy


def ulp32(t):
    """The spacing of fp32 numbers at |t| (t: fp64 tensor of fp32-representable magnitudes), 2^-149 at 0."""
    t = t.double().abs()
    _, e = torch.frexp(t)
    e = torch.where(t == 0, torch.full_like(e, -149), (e - 24).clamp_min(-149))
    return torch.ldexp(torch.ones_like(t), e)


def reduce_partials_ref(partial):
    """(sum over the slabs, sum of |terms|) of partial (S, ...)."""
    p = partial.double()
    return p.sum(0), p.abs().sum(0)


def wgrad_finish_ref(partial, dst0, kind, kh, kw, ctot, c_lo, beta):
    """dvg_wgrad_finish in fp64: (expected dst, sum of |terms| in dst's layout (0 outside the slice), slice mask).  partial:
    (S, kh * kw, Cout, Cin); dst0: the destination's contents before the call - kind 0: (Cout, Ctot, kh, kw), kind 1:
    (Ctot, Cout, kh, kw), kind 2: (kh * kw, Cout, Cin).  With beta == 0 the old contents of the slice do not enter."""
    _, taps, cout, cin = partial.shape
    tot, mag = reduce_partials_ref(partial)
    if kind == 0:
        place = lambda t: t.reshape(kh, kw, cout, cin).permute(2, 3, 0, 1)                      # noqa: E731
        index = (slice(None), slice(c_lo, c_lo + cin))
    elif kind == 1:
        place = lambda t: t.reshape(kh, kw, cout, cin).flip(0, 1).permute(3, 2, 0, 1)           # noqa: E731
        index = (slice(c_lo, c_lo + cin),)
    else:
        place = lambda t: t                                                                     # noqa: E731
        index = (slice(None),)
    out = dst0.double().clone()
    terms = torch.zeros_like(out)
    mask = torch.zeros(out.shape, dtype=torch.bool)
    mask[index] = True
    old = out[index].clone()
    if beta == 0:
        out[index] = place(tot)
        terms[index] = place(mag)
    else:
        b = float(torch.tensor(beta, dtype=torch.float32))
        out[index] = b * old + place(tot)
        terms[index] = (b * old).abs() + place(mag)
    return out, terms, mask


def wgrad_thin_ref(inp, dout, ks, dtype=torch.float64):
    """dW (C, nc, ks, ks) of the thin layers: the weight gradient of F.conv2d(inp (N, nc, Hi, Wi), W, stride ks == 4 ? 2 : 1,
    pad 1) under d out (N, C, Ho, Wo) - and, by adjointness, of the last transposed layers with the roles swapped."""
    w = torch.zeros(dout.shape[1], inp.shape[1], ks, ks, dtype=dtype, requires_grad=True)
    (F.conv2d(inp.to(dtype), w, None, 2 if ks == 4 else 1, 1) * dout.to(dtype)).sum().backward()
    return w.grad
