"""fp64 references of the forward implicit-GEMM convolutions (dvg_amd/csrc/conv_igemm2.hip), written from the mathematics in
plain torch on the CPU, the tile-wise comparison they are read with, references that carry a KNOWN defect, an emulation of the
kernel's accumulation order in fp32, and the cases the host and GPU tests share (tests/test_forward_ref_host.py,
tests/test_gpu_forward_igemm.py; docs/DESIGN_NOTES_forward_tests.md).  The forward counterpart of tests/backward_ref.py.

Everything here is NCHW on the CPU.  An addend is either a tensor of the output's shape or a triple (tensor of blocks * block
images, block, map): image n of the output adds image map[n // block] * block + n % block of the tensor (ops.SharedBlocks)."""
import functools

import torch
import torch.nn.functional as F

from oracle import params
from tests.backward_ref import (MODE_CONV3, MODE_CONV4S2, MODE_CONVT4S2, MODE_NAME, YARDSTICK_RATIO, bar,  # noqa: F401
                                conv_forward, conv_input, round16, sum_bound, weight_shape)

LATENCY, ENERGY = 0, 1          # dvg_set_tile_policy
TILE16_MIN_WGS = {LATENCY: 512, ENERGY: 256}      # plan2: the 8 x 16 tile from this many workgroups of it on


# ---- the reference -----------------------------------------------------------------------------------------------------------
def addend_images(addend, n):
    """The addend as one tensor of n images (module docstring), or None."""
    if addend is None or torch.is_tensor(addend):
        return addend
    t, block, gmap = addend
    assert n == len(gmap) * block, (n, block, gmap)
    return t[[gmap[i // block] * block + i % block for i in range(n)]]


def forward_ref(mode, x, skip, w, upsample, addend=None, dtype=torch.float64):
    """The raw convolution of cat([up(x), skip]) with w (nn layout: Conv2d (Cout, Cin, k, k), ConvTranspose2d (Cin, Cout, k, k))
    plus the addend, in `dtype`: float64 is the reference, float32 torch's own arithmetic at this shape."""
    inp = conv_input(x.to(dtype), None if skip is None else skip.to(dtype), upsample)
    u = conv_forward(mode, inp, w.to(dtype))
    a = addend_images(addend, x.shape[0])
    return u if a is None else u + a.to(dtype)


def tilewise_err(a, ref, ti, th, tw, parity=False):
    """max over every (run of `ti` images, th x tw pixel tile of the OUTPUT, 64-wide Cout block) of max |a - ref| / max |ref|
    WITHIN that block - what one workgroup of conv_igemm2_kernel writes, so a defect confined to one workgroup is measured
    against that block's own magnitude.  parity: the transposed conv - the four parity workgroups of a tile write the pixels
    (2 i + py, 2 j + px) of a 2 th x 2 tw output tile; each parity's pixels are a block of their own.  A NaN / inf in `a`
    comes back as inf."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape and a.dim() == 4, (a.shape, ref.shape)
    if parity:
        return max(tilewise_err(a[:, :, py::2, px::2], ref[:, :, py::2, px::2], ti, th, tw) for py in (0, 1) for px in (0, 1))
    n, c, h, w = ref.shape
    assert h % th == 0 and w % tw == 0, (h, w, th, tw)
    pn, pc = -n % ti, -c % 64
    # absent images / channels are padded with zeros: they add nothing to a block's error or magnitude
    diff = F.pad((a - ref).abs(), (0, 0, 0, 0, 0, pc, 0, pn))
    mag = F.pad(ref.abs(), (0, 0, 0, 0, 0, pc, 0, pn))
    shape = ((n + pn) // ti, ti, (c + pc) // 64, 64, h // th, th, w // tw, tw)
    # a NaN / inf in `a` must not vanish in a max: amax propagates NaN, and inf / x = inf
    d = diff.reshape(shape).amax((1, 3, 5, 7))
    m = mag.reshape(shape).amax((1, 3, 5, 7)).clamp_min(1e-300)
    e = (d / m).max()
    return float("inf") if torch.isnan(e) else float(e)


# ---- references with a known defect ---------------------------------------------------------------------------------------
PLANTS = ("plane_w", "plane_x", "tap", "halo", "chunk", "seam", "tail", "addend_tile")


def plant(kind, mode, x, skip, w, upsample=False, addend=None, *, ti=1, taps=(0, 1)):
    """An fp64 result like forward_ref's that carries a known defect:
      "plane_w":     W rounded to 16 significant bits (a lost low bf16 plane of the weights);
      "plane_x":     x and skip rounded to 16 significant bits;
      "tap":         two taps of W swapped (`taps`: flat indices a * k + b);
      "halo":        the input's border treated as replicated instead of zero;
      "chunk":       the last 16 input channels dropped;
      "seam":        the first 16 skip channels read from x's last 16 (ValueError without a skip);
      "tail":        the images beyond N - N % ti zero (ValueError where N % ti == 0: there is no partly filled tile);
      "addend_tile": every image of a `ti`-image tile takes the addend block of the tile's first image (ValueError unless the
                     addend is shared in blocks smaller than the tile)."""
    n = x.shape[0]
    if kind == "plane_w":
        return forward_ref(mode, x, skip, round16(w), upsample, addend)
    if kind == "plane_x":
        return forward_ref(mode, round16(x), None if skip is None else round16(skip), w, upsample, addend)
    if kind == "tap":
        k = w.shape[-1]
        (a0, b0), (a1, b1) = divmod(taps[0], k), divmod(taps[1], k)
        w2 = w.clone()
        w2[:, :, a0, b0], w2[:, :, a1, b1] = w[:, :, a1, b1], w[:, :, a0, b0]
        return forward_ref(mode, x, skip, w2, upsample, addend)
    if kind == "halo":
        inp = F.pad(conv_input(x.double(), None if skip is None else skip.double(), upsample), (1, 1, 1, 1), mode="replicate")
        if mode == MODE_CONVT4S2:       # output row 2 i - 1 + k of input row i; in the padded tensor row i sits at i + 1
            u = F.conv_transpose2d(inp, w.double(), None, 2, 1)[:, :, 2:-2, 2:-2]
        else:
            u = F.conv2d(inp, w.double(), None, 2 if mode == MODE_CONV4S2 else 1, 0)
        a = addend_images(addend, n)
        return u if a is None else u + a.double()
    if kind == "chunk":
        w2 = w.clone()
        if mode == MODE_CONVT4S2:
            w2[-16:] = 0
        else:
            w2[:, -16:] = 0
        return forward_ref(mode, x, skip, w2, upsample, addend)
    if kind == "seam":
        if skip is None:
            raise ValueError("no concat seam")
        s2 = skip.clone()
        s2[:, :16] = conv_input(x, None, upsample)[:, -16:]
        return forward_ref(mode, x, s2, w, upsample, addend)
    if kind == "tail":
        keep = n - n % ti
        if keep == n:
            raise ValueError("no image tail")
        u = forward_ref(mode, x, skip, w, upsample, addend).clone()
        u[keep:] = 0
        return u
    if kind == "addend_tile":
        if addend is None or torch.is_tensor(addend) or addend[1] >= ti:
            raise ValueError("no tile that spans two addend groups")
        t, block, gmap = addend
        wrong = t[[gmap[(i - i % ti) // block] * block + i % block for i in range(n)]]
        return forward_ref(mode, x, skip, w, upsample, wrong)
    raise ValueError(kind)


# ---- the kernel's accumulation order, emulated in fp32 -----------------------------------------------------------------
def _tap_groups(mode):
    """The order in which the stage loop of conv_igemm2_kernel walks the taps of one 16-channel chunk, as a list of
    (output parity or None, row offset into the 1-padded input, column offset, stride, weight tap (k, l) in the nn layout):
      conv3:    one stage, taps t = 0..8 -> (t / 3, t % 3);
      conv4s2:  four stages, one per INPUT parity g = (alpha, beta) = (g >> 1, g & 1), taps tt = 0..3 ->
                (2 (tt >> 1) + alpha, 2 (tt & 1) + beta)   (Cfg2::PAR4, tap_lds);
      convT4s2: the workgroup of output parity (py, px) runs taps tt = 0..3, reading input pixel (i + py - (tt >> 1),
                j + px - (tt & 1)) for output (2 i + py, 2 j + px): ConvTranspose2d tap (1 - py + 2 (tt >> 1), 1 - px + 2 (tt & 1))."""
    if mode == MODE_CONV3:
        return [(None, t // 3, t % 3, 1, (t // 3, t % 3)) for t in range(9)]
    if mode == MODE_CONV4S2:
        out = []
        for g in range(4):
            for tt in range(4):
                a, b = 2 * (tt >> 1) + (g >> 1), 2 * (tt & 1) + (g & 1)
                out.append((None, a, b, 2, (a, b)))
        return out
    out = []
    for par in range(4):
        py, px = par >> 1, par & 1
        for tt in range(4):
            out.append(((py, px), 1 + py - (tt >> 1), 1 + px - (tt & 1), 1, (1 - py + 2 * (tt >> 1), 1 - px + 2 * (tt & 1))))
    return out


def split_chunks(nchunks, splits):
    """launch2's split of the 16-channel chunks: cps = ceil(nchunks / S), S recomputed so that no split is empty; returns the
    list of (first chunk, end chunk) per split."""
    cps = -(-nchunks // max(splits, 1))
    s = -(-nchunks // cps)
    return [(k * cps, min(nchunks, (k + 1) * cps)) for k in range(s)]


# ---- the launch plan, restated (conv_igemm2.hip: plan2) ---------------------------------------------------------------------
def plan_tile(mode, n, hg, wg, cout, policy):
    """The tile rule on the grid the tiles cover (the output grid of conv3 / conv4s2, the input grid of convT4s2), or None."""
    if (hg, wg) == (4, 4):
        return (4, 4, 4)
    if hg % 8 or wg % 8:
        return None
    par = 4 if mode == MODE_CONVT4S2 else 1
    if wg % 16 == 0 and n * (hg // 8) * (wg // 16) * (cout // 64) * par >= TILE16_MIN_WGS[policy]:
        return (1, 8, 16)
    return (1, 8, 8)


def plan_splitk(wgs, nchunks):
    """choose_splitk: the first pick, then as many splits as are not empty at ceil(nchunks / pick) chunks each."""
    if wgs >= 384 or nchunks < 8:
        return 1
    s = min(512 // wgs, 8, nchunks // 4)
    return 1 if s < 2 else len(split_chunks(nchunks, s))


def plan(mode, n, h, w, cin, cout, policy, pool=False, with_ws=True):
    """dict(tile, wgs per split, tiles, splits, cps, rows) of a launch, or None where there is no tile: splits / cps as the launch
    runs them, rows = the statistics rows (the finish kernel's blocks of max(8, ceil(units / 1024)) pixels - pooled: 2 x 2 quads -
    when K is split, else one per tile)."""
    hg, wg = (h // 2, w // 2) if mode == MODE_CONV4S2 else (h, w)
    tile = plan_tile(mode, n, hg, wg, cout, policy)
    if tile is None:
        return None
    ti, th, tw = tile
    tiles = -(-n // ti) * (hg // th) * (wg // tw) * (4 if mode == MODE_CONVT4S2 else 1)
    wgs, nchunks = tiles * (cout // 64), cin // 16
    s = plan_splitk(wgs, nchunks) if with_ws and tw != 16 else 1      # the 16-wide kernels carry no split-K epilogue
    ho, wo = {MODE_CONV3: (h, w), MODE_CONV4S2: (h // 2, w // 2), MODE_CONVT4S2: (2 * h, 2 * w)}[mode]
    units = n * (ho // 2) * (wo // 2) if pool else n * ho * wo
    upb = max(8, -(-units // 1024))
    return dict(tile=tile, wgs=wgs, tiles=tiles, splits=s, cps=-(-nchunks // s), rows=-(-units // upb) if s > 1 else tiles)


def bf16_planes(t):
    """The exact bf16 triple (h, m, l) of fp32 values, each plane as fp64 (dvg_common.h: bf16x3_split_pair - h = t rounded to
    nearest bf16, m = the remainder rounded to nearest bf16, l the rest)."""
    t = t.float()
    h = t.bfloat16().float()
    r = t - h
    m = r.bfloat16().float()
    return h.double(), m.double(), (r - m).bfloat16().double()


# (activation plane, weight plane) of the six bf16 MFMAs of one (chunk, tap), in the stage loop's order: small terms first
PLANE_PAIRS = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))


def ordered_fp32_ref(mode, x, skip, w, upsample, addend=None, splits=1, per_mfma=False):
    """The convolution in the kernel's summation order: exact products (fp64 holds a 24 x 24-bit product exactly), the 16
    products of one (chunk, tap) summed and rounded to fp32 once (one group), the groups added sequentially into ONE fp32
    accumulator per output in chunk-then-tap order (_tap_groups), every K split from zero, the splits then added in split
    order and the addend last (splitk_finish_kernel; without a split the epilogue adds the addend to the accumulator).
    per_mfma: the product build's finer grain - a group is SIX v_mfma_f32_32x32x16_bf16 (PLANE_PAIRS) on the operands' bf16
    planes (the terms (m,l), (l,m), (l,l) are dropped, as in the kernel), and one such instruction adds its 16 exact plane
    products to the accumulator in TWO steps, k 0-7 then k 8-15, rounding the accumulator to nearest after each
    (tools/ubench/mfma_bf16_rounding.hip: the only one of ten candidate models that is bit-equal on ~ 90 % of random outputs;
    the rest lose low bits of small products inside a step, which this model does not have): twelve roundings of the accumulator
    per group instead of one.
    Returns (result fp32 NCHW, list of the per-split partial sums)."""
    inp32 = F.pad(conv_input(x.float(), None if skip is None else skip.float(), upsample), (1, 1, 1, 1))
    n, cin, hp, wp_ = inp32.shape
    h, wd = hp - 2, wp_ - 2
    cout = w.shape[1] if mode == MODE_CONVT4S2 else w.shape[0]
    ho, wo = {MODE_CONV3: (h, wd), MODE_CONV4S2: (h // 2, wd // 2), MODE_CONVT4S2: (2 * h, 2 * wd)}[mode]
    gh, gw = (h, wd) if mode == MODE_CONVT4S2 else (ho, wo)
    a_planes, w_planes = (bf16_planes(inp32), bf16_planes(w)) if per_mfma else ((inp32.double(),), (w.double(),))
    pairs = PLANE_PAIRS if per_mfma else ((0, 0),)
    groups = _tap_groups(mode)
    partials = []
    for c_lo, c_hi in split_chunks(cin // 16, splits):
        acc = torch.zeros(n, cout, ho, wo, dtype=torch.float32)
        for ch in range(c_lo, c_hi):
            cs = slice(16 * ch, 16 * ch + 16)
            for par, oy, ox, st, (k, l) in groups:
                view = acc if par is None else acc[:, :, par[0]::2, par[1]::2]
                for pa, pb in pairs:
                    win = a_planes[pa][:, cs, oy:oy + st * gh:st, ox:ox + st * gw:st]
                    wt = w_planes[pb][cs, :, k, l].t() if mode == MODE_CONVT4S2 else w_planes[pb][:, cs, k, l]
                    if per_mfma:
                        for half in (slice(0, 8), slice(8, 16)):       # acc = fl(acc + eight exact plane products), twice
                            g = torch.einsum("nkyx,ok->noyx", win[:, half], wt[:, half])
                            view.copy_((view.double() + g).float())
                    else:
                        view += torch.einsum("nkyx,ok->noyx", win, wt).float()     # the group rounded once, then added
        partials.append(acc)
    tot = partials[0].clone()
    for p in partials[1:]:
        tot += p
    a = addend_images(addend, n)
    if a is not None:
        tot += a.float()
    return tot, partials


# ---- the cases (docs/DESIGN_NOTES_forward_tests.md has the table) -----------------------------------------------------------
# shape: conv3 (N, H, W, C1, C2, Cout) on the conv's own grid (x enters at half of it when `up`); conv4s2 (N, H, W, Cin, Cout) on
# the input grid; convT4s2 (N, H, W, C1, C2, Cout) on the input grid.  tile / splits: what plan2 (the tile rule, choose_splitk with its
# rounding of the chunks per split) gives the case under the LATENCY policy, tile_e / splits_e under the ENERGY policy
# (tests/test_forward_ref_host.py asserts both against the library).  addend: (block, map) of a shared addend.
def _case(mode, n, h, w, c1, c2, cout, tile, splits, *, up=False, pool=False, addend=None, tile_e=None, why=""):
    name = f"{MODE_NAME[mode]}-n{n}-{h}x{w}-c{c1}+{c2}-o{cout}" + ("-up" if up else "") + ("-pool" if pool else "") + \
        ("-add" if addend else "")
    tile_e = tile_e or tile
    return dict(name=name, mode=mode, n=n, h=h, w=w, c1=c1, c2=c2, cout=cout, up=up, pool=pool, addend=addend,
                tile={LATENCY: tile, ENERGY: tile_e}, splits={LATENCY: splits, ENERGY: 1 if tile_e[2] == 16 else splits},
                why=why)


_ADD = (2, (0, 1, 0))
FWD_CASES = [
    _case(MODE_CONV3, 1, 8, 8, 16, 0, 64, (1, 8, 8), 1, why="one workgroup, one chunk: prologue = last stage"),
    _case(MODE_CONV3, 2, 8, 16, 48, 0, 64, (1, 8, 8), 1, pool=True, why="non-square, two tile columns, odd chunk count"),
    _case(MODE_CONV3, 1, 8, 8, 16, 16, 64, (1, 8, 8), 1, up=True,
          why="x at 4 x 4 read through the upsampling; concat seam after the first chunk"),
    _case(MODE_CONV3, 2, 8, 8, 208, 0, 64, (1, 8, 8), 3, pool=True, why="13 chunks, 3 splits of 5 / 5 / 3; pooled finish kernel"),
    _case(MODE_CONV3, 1, 16, 16, 48, 96, 128, (1, 8, 8), 2, up=True,
          why="9 chunks, 2 splits of 5 / 4; split 0 holds 3 x chunks and 2 skip chunks"),
    _case(MODE_CONV3, 16, 32, 32, 32, 0, 128, (1, 8, 8), 1, pool=True, tile_e=(1, 8, 16),
          why="256 workgroups of 8 x 16 under the energy policy, 8 x 8 under latency"),
    _case(MODE_CONV3, 6, 8, 8, 32, 0, 64, (1, 8, 8), 1, addend=_ADD, why="addend through the main kernel's epilogue"),
    _case(MODE_CONV3, 6, 8, 8, 128, 0, 64, (1, 8, 8), 2, addend=_ADD, why="8 chunks, 2 splits: addend through the finish kernel"),
    _case(MODE_CONV4S2, 1, 16, 16, 16, 0, 64, (1, 8, 8), 1, why="one 8 x 8 tile, one chunk"),
    _case(MODE_CONV4S2, 1, 8, 8, 32, 0, 64, (4, 4, 4), 1, why="one image in a four-image tile"),
    _case(MODE_CONV4S2, 4, 8, 8, 32, 0, 64, (4, 4, 4), 1, why="four images: the exact fit"),
    _case(MODE_CONV4S2, 5, 8, 8, 32, 0, 64, (4, 4, 4), 1, why="five images: tail of 1"),
    _case(MODE_CONV4S2, 3, 8, 8, 144, 0, 64, (4, 4, 4), 2, why="TI = 4 with 2 splits of 5 / 4; statistics from the finish kernel"),
    _case(MODE_CONV4S2, 1, 16, 48, 16, 0, 64, (1, 8, 8), 1, why="8 x 24 grid: three columns, never 16-wide"),
    _case(MODE_CONV4S2, 3, 16, 16, 64, 0, 64, (1, 8, 8), 1, why="K = 1024: the case of the open question"),
    _case(MODE_CONV4S2, 32, 32, 32, 16, 0, 256, (1, 8, 8), 1, tile_e=(1, 8, 16), why="8 x 16 tile under the energy policy"),
    _case(MODE_CONVT4S2, 1, 8, 8, 16, 0, 64, (1, 8, 8), 1, why="four parity workgroups, one chunk"),
    _case(MODE_CONVT4S2, 5, 4, 4, 16, 16, 64, (4, 4, 4), 1, why="TI = 4, tail of 1, concat"),
    _case(MODE_CONVT4S2, 3, 4, 4, 48, 96, 64, (4, 4, 4), 2, why="2 splits of 5 / 4 straddling the seam"),
    _case(MODE_CONVT4S2, 6, 4, 4, 32, 0, 64, (4, 4, 4), 1, addend=_ADD, why="a 4-image tile spans two groups; tail of 2"),
    _case(MODE_CONVT4S2, 2, 8, 8, 256, 0, 64, (1, 8, 8), 4, why="K = 1024 per parity, for the comparison with conv4s2"),
    _case(MODE_CONVT4S2, 16, 16, 16, 16, 0, 128, (1, 8, 8), 1, tile_e=(1, 8, 16), why="8 x 16 tile under the energy policy"),
    # ragged splits: choose_splitk's first pick (6, 8, 6, 6) would leave a split empty, the launch runs one or two fewer
    _case(MODE_CONV3, 1, 8, 8, 400, 0, 64, (1, 8, 8), 5, why="25 chunks, 5 splits of 5 / 5 / 5 / 5 / 5; not 6"),
    _case(MODE_CONV3, 1, 8, 8, 528, 0, 64, (1, 8, 8), 7, why="33 chunks, 7 splits of 5 / 5 / 5 / 5 / 5 / 5 / 3; not 8"),
    _case(MODE_CONV4S2, 1, 16, 16, 400, 0, 64, (1, 8, 8), 5, why="25 chunks, 5 splits of 5 / 5 / 5 / 5 / 5; not 6"),
    _case(MODE_CONVT4S2, 1, 4, 4, 400, 0, 64, (4, 4, 4), 5, why="25 chunks, 5 splits of 5 / 5 / 5 / 5 / 5; not 6; four workgroups"),
]
CASE_BY_NAME = {c["name"]: c for c in FWD_CASES}
CASE_NAMES = [c["name"] for c in FWD_CASES]
assert len(CASE_BY_NAME) == len(FWD_CASES)
# (case, policy) pairs the GPU tests run: every case under the latency policy, the three 8 x 16 cases under the energy one too
VARIANTS = [(c["name"], LATENCY) for c in FWD_CASES] + \
           [(c["name"], ENERGY) for c in FWD_CASES if c["tile"][ENERGY] != c["tile"][LATENCY]]
VARIANT_IDS = [f"{n}-{'energy' if p else 'latency'}" for n, p in VARIANTS]


def out_hw(case):
    h, w = case["h"], case["w"]
    return {MODE_CONV3: (h, w), MODE_CONV4S2: (h // 2, w // 2), MODE_CONVT4S2: (2 * h, 2 * w)}[case["mode"]]


def fwd_inputs(case):
    """{"x", "skip", "w", "addend"}: the case's operands, NCHW fp32 on the CPU, from params.normal (full 24-bit significands;
    w in the nn layout, scaled to unit-variance outputs); addend None or the (tensor, block, map) triple."""
    k = FWD_CASES.index(case)
    mode, n, h, w, c1, c2, cout = (case[f] for f in ("mode", "n", "h", "w", "c1", "c2", "cout"))
    hx, wx = (h // 2, w // 2) if case["up"] else (h, w)
    seed = 9000 + 100 * k
    taps = 9 if mode == MODE_CONV3 else (16 if mode == MODE_CONV4S2 else 4)
    out = {"x": params.normal(seed, n, c1, hx, wx), "skip": params.normal(seed + 1, n, c2, h, w) if c2 else None,
           "w": params.normal(seed + 2, *weight_shape(mode, c1 + c2, cout), scale=(taps * (c1 + c2)) ** -0.5), "addend": None}
    if case["addend"]:
        block, gmap = case["addend"]
        out["addend"] = (params.normal(seed + 3, (max(gmap) + 1) * block, cout, *out_hw(case)), block, gmap)
    return out


def case_args(case):
    i = fwd_inputs(case)
    return (case["mode"], i["x"], i["skip"], i["w"], case["up"], i["addend"])


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """The fp64 reference, torch's fp32 result and the two lost-plane results, computed once per case and shared (the tensors are
    not to be modified)."""
    case = CASE_BY_NAME[name]
    args = case_args(case)
    return {"ref": forward_ref(*args), "f32": forward_ref(*args, dtype=torch.float32),
            "plane_w": plant("plane_w", *args), "plane_x": plant("plane_x", *args)}


@functools.lru_cache(maxsize=None)
def case_ordered_parts(name, policy=LATENCY, per_mfma=False):
    """(result, per-split partial sums) of the emulation with the split the policy gives the case."""
    case = CASE_BY_NAME[name]
    return ordered_fp32_ref(*case_args(case), splits=case["splits"][policy], per_mfma=per_mfma)


def case_ordered(name, policy=LATENCY, per_mfma=False):
    return case_ordered_parts(name, policy, per_mfma)[0]


def case_err(name, policy, a):
    """tilewise_err of `a` against the case's fp64 reference at the tile the policy gives the case."""
    case = CASE_BY_NAME[name]
    return tilewise_err(a, case_ref(name)["ref"], *case["tile"][policy], parity=case["mode"] == MODE_CONVT4S2)


# Which measured reference is the fp32 yardstick of a mode (docs/DESIGN_NOTES_forward_tests.md, "The open question"): "torch" -
# torch's fp32 CPU convolution -, "ordered" - ordered_fp32_ref, fp32 in the kernel's summation order with one rounding per
# (chunk, tap) - or "mfma" - the same with the accumulator rounded where the MFMAs round it.  conv3 and conv4s2 walk all of K in
# one chain and sit at 2 ... 3 x torch, which "mfma" reproduces (to the last digit at most cases); the transposed conv's chains
# are a quarter as long (four taps per parity) and it passes torch's bar.
YARDSTICK = {MODE_CONV3: "mfma", MODE_CONV4S2: "mfma", MODE_CONVT4S2: "torch"}


@functools.lru_cache(maxsize=None)
def case_figures(name, policy=LATENCY):
    """{"e32": torch's fp32 error, "e_ord": the emulation's, "e_y": the mode's yardstick of the two, "e_plane_w", "e_plane_x",
    "e_plane": the smaller of the two lost planes} - all tile-wise against fp64 at the (case, policy)'s tile."""
    r = case_ref(name)
    f = {"e32": case_err(name, policy, r["f32"]), "e_ord": case_err(name, policy, case_ordered(name, policy)),
         "e_mfma": case_err(name, policy, case_ordered(name, policy, True)),
         "e_plane_w": case_err(name, policy, r["plane_w"]), "e_plane_x": case_err(name, policy, r["plane_x"])}
    f["e_plane"] = min(f["e_plane_w"], f["e_plane_x"])
    f["e_y"] = f[{"torch": "e32", "ordered": "e_ord", "mfma": "e_mfma"}[YARDSTICK[CASE_BY_NAME[name]["mode"]]]]
    return f


@functools.lru_cache(maxsize=None)
def mode_worst(mode):
    """The yardstick's worst error over the mode's (case, policy) pairs."""
    return max(case_figures(n, p)["e_y"] for n, p in VARIANTS if CASE_BY_NAME[n]["mode"] == mode)


def case_bar(name, policy=LATENCY):
    f = case_figures(name, policy)
    return bar(f["e_y"], mode_worst(CASE_BY_NAME[name]["mode"]), f["e_plane"])
