"""Block backward WITH its gradient routing against fp64 autograd of the plain composition: every block kind through
autograd.conv_block_autograd / last_layer_autograd / dense_block_autograd in train mode, every gradient (x, skip, weight,
gamma, beta; the last layers' bias), and for the concat blocks the three ways the decoder reaches them - plain concat, the
shared skip half of several decoder calls (autograd._SkipHalf, du_sum, the K4 form of upsample + conv3x3), and the shared
skip BLOCKS of the time-batched calls (ops.SharedBlocks, ops.group_sum).

Reference: the same composition in torch on the CPU in fp64; LeakyReLU branches taken from the sign of the HIP forward's
output (as oracle.forced_kinks does: an element within rounding of 0 cannot then move a gradient entry by percents).  The
same composition in fp32 is the yardstick (_compare): a HIP gradient may be at most 1.5 x as far from fp64 as that - floored
at the worst fp32 error among the block's own gradients, and for the conv blocks' matrix-pipe gradients capped at half the
error of a lost bf16 plane -, and the weight gradient's element-wise error (floor 1e-2 of its largest entry) at most 10 x its
fp32 figure: a wrong small entry hides in a max-norm.  The conv bias feeds a batch-statistics BatchNorm: its gradient is
analytically 0 and only asserted small.

d x / d skip of the conv blocks get the ratio 4, not 1.5 (MI355X, product build; e_hip / e_32 against fp64):
  convT4s2 (3, 8, 128, 128, 64) shared half   d x 1.20e-6 / 4.85e-7   d skip 8.27e-7 / 4.14e-7   (e_plane 7.2e-6 / 6.3e-6)
  convT4s2 (3, 8, 128, 128, 64) shared blocks d x 8.75e-7 / 3.57e-7   d skip 1.12e-6 / 3.44e-7
  conv3-up (2, 16, 64, 64, 64) shared blocks  d x 8.20e-7 / 2.28e-7   d skip 8.42e-7 / 3.32e-7   (the largest ratio: 3.6)
They are made by the FORWARD implicit-GEMM kernels run on d u (fused.BLOCKS[..].dgrad), and those - alone, on exact operands,
K = 576 / 1024 - are 2.2 - 2.5 x torch's fp32 error from fp64 (2.3 - 3.0 x in the native-f32-MFMA build: the accumulation
order, not the bf16 split; the weight-gradient kernel and the transposed-conv forward are at 0.1 - 0.8 x).  4 is the bar
the suite already holds these kernels to against the fp32 oracle (test_vgg_backward_free_running_noise_is_the_fp32_noise); the
cap keeps it meaningful: every such bar stays below half of what a lost plane costs (5.8e-6 ... 7.3e-6 here), so a dropped
cross term, a lost pixel or a wrong route (percents) cannot pass.  docs/DESIGN_NOTES_backward_tests.md has every figure."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import params
from tests import backward_ref as br
from tests.common import dev, rel_err, rel_err_elem

pytestmark = pytest.mark.gpu

MODE = {"conv3": br.MODE_CONV3, "conv4s2": br.MODE_CONV4S2, "convT4s2": br.MODE_CONVT4S2}


def nhwc_leaf(t):
    return t.to(dev()).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)


def _fill(conv, bn, seed):
    with torch.no_grad():
        conv.weight.copy_(params.normal(seed, *conv.weight.shape, scale=0.05))
        conv.bias.copy_(params.normal(seed + 1, *conv.bias.shape, scale=0.1))
        if bn is not None:
            bn.weight.copy_(1 + 0.1 * params.normal(seed + 2, *bn.weight.shape))
            bn.bias.copy_(0.1 * params.normal(seed + 3, *bn.bias.shape))
    p = {"w": conv.weight.detach().clone(), "b": conv.bias.detach().clone()}
    if bn is not None:
        p.update(g=bn.weight.detach().clone(), be=bn.bias.detach().clone())
    return p


def _lrelu_forced(z, y_hip):
    one = torch.ones((), dtype=z.dtype)
    return z * torch.where(y_hip.to(z.dtype) > 0, one, 0.2 * one)


def _reference(compose, p, leaves, dtype, trainable=("w", "g", "be")):
    """Gradients of compose(P, L) (a scalar) in `dtype`: P the parameters (those in `trainable` differentiated), L the leaves."""
    P = {k: v.to(dtype).clone().requires_grad_(k in trainable) for k, v in p.items()}
    L = {k: v.to(dtype).clone().requires_grad_(True) for k, v in leaves.items()}
    out = compose(P, L)
    out["loss"].backward()
    grads = {k: v.grad for k, v in list(P.items()) + list(L.items()) if v.grad is not None}
    return grads, [y.detach() for y in out["ys"]]


DATA_RATIO = 4.0      # d x / d skip of the conv blocks: see _compare and docs/DESIGN_NOTES_backward_tests.md
GEMM_MADE = ("w", "x", "skip")


def _compare(tag, hip, r32, r64, *, plane=None, data_ratio=1.5, slices=None, wkeys=("w",)):
    """Every gradient k: HIP's error against fp64 (tests.common.rel_err) at most
        max(ratio_k * e32_k, floor)  [, and at most 0.5 * e_plane_k where `plane` has k]
    e32_k: the fp32 composition's own error; ratio_k = 1.5 (tests.common.yardstick's), `data_ratio` for d x / d skip; floor: the
    worst e32 among this block's gradients (tests.backward_ref.bar's floor: a tensor where torch's fp32 lands unusually close -
    a one-element bias gradient, a 64-entry d gamma - does not fail a correct kernel); plane: the gradients of the fp64
    composition with x, skip and W rounded to 16 significant bits (a lost low bf16 plane of one operand of every product): the
    bar of a gradient that a matrix-pipe kernel makes must reject that, whatever the yardstick says.
    Every figure is printed before anything is asserted."""
    assert set(r64) <= set(hip), (sorted(r64), sorted(hip))
    hip, r32, r64 = dict(hip), dict(r32), dict(r64)
    plane = None if plane is None else dict(plane)
    for name, (k, sl) in (slices or {}).items():
        hip[name], r32[name], r64[name] = hip[k][sl], r32[k][sl], r64[k][sl]
        if plane is not None:
            plane[name] = plane[k][sl]
    e32 = {k: rel_err(r32[k], r64[k]) for k in r64}
    floor = max(e32.values())
    bad = []
    for k in r64:
        e_hip = rel_err(hip[k], r64[k])
        base = k.split("[")[0]
        b = max((data_ratio if base in ("x", "skip") else 1.5) * e32[k], floor)
        e_pl = rel_err(plane[k], r64[k]) if plane is not None and base in GEMM_MADE else None
        if e_pl is not None:
            b = min(b, 0.5 * e_pl)
        print(f"{tag} d{k}: e_hip {e_hip:.2e} e_32 {e32[k]:.2e} ratio {e_hip / max(e32[k], 1e-30):.2f} "
              f"e_plane {'-' if e_pl is None else format(e_pl, '.2e')} bar {b:.2e}")
        if not e_hip <= b:
            bad.append((k, e_hip, e32[k], e_pl, b))
    for k in wkeys:
        e_hip, e_32 = rel_err_elem(hip[k], r64[k], floor=1e-2), rel_err_elem(r32[k], r64[k], floor=1e-2)
        print(f"{tag} d{k} element-wise (floor 1e-2): HIP {e_hip:.2e} fp32 {e_32:.2e}")
        if not e_hip <= 10 * e_32:
            bad.append((k + " element-wise", e_hip, e_32, None, 10 * e_32))
    assert not bad, (tag, bad)


def _bias_grad_is_small(conv, dw):
    assert float(conv.bias.grad.abs().max()) < 1e-3 * float(dw.abs().max()) + 1e-6      # ~0 under batch statistics


# ---- conv + BatchNorm + LeakyReLU blocks -------------------------------------------------------------------------------------
def _block_compose(kind, up, calls, gys, y_hips):
    """loss = sum over the calls of <LeakyReLU(BN_train(conv(cat(up(x), skip)) + b)), gy>; calls(L) -> [(x, skip), ...]."""
    def compose(P, L):
        ys, loss = [], 0
        for (x, skip), gy, yh in zip(calls(L), gys, y_hips):
            u = br.conv_forward(MODE[kind], br.conv_input(x, skip, up), P["w"]) + P["b"].view(1, -1, 1, 1)
            y = _lrelu_forced(F.batch_norm(u, None, None, P["g"], P["be"], True, 0.1, 1e-5), yh)
            ys.append(y)
            loss = loss + (y * gy.to(y.dtype)).sum()
        return {"loss": loss, "ys": ys}
    return compose


def _make_block(kind, cin, cout, seed):
    conv = {"conv3": lambda: nn.Conv2d(cin, cout, 3, 1, 1), "conv4s2": lambda: nn.Conv2d(cin, cout, 4, 2, 1),
            "convT4s2": lambda: nn.ConvTranspose2d(cin, cout, 4, 2, 1)}[kind]()
    bn = nn.BatchNorm2d(cout)
    p = _fill(conv, bn, seed)
    return conv.to(dev()), bn.to(dev()).train(), p


def _run_block(tag, kind, up, conv, bn, p, leaves, hip_forward, calls, gys, *, start_grads=False, slices=None):
    """hip_forward(D) -> list of HIP outputs from the device leaves D; calls(L) -> the reference's [(x, skip), ...]."""
    D = {k: nhwc_leaf(v) for k, v in leaves.items()}
    ys = hip_forward(D)
    y_hips = [y.detach().cpu() for y in ys]
    r64, y64 = _reference(_block_compose(kind, up, calls, gys, y_hips), p, leaves, torch.float64)
    r32, _ = _reference(_block_compose(kind, up, calls, gys, y_hips), p, leaves, torch.float32)
    plane, _ = _reference(_block_compose(kind, up, calls, gys, y_hips), dict(p, w=br.round16(p["w"])),
                          {k: br.round16(v) for k, v in leaves.items()}, torch.float64)
    for yh, yr in zip(y_hips, y64):
        assert rel_err(yh, yr) < 1e-4
    g0 = {}
    if start_grads:          # `.grad` already holds something: the in-place finish adds to it, autograd accumulates on top of it
        for i, (k, prm) in enumerate((("w", conv.weight), ("g", bn.weight), ("be", bn.bias))):
            g0[k] = 0.25 * float(r64[k].abs().max()) * params.normal(9900 + i, *prm.shape)
            prm.grad = g0[k].to(dev())
            r64[k], r32[k], plane[k] = r64[k] + g0[k].double(), r32[k] + g0[k], plane[k] + g0[k].double()
    sum((y * gy.to(dev())).sum() for y, gy in zip(ys, gys)).backward()
    torch.cuda.synchronize()
    hip = {k: v.grad for k, v in D.items()}
    hip.update(w=conv.weight.grad, g=bn.weight.grad, be=bn.bias.grad)
    assert all(v is not None for v in hip.values())
    _compare(tag, hip, r32, r64, plane=plane, data_ratio=DATA_RATIO, slices=slices)
    _bias_grad_is_small(conv, r64["w"] - (g0["w"].double() if g0 else 0.0))


@pytest.mark.parametrize("N,H,Cin,Cout", [(3, 16, 64, 128), (3, 8, 256, 512)])
def test_conv4s2_block_backward(N, H, Cin, Cout):
    from dvg_amd import autograd as ag, ops
    conv, bn, p = _make_block("conv4s2", Cin, Cout, 9000 + H)
    leaves = {"x": params.normal(9010 + H, N, Cin, H, H)}
    gys = [params.normal(9011 + H, N, Cout, H // 2, H // 2)]
    _run_block(f"conv4s2 {(N, H, Cin, Cout)}", "conv4s2", False, conv, bn, p, leaves,
               lambda D: [ag.conv_block_autograd("conv4s2", conv, bn, D["x"], None, act=ops.ACT_LRELU, slope=0.2)],
               lambda L: [(L["x"], None)], gys)


CONCAT = [("convT4s2", 5, 4, 128, 128, 64), ("convT4s2", 3, 8, 128, 128, 64), ("conv3", 2, 16, 64, 64, 64)]
GMAP = (0, 1, 0)


@pytest.mark.parametrize("path", ["plain", "shared_half_direct", "shared_half_autograd", "shared_blocks"])
@pytest.mark.parametrize("kind,N,H,C1,C2,Cout", CONCAT)
def test_concat_block_backward_with_routing(kind, N, H, C1, C2, Cout, path):
    """convT4s2 on cat([x, skip]) (H: the input grid) and upsample + conv3 on cat([up(x), skip]) (H: the conv's grid), three ways:
      plain          one fused concat conv;
      shared_half_*  inside fused.share_skip_halves(), two calls on the same skip with x and 0.5 x: the reference is the sum of
                     two plain blocks (autograd._SkipHalf, du_sum modes 1 and 2; conv3: the K4 transposed-conv form of the x half,
                     dvg_k4_to_w3 and the adjoint data gradient), with DIRECT_PARAM_GRADS on and off, from a non-zero `.grad`;
                     the weight gradient's x and skip channel slices each against their own reference slice;
      shared_blocks  ops.SharedBlocks: 3 groups of N images over 2 skip blocks, map (0, 1, 0), BatchNorm per group as the
                     time-batched decoder calls run it: the reference is three plain blocks (ops.group_sum)."""
    from dvg_amd import autograd as ag, fused, ops
    up = kind == "conv3"
    hx, ho = (H // 2 if up else H), (H if up else 2 * H)
    conv, bn, p = _make_block(kind, C1 + C2, Cout, 9100 + H)
    tag = f"{kind} {(N, H, C1, C2, Cout)} {path}"

    def block(x, skip):
        return ag.conv_block_autograd(kind, conv, bn, x, skip, upsample=up, act=ops.ACT_LRELU, slope=0.2)

    if path == "plain":
        leaves = {"x": params.normal(9110 + H, N, C1, hx, hx), "skip": params.normal(9111 + H, N, C2, H, H)}
        gys = [params.normal(9112 + H, N, Cout, ho, ho)]
        _run_block(tag, kind, up, conv, bn, p, leaves, lambda D: [block(D["x"], D["skip"])],
                   lambda L: [(L["x"], L["skip"])], gys)
    elif path.startswith("shared_half"):
        leaves = {"x": params.normal(9110 + H, N, C1, hx, hx), "skip": params.normal(9111 + H, N, C2, H, H)}
        gys = [params.normal(9112 + H + i, N, Cout, ho, ho) for i in range(2)]

        def hip_forward(D):
            with fused.share_skip_halves():
                return [block(D["x"], D["skip"]), block(D["x"] * 0.5, D["skip"])]

        old = ag.DIRECT_PARAM_GRADS
        ag.DIRECT_PARAM_GRADS = path == "shared_half_direct"
        cat = fused.BLOCKS[kind].cat
        slices = {f"w[{name}]": ("w", (slice(lo, hi),) if cat == 0 else (slice(None), slice(lo, hi)))
                  for name, lo, hi in (("x", 0, C1), ("skip", C1, C1 + C2))}
        try:
            _run_block(tag, kind, up, conv, bn, p, leaves, hip_forward,
                       lambda L: [(L["x"], L["skip"]), (0.5 * L["x"], L["skip"])], gys, start_grads=True, slices=slices)
            assert not ag._wgrad_queues, "every queued weight gradient is flushed when backward() returns"
        finally:
            ag.DIRECT_PARAM_GRADS = old
    else:
        g, blocks = len(GMAP), max(GMAP) + 1
        leaves = {"x": params.normal(9110 + H, g * N, C1, hx, hx), "skip": params.normal(9111 + H, blocks * N, C2, H, H)}
        gy = params.normal(9112 + H, g * N, Cout, ho, ho)

        def hip_forward(D):
            shared = ops.SharedBlocks(D["skip"], N, ops.shared_map(GMAP, dev()), GMAP)
            with fused.bn_groups(g):
                y = block(D["x"], shared)
            return [y[i * N:(i + 1) * N] for i in range(g)]

        _run_block(tag, kind, up, conv, bn, p, leaves, hip_forward,
                   lambda L: [(L["x"][i * N:(i + 1) * N], L["skip"][b * N:(b + 1) * N]) for i, b in enumerate(GMAP)],
                   [gy[i * N:(i + 1) * N] for i in range(g)])


# ---- the layers on the raw frame ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["conv3_first", "conv4s2_first"])
@pytest.mark.parametrize("N,nc,H", [(3, 3, 24), (2, 1, 64)])
def test_first_layer_backward(kind, N, nc, H):
    from dvg_amd import autograd as ag, ops
    ks, st = (3, 1) if kind == "conv3_first" else (4, 2)
    conv, bn = nn.Conv2d(nc, 64, ks, st, 1), nn.BatchNorm2d(64)
    p = _fill(conv, bn, 9200 + H)
    conv.to(dev()), bn.to(dev()).train()
    x = params.frames(9210 + H, N, nc, H)
    gy = params.normal(9211 + H, N, 64, H // st, H // st)
    y = ag.conv_block_autograd(kind, conv, bn, x.to(dev()), None, act=ops.ACT_LRELU, slope=0.2)
    y_hip = y.detach().cpu()

    def compose(P, L):
        u = F.conv2d(x.to(P["w"].dtype), P["w"], P["b"], st, 1)
        yr = _lrelu_forced(F.batch_norm(u, None, None, P["g"], P["be"], True, 0.1, 1e-5), y_hip)
        return {"loss": (yr * gy.to(yr.dtype)).sum(), "ys": [yr]}

    (r64, y64), (r32, _) = _reference(compose, p, {}, torch.float64), _reference(compose, p, {}, torch.float32)
    assert rel_err(y_hip, y64[0]) < 1e-4
    (y * gy.to(dev())).sum().backward()
    _compare(f"{kind} {(N, nc, H)}", {"w": conv.weight.grad, "g": bn.weight.grad, "be": bn.bias.grad}, r32, r64)
    _bias_grad_is_small(conv, r64["w"])
    # a gradient w.r.t. the frames is not part of the training path: asking for one raises
    conv2, bn2 = nn.Conv2d(nc, 64, ks, st, 1).to(dev()), nn.BatchNorm2d(64).to(dev()).train()
    xg = x.to(dev()).requires_grad_(True)
    y2 = ag.conv_block_autograd(kind, conv2, bn2, xg, None, act=ops.ACT_LRELU, slope=0.2)
    with pytest.raises(RuntimeError, match="input frames"):
        y2.sum().backward()


@pytest.mark.parametrize("kind,nc,shared", [("convT3", 1, False), ("convT3", 3, False), ("convT4s2", 1, False),
                                            ("convT4s2", 3, False), ("convT4s2", 1, True), ("convT4s2", 3, True)])
def test_last_layer_backward(kind, nc, shared):
    """ConvTranspose2d(64, nc, 3, 1, 1) + Sigmoid and ConvTranspose2d(64 + 64, nc, 4, 2, 1) + Tanh on cat([x, skip]) at N = 3,
    16 x 16: dx, dskip, dW (dvg_wgrad_thin into the two row slices of the weight's gradient) and db; the 4x4 layer also with
    the skip as SharedBlocks (2 blocks of one image, map (0, 0, 1))."""
    from dvg_amd import autograd as ag, ops
    N, C, H = 3, 64, 16
    ks, st, act = (3, 1, ops.ACT_SIGMOID) if kind == "convT3" else (4, 2, ops.ACT_TANH)
    gmap = (0, 0, 1)
    conv = nn.ConvTranspose2d(C if ks == 3 else 2 * C, nc, ks, st, 1)
    p = _fill(conv, None, 9300 + nc + ks)
    conv.to(dev())
    leaves = {"x": params.normal(9310 + nc, N, C, H, H)}
    if ks == 4:
        leaves["skip"] = params.normal(9311 + nc, 2 if shared else N, C, H, H)
    gy = params.normal(9312 + nc, N, nc, H * st, H * st)

    def compose(P, L):
        inp = L["x"]
        if ks == 4:
            inp = torch.cat([inp, L["skip"][list(gmap)] if shared else L["skip"]], 1)
        pre = F.conv_transpose2d(inp, P["w"], P["b"], st, 1)
        y = torch.sigmoid(pre) if ks == 3 else torch.tanh(pre)
        return {"loss": (y * gy.to(y.dtype)).sum(), "ys": [y]}

    (r64, y64), (r32, _) = (_reference(compose, p, leaves, dt, trainable=("w", "b")) for dt in (torch.float64, torch.float32))
    D = {k: nhwc_leaf(v) for k, v in leaves.items()}
    skip = D.get("skip")
    if shared:
        skip = ops.SharedBlocks(skip, 1, ops.shared_map(gmap, dev()), gmap)
    y = ag.last_layer_autograd(kind, conv, D["x"], skip, act=act)
    assert tuple(y.shape) == tuple(gy.shape) and rel_err(y, y64[0]) < 1e-4
    (y * gy.to(dev())).sum().backward()
    hip = {k: v.grad for k, v in D.items()}
    hip.update(w=conv.weight.grad, b=conv.bias.grad)
    _compare(f"{kind} last nc={nc} shared={shared}", hip, r32, r64)


# ---- the dense ends ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["head", "stem"])
def test_dense_block_backward(kind):
    """Encoder head Conv2d(512, 90, 4, 1, 0) + BN + Tanh on (5, 512, 4, 4) and decoder stem ConvTranspose2d(90, 512, 4, 1, 0) +
    BN + LeakyReLU on (5, 90): dx, dW, dgamma, dbeta."""
    from dvg_amd import autograd as ag, ops
    N, dim = 5, 90
    if kind == "head":
        conv, bn = nn.Conv2d(512, dim, 4, 1, 0), nn.BatchNorm2d(dim)
        x = params.normal(9400, N, 512, 4, 4)
        gy = params.normal(9401, N, dim)
    else:
        conv, bn = nn.ConvTranspose2d(dim, 512, 4, 1, 0), nn.BatchNorm2d(512)
        x = params.normal(9402, N, dim, scale=0.5).tanh()
        gy = params.normal(9403, N, 512, 4, 4)
    p = _fill(conv, bn, 9410 + len(kind))
    conv.to(dev()), bn.to(dev()).train()
    xd = nhwc_leaf(x) if kind == "head" else x.to(dev()).requires_grad_(True)
    if kind == "head":
        y = ag.dense_block_autograd("head", conv, bn, xd, act=ops.ACT_TANH)
    else:
        y = ag.dense_block_autograd("stem", conv, bn, xd, act=ops.ACT_LRELU, slope=0.2)
    y_hip = y.detach().cpu()

    def compose(P, L):
        if kind == "head":
            z = F.batch_norm(F.conv2d(L["x"], P["w"], P["b"]), None, None, P["g"], P["be"], True, 0.1, 1e-5)
            yr = torch.tanh(z).reshape(N, dim)
        else:
            z = F.batch_norm(F.conv_transpose2d(L["x"].view(N, dim, 1, 1), P["w"], P["b"]), None, None, P["g"], P["be"], True,
                             0.1, 1e-5)
            yr = _lrelu_forced(z, y_hip)
        return {"loss": (yr * gy.to(yr.dtype)).sum(), "ys": [yr]}

    (r64, y64), (r32, _) = (_reference(compose, p, {"x": x}, dt) for dt in (torch.float64, torch.float32))
    assert tuple(y_hip.shape) == tuple(gy.shape) and rel_err(y_hip, y64[0]) < 1e-4
    (y * gy.to(dev())).sum().backward()
    _compare(f"dense {kind}", {"x": xd.grad, "w": conv.weight.grad, "g": bn.weight.grad, "be": bn.bias.grad}, r32, r64)
    _bias_grad_is_small(conv, r64["w"])
