"""Train-mode BatchNorm and the training losses, kernel by kernel, against float64 references on the host.

Every statistics writer (dvg_channel_stats, the igemm conv epilogues with and without split-K, the first-layer kernels) feeds
dvg_bn_finalize, whose scale / shift / saved statistics / running statistics are checked; the apply (dvg_bn_act_apply), the backward (dvg_bn_act_bwd_reduce -> dvg_bn_bwd_finalize -> dvg_affine3_apply)
and the losses (dvg_frame_losses, dvg_mse_sum_grad) are checked through the dvg_amd.ops wrappers the training path calls.

The hard inputs are channels whose mean is large next to their standard deviation (|mean| / std up to 1000, mixed within
one launch): trained weights and offset inputs (frames near 0.5, everything after a LeakyReLU) produce them, freshly
initialised modules never do.  Sums of raw x and x^2 in fp32 lose the digits E[x^2] - mean^2 needs there, so the writers
can accumulate around a per-channel pivot ("warm": within one std of the batch mean, as a running mean that training has
moved) and the backward accumulates around the saved batch mean.  No pivot ("cold", K = 0) is the raw-sum arithmetic the
training path runs and is held to ratio 3.

Bars: 1e-6 absolute (global relative error), or within 2x of what torch's fp32 CPU run of the same operation loses against
float64 (tests.common.yardstick) where fp32 rounding of the inputs alone costs more than that."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import params
from dvg_amd._lib import lib
from tests.common import dev, nhwc, rel_err, rel_err_elem, yardstick

pytestmark = pytest.mark.gpu

EPS = 1e-5
RATIOS = (0, 3, -3, 30, -30, 300, -300, 1000, -1000)
# (pivot, largest |mean| / std): the cold pivot is the raw-sum arithmetic, held to the ratios of freshly initialised layers
PIVOTS = [("cold", 3), ("warm", 1000)]
# the conv writers (implicit-GEMM epilogues, their split-K finish, the first-layer kernels) sum around 0
RAW_PIVOTS = [("cold", 3)]
ACTS = {0: lambda t: t, 1: lambda t: F.leaky_relu(t, 0.2), 2: torch.tanh, 3: torch.sigmoid}


def _pkw(pivot):
    return {} if pivot is None else {"pivot": pivot}


def _ratios(c, rmax):
    r = [x for x in RATIOS if abs(x) <= rmax]
    return torch.tensor([r[i % len(r)] for i in range(c)], dtype=torch.float64)


def _leg(name, hip, r32, r64, elem=False, den=None):
    """HIP vs fp64 within 1e-6, or within 2x of the fp32 torch run's own error.  Error: global relative (rel_err),
    element-wise relative (`elem`) or max |a - b| / den per element (`den`: a per-channel scale such as the batch std)."""
    if den is not None:
        e_hip = float(((hip.detach().double().cpu() - r64) / den).abs().max())
        e_32 = float(((r32.double() - r64) / den).abs().max())
    elif elem:
        e_hip, e_32 = rel_err_elem(hip, r64), rel_err_elem(r32, r64)
    else:
        yardstick(name, hip, r32, r64, ratio=2.0, slack=1e-6)
        return
    print(f"{name}: HIP vs fp64 {e_hip:.2e} | fp32 torch vs fp64 {e_32:.2e}")
    assert e_hip <= 2.0 * e_32 + 1e-6, (name, e_hip, e_32)


def _sd_den(u64_2d):
    """Per-channel std (floored for constant channels): the unit of the mean's error."""
    m, s = u64_2d.mean(0), u64_2d.std(0, unbiased=False)
    return s.clamp_min(1e-6 * (float(m.abs().max()) + 1.0))


def _rows_with_ratios(seed, rows, c, rmax, groups=1):
    """[groups * rows][C] fp32 whose channels (per group) have mean ratio * std, std in [0.5, 2]."""
    z = params.normal(seed, groups, rows, c).double()
    if rows > 1:
        z = (z - z.mean(1, keepdim=True)) / z.std(1, unbiased=False, keepdim=True).clamp_min(1e-30)
    sd = 0.5 + 1.5 * torch.rand(c, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64)
    return ((z + _ratios(c, rmax)) * sd).float().reshape(groups * rows, c)


def _warm(u64_2d, seed):
    """A running mean within one std of the batch mean (the state once training has moved it)."""
    m, s = u64_2d.mean(0), u64_2d.std(0, unbiased=False)
    t = torch.rand(m.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1
    return (m + 0.5 * s * t).float()


def _finalize_and_check(name, u2d, st, pivot, momentum=0.1, passes=2):
    """ops.bn_finalize on the partial rows `st` of the fp32 [rows][C] values `u2d` (CPU), the running mean = `pivot` (or 0)
    before; scale / shift / save_mean / save_invstd / running statistics / num_batches_tracked against fp64."""
    from dvg_amd import ops
    rows, c = u2d.shape
    gamma, beta = (1 + 0.1 * params.normal(7, c)).float(), (0.1 * params.normal(8, c)).float()
    rm0 = pivot.clone() if pivot is not None else torch.zeros(c)
    rv0 = 0.5 + torch.rand(c, generator=torch.Generator().manual_seed(9))
    rm, rv = rm0.to(dev()), rv0.to(dev())
    nbt = torch.full((), 5, dtype=torch.int64, device=dev())
    sc, sh, sm, si = ops.bn_finalize(st, gamma.to(dev()), beta.to(dev()), rm, rv, rows, EPS, momentum, save=True,
                                     num_batches_tracked=nbt, passes=passes, **_pkw(rm if pivot is not None else None))
    torch.cuda.synchronize()
    assert int(nbt) == 5 + passes
    u64 = u2d.double()
    m64, v64 = u64.mean(0), u64.var(0, unbiased=False)
    m32, v32 = u2d.mean(0), u2d.var(0, unbiased=False)
    sd = _sd_den(u64)
    _leg(f"{name} save_mean", sm, m32, m64, den=sd)
    _leg(f"{name} save_invstd", si, 1 / torch.sqrt(v32 + EPS), 1 / torch.sqrt(v64 + EPS), elem=True)
    # the normalised output the apply kernels form from scale / shift (evaluated in fp64: finalize's error alone)
    y64 = F.batch_norm(u64, None, None, gamma.double(), beta.double(), True, 0.0, EPS)
    y32 = F.batch_norm(u2d, None, None, gamma, beta, True, 0.0, EPS)
    _leg(f"{name} scale/shift", u64 * sc.double().cpu() + sh.double().cpu(), y32, y64)
    rm64, rv64, rm32, rv32 = rm0.double(), rv0.double(), rm0.clone(), rv0.clone()
    F.batch_norm(u64, rm64, rv64, None, None, True, momentum, EPS)
    F.batch_norm(u2d, rm32, rv32, None, None, True, momentum, EPS)
    _leg(f"{name} running_mean", rm, rm32, rm64, den=torch.maximum(rm64.abs(), sd))
    _leg(f"{name} running_var", rv, rv32, rv64, elem=True)


# ---- forward statistics: every writer -> bn_finalize --------------------------------------------------------------------
@pytest.mark.parametrize("pivot,rmax", PIVOTS)
@pytest.mark.parametrize("rows,c", [(8192, 64), (3000, 100), (16 * 1024 + 1, 17)])
def test_channel_stats_high_ratio(pivot, rmax, rows, c):
    from dvg_amd import ops
    u = _rows_with_ratios(100 + c, rows, c, rmax)
    p = _warm(u.double(), 11) if pivot == "warm" else None
    ud = u.to(dev())
    st = ops.channel_stats(ud, **_pkw(None if p is None else p.to(dev())))
    assert st.shape == (lib().dvg_channel_stats_rows(rows), 2, c)
    _finalize_and_check(f"channel_stats {rows}x{c} {pivot}", u, st, p)


@pytest.mark.parametrize("c", [1, 3, 17, 33, 64, 100, 512])
@pytest.mark.parametrize("rows", [2, 7, 15, 16, 17, 16 * 37 - 1, 16 * 37 + 1, 16 * 1024 - 1, 16 * 1024, 16 * 1024 + 1])
def test_channel_stats_edges(rows, c):
    """Row counts below, at and beyond the slab boundaries of dvg_channel_stats_rows (16 rows per slab up to 1024 slabs),
    channel counts that are not multiples of 4 or of the finalize workgroup's 16; warm pivot, ratios up to 3."""
    from dvg_amd import ops
    u = _rows_with_ratios(200 + rows % 97 + c, rows, c, 3)
    p = _warm(u.double(), 12)
    st = ops.channel_stats(u.to(dev()), **_pkw(p.to(dev())))
    _finalize_and_check(f"channel_stats edge {rows}x{c}", u, st, p)


@pytest.mark.parametrize("pivot,rmax", PIVOTS)
def test_channel_stats_groups_and_running_update(pivot, rmax):
    """bn_finalize(groups=G) + dvg_bn_running_update (first / middle / last momenta) == G sequential fp64 BatchNorm calls."""
    from dvg_amd import ops
    G, rows, c = 4, 2500, 36
    u = _rows_with_ratios(300, rows, c, rmax, groups=G)
    u64 = u.double().view(G, rows, c)
    p = _warm(u64[0], 13) if pivot == "warm" else None
    rm0 = p.clone() if p is not None else torch.zeros(c)
    rv0 = 0.5 + torch.rand(c, generator=torch.Generator().manual_seed(14))
    rm, rv = rm0.to(dev()), rv0.to(dev())
    nbt = torch.zeros((), dtype=torch.int64, device=dev())
    gamma, beta = (1 + 0.1 * params.normal(15, c)).float(), (0.1 * params.normal(16, c)).float()
    moms = (0.1, 1 - 0.9 ** 2, 0.05)
    st = ops.channel_stats(u.to(dev()), G, **_pkw(None if p is None else rm))
    assert st.shape[0] == G * lib().dvg_channel_stats_rows(rows)
    sc, sh, sm, si = ops.bn_finalize(st, gamma.to(dev()), beta.to(dev()), rm, rv, rows, EPS, 0.0, save=True,
                                     num_batches_tracked=nbt, passes=7, groups=G, group_momenta=moms,
                                     **_pkw(None if p is None else rm))
    torch.cuda.synchronize()
    assert int(nbt) == 7 and sc.shape == (G, c)
    rm64, rv64, rm32, rv32 = rm0.double(), rv0.double(), rm0.clone(), rv0.clone()
    for g in range(G):
        mom = moms[0] if g == 0 else (moms[2] if g == G - 1 else moms[1])
        y64 = F.batch_norm(u64[g], rm64, rv64, gamma.double(), beta.double(), True, mom, EPS)
        y32 = F.batch_norm(u[g * rows:(g + 1) * rows], rm32, rv32, gamma, beta, True, mom, EPS)
        _leg(f"groups {pivot} g{g} scale/shift", u64[g] * sc[g].double().cpu() + sh[g].double().cpu(), y32, y64)
        _leg(f"groups {pivot} g{g} save_mean", sm[g], u[g * rows:(g + 1) * rows].mean(0), u64[g].mean(0), den=_sd_den(u64[g]))
        _leg(f"groups {pivot} g{g} save_invstd", si[g], 1 / torch.sqrt(u[g * rows:(g + 1) * rows].var(0, unbiased=False) + EPS),
             1 / torch.sqrt(u64[g].var(0, unbiased=False) + EPS), elem=True)
    _leg(f"groups {pivot} running_mean", rm, rm32, rm64, den=torch.maximum(rm64.abs(), _sd_den(u64[-1])))
    _leg(f"groups {pivot} running_var", rv, rv32, rv64, elem=True)


def test_bn_finalize_count_two():
    from dvg_amd import ops
    u = torch.tensor([[1.0, -3.0, 2.0, 5.0], [3.0, -2.0, 2.5, -5.0]])
    st = ops.channel_stats(u.to(dev()))
    _finalize_and_check("count 2", u, st, None)


def _bias_for_ratio(u0, rmax, seed):
    """Conv bias that puts the per-channel mean / std of u = conv(x) + b at the ratios (u0: conv(x) in fp64, NCHW)."""
    m, s = u0.mean((0, 2, 3)), u0.std((0, 2, 3), unbiased=False)
    return (_ratios(u0.shape[1], rmax) * s - m).float()


def _writer_case(name, u, st, pivot):
    """u: the writer's own output (act NONE, scale None: u = conv(x) + b), NHWC-in-memory (N,C,H,W) on the device."""
    u2d = u.permute(0, 2, 3, 1).reshape(-1, u.shape[1]).cpu()
    _finalize_and_check(name, u2d, st, None if pivot is None else pivot.cpu())


def _pivot_for(u0, b, kind, seed):
    return _warm((u0 + b.double().view(1, -1, 1, 1)).permute(0, 2, 3, 1).reshape(-1, u0.shape[1]), seed) if kind == "warm" else None


@pytest.mark.parametrize("pivot,rmax", RAW_PIVOTS)
@pytest.mark.parametrize("N,H,W,C,Cout", [(4, 16, 16, 32, 64), (4, 8, 8, 128, 64)])   # second: the split-K finish kernel
def test_conv3x3_stats_high_ratio(pivot, rmax, N, H, W, C, Cout):
    from dvg_amd import ops
    x = params.normal(400, N, C, H, W)
    w = params.normal(401, Cout, C, 3, 3, scale=0.1)
    u0 = F.conv2d(x.double(), w.double(), None, 1, 1)
    b = _bias_for_ratio(u0, rmax, 402)
    p = _pivot_for(u0, b, pivot, 403)
    u, st = ops.conv3x3(nhwc(x), None, ops.pack_igemm_weight(w.to(dev())), None, b.to(dev()), act=ops.ACT_NONE, stats=True)
    assert rel_err(u, u0 + b.double().view(1, -1, 1, 1)) < 2e-5
    _writer_case(f"conv3x3 {N}x{C}x{H}x{W}->{Cout} {pivot}", u, st, p)


@pytest.mark.parametrize("pivot,rmax", RAW_PIVOTS)
@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 32, 32, 64, 128), (5, 8, 8, 256, 512)])
def test_conv4x4s2_stats_high_ratio(pivot, rmax, N, H, W, Cin, Cout):
    from dvg_amd import ops
    x = params.normal(410, N, Cin, H, W)
    w = params.normal(411, Cout, Cin, 4, 4, scale=1.0 / np.sqrt(16 * Cin))
    u0 = F.conv2d(x.double(), w.double(), None, 2, 1)
    b = _bias_for_ratio(u0, rmax, 412)
    p = _pivot_for(u0, b, pivot, 413)
    u, st = ops.conv4x4s2(nhwc(x), ops.pack_igemm_weight(w.to(dev())), None, b.to(dev()), act=ops.ACT_NONE, stats=True)
    assert rel_err(u, u0 + b.double().view(1, -1, 1, 1)) < 2e-5
    _writer_case(f"conv4x4s2 {N}x{Cin}x{H}x{W}->{Cout} {pivot}", u, st, p)


@pytest.mark.parametrize("pivot,rmax", RAW_PIVOTS)
@pytest.mark.parametrize("N,H,W,C1,C2,Cout", [(2, 16, 16, 128, 128, 64), (3, 8, 8, 256, 256, 128), (16, 4, 4, 512, 512, 256)])
def test_convT4x4s2_stats_high_ratio(pivot, rmax, N, H, W, C1, C2, Cout):
    """convT writes tile_id * 4 + parity rows."""
    from dvg_amd import ops
    x, sk = params.normal(420, N, C1, H, W), params.normal(421, N, C2, H, W)
    w = params.normal(422, C1 + C2, Cout, 4, 4, scale=1.0 / np.sqrt(4 * (C1 + C2)))
    u0 = F.conv_transpose2d(torch.cat([x, sk], 1).double(), w.double(), None, 2, 1)
    b = _bias_for_ratio(u0, rmax, 423)
    p = _pivot_for(u0, b, pivot, 424)
    u, st = ops.convT4x4s2(nhwc(x), nhwc(sk), ops.pack_igemm_weight(w.to(dev()), True), None, b.to(dev()), act=ops.ACT_NONE,
                           stats=True)
    assert rel_err(u, u0 + b.double().view(1, -1, 1, 1)) < 2e-5
    _writer_case(f"convT4x4s2 {N}x{C1}+{C2}x{H}x{W}->{Cout} {pivot}", u, st, p)


@pytest.mark.parametrize("pivot,rmax", RAW_PIVOTS)
@pytest.mark.parametrize("ks,nc,res", [(3, 1, 64), (3, 3, 24), (4, 1, 64), (4, 3, 40)])
def test_first_layer_stats_high_ratio(pivot, rmax, ks, nc, res):
    """conv3x3_first / conv4x4s2_first (conv3x3_first_pair is eval-only and writes no statistics).  Frames near 0.5 with a
    zero background, as the first layer sees them."""
    from dvg_amd import ops
    x = params.frames(430, 3, nc, res)
    x[:, :, :, : res // 3] = 0.0
    w = params.normal(431, 64, nc, ks, ks, scale=0.3)
    st_ = 1 if ks == 3 else 2
    u0 = F.conv2d(x.double(), w.double(), None, st_, 1)
    b = _bias_for_ratio(u0, rmax, 432)
    p = _pivot_for(u0, b, pivot, 433)
    fn = ops.conv3x3_first if ks == 3 else ops.conv4x4s2_first
    u, st = fn(x.to(dev()), w.to(dev()), None, b.to(dev()), act=ops.ACT_NONE, stats=True)
    assert rel_err(u, u0 + b.double().view(1, -1, 1, 1)) < 2e-5
    _writer_case(f"first{ks} nc{nc} {res} {pivot}", u, st, p)


# ---- apply ---------------------------------------------------------------------------------------------------------------
def _tied(seed, n, c, h, w, rmax):
    """NHWC-in-memory (N,C,H,W) fp32 at the ratios; the first half of the images is constant over every 2x2 window (exact
    ties of the max-pool, like the zero background of Moving MNIST)."""
    z = params.normal(seed, n, c, h, w).double()
    if h % 2 == 0 and w % 2 == 0:
        z[: n // 2] = F.interpolate(z[: n // 2, :, ::2, ::2], scale_factor=2, mode="nearest")
    z = (z - z.mean((0, 2, 3), keepdim=True)) / z.std((0, 2, 3), unbiased=False, keepdim=True)
    return (z + _ratios(c, rmax).view(1, -1, 1, 1)).float()


@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("path,c", [("vec", 64), ("scalar", 6), ("pool", 32)])
@pytest.mark.parametrize("groups", [1, 3])
def test_bn_act_apply(act, path, c, groups):
    from dvg_amd import ops
    n, h, w = 6, 8, 10
    u = _tied(500 + c, n, c, h, w, 3)
    sc = (0.5 + torch.rand(groups, c, generator=torch.Generator().manual_seed(501))).float()
    sh = (params.normal(502, groups, c) - 3 * sc.double()).float()
    ref = torch.cat([ACTS[act](u.double()[g * (n // groups):(g + 1) * (n // groups)] * sc[g].double().view(1, -1, 1, 1)
                               + sh[g].double().view(1, -1, 1, 1)) for g in range(groups)])
    scd, shd = (sc[0], sh[0]) if groups == 1 else (sc, sh)
    out = ops.bn_act_apply(nhwc(u), scd.to(dev()).contiguous(), shd.to(dev()).contiguous(), act=act, slope=0.2,
                           pool=path == "pool", inplace=False)
    y, yp = out if path == "pool" else (out, None)
    assert rel_err(y, ref) < 1e-6
    if yp is not None:
        assert torch.equal(yp.cpu(), F.max_pool2d(y.cpu(), 2, 2))
        assert rel_err(yp, F.max_pool2d(ref, 2, 2)) < 1e-6


# ---- backward ------------------------------------------------------------------------------------------------------------
def _bwd_case(seed, n, c, h, w, rmax, groups, act, train, pool, with_dy, sinks=False, du_sum=0):
    from dvg_amd import ops
    u = _tied(seed, n, c, h, w, rmax)
    gamma, beta = (1 + 0.1 * params.normal(seed + 1, c)).float(), (0.1 * params.normal(seed + 2, c)).float()
    u64 = u.double()
    B = n // groups
    ug = u64.view(groups, B, c, h, w)
    m64, v64 = ug.mean((1, 3, 4)), ug.var((1, 3, 4), unbiased=False)           # [G][C]
    if not train:      # eval mode: running statistics away from the batch's
        m64, v64 = m64 + 0.3 * v64.sqrt(), 1.5 * v64
    mean, invstd = m64.float(), (1 / torch.sqrt(v64 + EPS)).float()

    def forward(uu, dt):
        outs = []
        for g in range(groups):
            t = F.batch_norm(uu[g * B:(g + 1) * B], m64[g].to(dt), v64[g].to(dt), gamma.to(dt), beta.to(dt), False, 0.0, EPS) \
                if not train else F.batch_norm(uu[g * B:(g + 1) * B], None, None, gamma.to(dt), beta.to(dt), True, 0.0, EPS)
            outs.append(ACTS[act](t))
        return torch.cat(outs)
    y64 = forward(u64, torch.float64).detach()
    y = y64.float()           # the saved output the kernel decides the LeakyReLU / max-pool branches from
    dy = params.normal(seed + 3, n, c, h, w).float() if with_dy else None
    dyp = params.normal(seed + 4, n, c, h // 2, w // 2).float() if pool else None

    def grads(dt):
        uu = u.to(dt).requires_grad_(True)
        g_ = gamma.to(dt).requires_grad_(True)
        b_ = beta.to(dt).requires_grad_(True)
        outs = []
        for g in range(groups):
            sl = uu[g * B:(g + 1) * B]
            t = F.batch_norm(sl, None, None, g_, b_, True, 0.0, EPS) if train else \
                F.batch_norm(sl, m64[g].to(dt), v64[g].to(dt), g_, b_, False, 0.0, EPS)
            outs.append(ACTS[act](t))
        ya = torch.cat(outs)
        loss = 0
        if dy is not None:
            loss = loss + (ya * dy.to(dt)).sum()
        if dyp is not None:
            loss = loss + (F.max_pool2d(ya, 2, 2) * dyp.to(dt)).sum()
        loss.backward()
        return uu.grad, g_.grad, b_.grad, uu.grad.sum((0, 2, 3))
    r64, r32 = grads(torch.float64), grads(torch.float32)

    md, isd = (mean[0], invstd[0]) if groups == 1 else (mean, invstd)
    snk = None
    if sinks:
        s0 = [params.normal(seed + 5 + k, c).float() for k in range(3)]
        snk = tuple(t.to(dev()) for t in s0)
    sum_t, s_prev = None, None
    if du_sum:
        s_prev = params.normal(seed + 9, n, c, h, w).float()
        sum_t = nhwc(s_prev.clone())
    du, dg, db, dbias = ops.bn_act_bwd(None if dy is None else nhwc(dy), None if dyp is None else nhwc(dyp), nhwc(y), nhwc(u),
                                       gamma.to(dev()), md.to(dev()).contiguous(), isd.to(dev()).contiguous(), B * h * w,
                                       act=act, slope=0.2, train=train, sinks=snk,
                                       du_sum=None if not du_sum else (sum_t, du_sum))
    if sinks:
        assert dg is None and db is None and dbias is None
        dg, db = snk[0].cpu() - s0[0], snk[1].cpu() - s0[1]
        dbias = snk[2].cpu() - s0[2]
        if train:
            assert torch.equal(snk[2].cpu(), s0[2]), "train-mode BatchNorm: d(bias) is 0, nothing to accumulate"
    name = f"bwd act{act} train{int(train)} pool{int(pool)} dy{int(with_dy)} G{groups} r{rmax}"
    _leg(f"{name} du", du, r32[0], r64[0])
    _leg(f"{name} dgamma", dg, r32[1], r64[1])
    _leg(f"{name} dbeta", db, r32[2], r64[2])
    if train:
        if not sinks:
            assert torch.equal(dbias.cpu(), torch.zeros(c))
        assert float(r64[3].abs().max()) < 1e-9 * float(r64[0].abs().max()) * n * h * w
    else:
        _leg(f"{name} dbias", dbias, r32[3], r64[3])
    if du_sum == 1:
        assert torch.equal(sum_t.cpu(), du.cpu())
    elif du_sum == 2:
        assert torch.equal(sum_t.cpu(), s_prev + du.cpu())


@pytest.mark.parametrize("rmax", [3, 1000])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("pool,with_dy", [(False, True), (True, True), (True, False)])
def test_bn_act_bwd_lrelu(rmax, train, pool, with_dy):
    _bwd_case(600, 8, 64, 16, 16, rmax, 1, 1, train, pool, with_dy)


@pytest.mark.parametrize("rmax", [3, 1000])
@pytest.mark.parametrize("act", [0, 2, 3])
def test_bn_act_bwd_acts(rmax, act):
    _bwd_case(610, 4, 32, 8, 8, rmax, 1, act, True, True, True)


@pytest.mark.parametrize("rmax", [3, 1000])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("pool", [False, True])
def test_bn_act_bwd_groups(rmax, train, pool):
    _bwd_case(620, 9, 128, 8, 8, rmax, 3, 1, train, pool, True)


@pytest.mark.parametrize("rmax", [3, 1000])
def test_bn_act_bwd_scalar_path(rmax):
    """C % 4 != 0: the scalar reduce and affine kernels (the (N, 90) encoder head runs through them as (rows, C, 1, 1); at 3
    rows per group du's B * u + C form itself loses digits once |mean| / std >> 3, as torch's fp32 run does)."""
    _bwd_case(630, 4, 6, 6, 10, rmax, 1, 1, True, False, True)
    _bwd_case(631, 6, 90, 1, 1, min(rmax, 3), 2, 2, True, False, True)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("groups", [1, 2])
def test_bn_act_bwd_sinks(train, groups):
    _bwd_case(640, 4, 64, 8, 8, 1000, groups, 1, train, True, True, sinks=True)


@pytest.mark.parametrize("mode", [1, 2])
def test_bn_act_bwd_du_sum(mode):
    _bwd_case(650, 4, 64, 8, 8, 300, 1, 1, True, False, True, du_sum=mode)


def test_bn_act_bwd_pool_ties_first_maximum():
    """Every window of the first half of the batch is a 4-way tie: the gradient goes to the first element in scan order
    (nn.MaxPool2d), pinned against torch's max_pool2d backward by the du comparison - and directly on dp here."""
    from dvg_amd import ops
    n, c, h, w = 2, 4, 4, 4
    u = _tied(660, n, c, h, w, 0)
    y = u.clone()
    dyp = torch.ones(n, c, h // 2, w // 2)
    du, *_ = ops.bn_act_bwd(None, nhwc(dyp), nhwc(y), nhwc(u), torch.ones(c, device=dev()), torch.zeros(c, device=dev()),
                            torch.ones(c, device=dev()), n * h * w, act=0, slope=0.2, train=False)
    ut = u.clone().requires_grad_(True)
    F.max_pool2d(ut, 2, 2).backward(dyp)
    assert torch.equal(du.cpu(), ut.grad)
    assert torch.equal(du.cpu()[0, :, ::2, ::2], torch.ones(c, h // 2, w // 2))
    _bwd_case(661, 4, 32, 8, 8, 3, 1, 1, True, True, False)


# ---- losses --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("S,shape", [(3, (5, 1, 4, 11)), (2, (7, 3, 12, 12)), (19, (64, 1, 64, 64))])
def test_frame_losses(K, S, shape):
    """S = 19, 64 x 64 x 64: the training size (5 M elements per call position through fp32 per-thread partial sums)."""
    from dvg_amd import ops
    n = int(np.prod(shape))
    target = torch.rand((S,) + shape, generator=torch.Generator().manual_seed(700))
    pred = (target.unsqueeze(1) + 0.1 * params.normal(701, S, K, *shape).float()).contiguous()
    weights = [1.0 / n, 0.5 / n, 2.0 / n][:K]
    sums, dpred = ops.frame_losses(pred.to(dev()), target.to(dev()), weights)
    d64 = pred.double() - target.double().unsqueeze(1)
    ref = (d64 ** 2).sum(tuple(i for i in range(d64.dim()) if i != 1))
    assert rel_err_elem(sums, ref) < 1e-6, (sums.cpu(), ref)
    w64 = torch.tensor(weights, dtype=torch.float64).view((1, K) + (1,) * len(shape))
    assert rel_err(dpred, 2 * w64 * d64) < 1e-6


@pytest.mark.parametrize("n", [1, 90, 1023, 1025, 19 * 64 * 90])
def test_mse_sum_grad(n):
    from dvg_amd import ops
    a, b = params.normal(710, n).float(), params.normal(711, n).float()
    scale = 0.37 / n
    s, da = ops.mse_sum_grad(a.to(dev()), b.to(dev()), scale)
    d64 = a.double() - b.double()
    assert abs(float(s) - float((d64 ** 2).sum())) <= 1e-6 * float((d64 ** 2).sum())
    assert rel_err(da, 2 * scale * d64) < 1e-6
    s2, none = ops.mse_sum_grad(a.to(dev()), b.to(dev()), scale, need_grad=False)
    assert none is None and float(s2) == float(s)
