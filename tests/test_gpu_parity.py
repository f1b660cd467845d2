"""GPU parity tests, kernel level: every kernel of libdvg_hip.so, through the C ABI, against the CPU oracle on the same seeded
inputs.  (Modules against the golden vectors produced by the REFERENCE: tests/test_gpu_modules.py; the Winograd forms and their
hand-over kernels: tests/test_gpu_winograd.py.)

Tolerance: the north star asks for 1e-4 relative on fp32 frames; tests use REL = 1e-4 on
max|a-b| / max|b| (and a tighter figure where noted).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dvg_oracle as orc
from oracle import params
from tests.common import BACKBONE_CASES, backbone_case, dev, nhwc, oracle_backbone, rel_err, summarize, to64, yardstick

pytestmark = pytest.mark.gpu
REL = 1e-4


def test_layout_roundtrip():
    from dvg_amd import ops
    x = params.normal(1, 3, 70, 9, 13).to(dev())
    y = ops.to_nhwc(x)
    assert ops.is_nhwc(y) and torch.equal(y, x)
    assert torch.equal(ops.to_nchw(y), x) and ops.to_nchw(y).is_contiguous()


def test_weight_pack_roundtrip_is_bit_exact():
    from dvg_amd import ops
    w = params.normal(2, 64, 32, 3, 3).to(dev())
    wp = ops.pack_conv_weight(w)
    assert torch.equal(wp, w.permute(2, 3, 0, 1).reshape(9, 64, 32))
    assert torch.equal(ops.unpack_conv_weight(wp, 3, 3), w)
    wt = params.normal(3, 32, 64, 4, 4).to(dev())
    wtp = ops.pack_convT_weight(wt)
    assert torch.equal(wtp, wt.flip(2, 3).permute(2, 3, 1, 0).reshape(16, 64, 32))
    assert torch.equal(ops.unpack_convT_weight(wtp, 4, 4), wt)


@pytest.mark.parametrize("N,H,W,C1,C2,Cout,up,pool", [
    (2, 16, 16, 32, 0, 64, False, False),
    (2, 16, 32, 64, 0, 128, False, True),     # 8x16 tiles, BN=64 fallback, pooled output
    (3, 8, 8, 64, 0, 64, False, True),        # 8x8 tiles
    (2, 16, 16, 32, 32, 64, True, False),     # fused nearest-up + cat
    (1, 8, 8, 64, 64, 128, True, False),
    (2, 32, 32, 32, 64, 64, False, False),    # cat without upsample
    (64, 8, 8, 64, 0, 128, False, False),     # enough tiles for BN=128
    (8, 8, 8, 512, 0, 256, False, True),      # 32 workgroups, 32 K chunks: split-K x8 + finish kernel (pool)
    (4, 16, 16, 128, 128, 64, True, False),   # split-K with fused up + cat
])
def test_conv3x3_igemm(N, H, W, C1, C2, Cout, up, pool):
    from dvg_amd import ops
    hx, wx = (H // 2, W // 2) if up else (H, W)
    x = params.normal(10, N, C1, hx, wx)
    sk = params.normal(11, N, C2, H, W) if C2 else None
    w = params.normal(12, Cout, C1 + C2, 3, 3, scale=1.0 / np.sqrt(9 * (C1 + C2)))
    sc = 1.0 + 0.1 * params.normal(13, Cout)
    sh = 0.1 * params.normal(14, Cout)
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    if sk is not None:
        xin = torch.cat([xin, sk], 1)
    ref = F.leaky_relu(F.conv2d(xin, w, None, 1, 1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1), 0.2)
    wp = ops.pack_igemm_weight(w.to(dev()))
    out = ops.conv3x3(nhwc(x), None if sk is None else nhwc(sk), wp, sc.to(dev()), sh.to(dev()), upsample=up,
                      pool=pool)
    y, yp = out if pool else (out, None)
    assert rel_err(y, ref) < 2e-5
    if pool:
        assert torch.equal(yp, F.max_pool2d(y, 2, 2)), "fused max-pool must be bit-exact w.r.t. its own y"
        assert rel_err(yp, F.max_pool2d(ref, 2, 2)) < 2e-5


@pytest.mark.parametrize("N,H,W,C,Cout", [(4, 16, 16, 32, 64), (4, 8, 8, 128, 64)])   # second case: split-K finish path
def test_conv3x3_stats_epilogue(N, H, W, C, Cout):
    from dvg_amd import ops
    x = params.normal(20, N, C, H, W)
    w = params.normal(21, Cout, C, 3, 3, scale=0.1)
    b = params.normal(22, Cout, scale=0.2)
    u_ref = F.conv2d(x, w, b, 1, 1)
    (u, st) = ops.conv3x3(nhwc(x), None, ops.pack_igemm_weight(w.to(dev())), None, b.to(dev()), act=ops.ACT_NONE,
                          stats=True)
    assert rel_err(u, u_ref) < 2e-5
    tot = st.double().sum(0).cpu()
    np.testing.assert_allclose(tot[0].numpy(), u_ref.double().sum((0, 2, 3)).numpy(), rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(tot[1].numpy(), (u_ref.double() ** 2).sum((0, 2, 3)).numpy(), rtol=1e-4)
    gamma, beta = 1 + 0.1 * params.normal(23, Cout), 0.1 * params.normal(24, Cout)
    rm, rv = torch.zeros(Cout), torch.ones(Cout)
    ref = F.batch_norm(u_ref, rm, rv, gamma, beta, True, 0.1, 1e-5)
    rmd, rvd = torch.zeros(Cout, device=dev()), torch.ones(Cout, device=dev())
    sc, sh = ops.bn_finalize(st, gamma.to(dev()), beta.to(dev()), rmd, rvd, N * H * W, 1e-5, 0.1)
    y, yp = ops.bn_act_apply(u, sc, sh, act=ops.ACT_LRELU, pool=True, inplace=False)
    assert rel_err(y, F.leaky_relu(ref, 0.2)) < 2e-5
    assert torch.equal(yp, F.max_pool2d(y, 2, 2))
    assert rel_err(rmd, rm) < 1e-5 and rel_err(rvd, rv) < 1e-5


@pytest.mark.parametrize("nc,res", [(1, 64), (3, 64), (3, 128), (1, 24)])
def test_first_layers(nc, res):
    from dvg_amd import ops
    x = params.frames(30, 2, nc, res)
    for ks, st, fn in ((3, 1, ops.conv3x3_first), (4, 2, ops.conv4x4s2_first)):
        w = params.normal(31, 64, nc, ks, ks, scale=0.3)
        sc, sh = 1 + 0.1 * params.normal(32, 64), 0.1 * params.normal(33, 64)
        ref = F.leaky_relu(F.conv2d(x, w, None, st, 1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1), 0.2)
        y, stt = fn(x.to(dev()), w.to(dev()), sc.to(dev()), sh.to(dev()), stats=True)
        assert rel_err(y, ref) < 2e-5
        pre = F.conv2d(x, w, None, st, 1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
        np.testing.assert_allclose(stt.double().sum(0)[0].cpu().numpy(), pre.double().sum((0, 2, 3)).numpy(),
                                   rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 32, 32, 64, 128), (2, 16, 16, 128, 256), (5, 8, 8, 256, 512),
                                            (2, 64, 64, 64, 64), (16, 8, 8, 256, 512), (128, 32, 32, 32, 128),
                                            (3, 16, 48, 16, 64)])
def test_conv4x4s2_igemm(N, H, W, Cin, Cout):
    """dvg_conv4x4s2_bn_act_v2 (one stage per input parity, r05) vs F.conv2d: 8 x 8 tiles, the 4-image 4 x 4 tile with a ragged
    batch, the 8 x 16 tile (>= 512 workgroups: the (128, 32, 32, 32, 128) case), a non-square map with three tile columns."""
    from dvg_amd import ops
    x = params.normal(40, N, Cin, H, W)
    w = params.normal(41, Cout, Cin, 4, 4, scale=1.0 / np.sqrt(16 * Cin))
    sc, sh = 1 + 0.1 * params.normal(42, Cout), 0.1 * params.normal(43, Cout)
    ref = F.leaky_relu(F.conv2d(x, w, None, 2, 1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1), 0.2)
    y, st = ops.conv4x4s2(nhwc(x), ops.pack_igemm_weight(w.to(dev())), sc.to(dev()), sh.to(dev()), stats=True)
    assert rel_err(y, ref) < 2e-5
    pre = F.conv2d(x, w, None, 2, 1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    np.testing.assert_allclose(st.double().sum(0)[1].cpu().numpy(), (pre.double() ** 2).sum((0, 2, 3)).numpy(),
                               rtol=1e-4)


def test_conv4x4s2_splits_a_batch_beyond_the_kernels_32_bit_offsets(monkeypatch):
    """the parity-split stride-2 conv addresses its activation with 32-bit offsets (N H W Cin < 2^31) and the
    wrapper used to hard-fail above that.  It now runs such a batch as several launches over runs of images; exercised here by
    lowering the wrapper's threshold (the kernel's own limit is unchanged) so that a 200-image batch splits into three runs:
    the output equals the single launch's bit for bit, the per-tile statistics rows sum to the same totals, ragged last run
    included; the dgrad of the transposed conv goes through the same wrapper."""
    from dvg_amd import ops
    from dvg_amd.ops import conv as conv_mod
    N, H, W, Cin, Cout = 200, 32, 32, 64, 128          # (every run stays above the split-K threshold: same kernels as one launch)
    x = nhwc(params.normal(44, N, Cin, H, W))
    wp = ops.pack_igemm_weight((params.normal(45, Cout, Cin, 4, 4, scale=1.0 / np.sqrt(16 * Cin))).to(dev()))
    sc, sh = (1 + 0.1 * params.normal(46, Cout)).to(dev()), (0.1 * params.normal(47, Cout)).to(dev())
    y0, st0 = ops.conv4x4s2(x, wp, sc, sh, stats=True)
    assert st0.tile_images == 1
    monkeypatch.setattr(conv_mod, "CONV4S2_MAX_FLOATS", 97 * Cin * H * W)       # at most 96 images per launch: runs of 72 + 72 + 56
    y1, st1 = ops.conv4x4s2(x, wp, sc, sh, stats=True)
    y2 = ops.conv4x4s2(x, wp, sc, sh)
    # every output element is the same K-ordered sum whatever tile or launch it is part of: bit-equal outputs; the statistics
    # rows are per tile (the runs pick 8 x 8 tiles where the whole batch picks 8 x 16): equal sums
    assert torch.equal(y1, y0) and torch.equal(y2, y0) and ops.is_nhwc(y1)
    assert st1.tile_images == 1 and st1.shape[1:] == st0.shape[1:]
    np.testing.assert_allclose(st1.double().sum(0).cpu().numpy(), st0.double().sum(0).cpu().numpy(), rtol=1e-6, atol=1e-4)
    monkeypatch.setattr(conv_mod, "CONV4S2_MAX_FLOATS", Cin * H * W)            # not even one image fits: a clear error
    with pytest.raises(RuntimeError, match="32-bit offsets"):
        ops.conv4x4s2(x, wp, sc, sh)


@pytest.mark.parametrize("N,H,W,C1,C2,Cout", [(2, 4, 4, 512, 512, 256), (3, 8, 8, 256, 256, 128),
                                              (2, 16, 16, 128, 128, 64), (2, 32, 32, 64, 0, 64),
                                              (16, 4, 4, 512, 512, 256)])
def test_convT4x4s2_igemm(N, H, W, C1, C2, Cout):
    from dvg_amd import ops
    x = params.normal(50, N, C1, H, W)
    sk = params.normal(51, N, C2, H, W) if C2 else None
    w = params.normal(52, C1 + C2, Cout, 4, 4, scale=1.0 / np.sqrt(4 * (C1 + C2)))
    sc, sh = 1 + 0.1 * params.normal(53, Cout), 0.1 * params.normal(54, Cout)
    xin = x if sk is None else torch.cat([x, sk], 1)
    pre = F.conv_transpose2d(xin, w, None, 2, 1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    y, st = ops.convT4x4s2(nhwc(x), None if sk is None else nhwc(sk), ops.pack_igemm_weight(w.to(dev()), True),
                           sc.to(dev()), sh.to(dev()), stats=True)
    assert rel_err(y, F.leaky_relu(pre, 0.2)) < 2e-5
    np.testing.assert_allclose(st.double().sum(0)[0].cpu().numpy(), pre.double().sum((0, 2, 3)).numpy(), rtol=1e-4,
                               atol=1e-2)


@pytest.mark.parametrize("nc", [1, 3])
def test_last_layers(nc):
    from dvg_amd import ops
    x = params.normal(60, 2, 64, 40, 64)
    w = params.normal(61, 64, nc, 3, 3, scale=0.05)
    b = params.normal(62, nc, scale=0.1)
    ref = torch.sigmoid(F.conv_transpose2d(x, w, b, 1, 1))
    y = ops.convT3x3_last(nhwc(x), w.to(dev()), b.to(dev()), nc)
    assert rel_err(y, ref) < 2e-5 and y.is_contiguous()
    x1, x2 = params.normal(63, 2, 64, 32, 32), params.normal(64, 2, 64, 32, 32)
    w4 = params.normal(65, 128, nc, 4, 4, scale=0.05)
    ref = torch.tanh(F.conv_transpose2d(torch.cat([x1, x2], 1), w4, b, 2, 1))
    y = ops.convT4x4s2_last(nhwc(x1), nhwc(x2), w4.to(dev()), b.to(dev()), nc, act=ops.ACT_TANH)
    assert rel_err(y, ref) < 2e-5


@pytest.mark.parametrize("C,T,P", [(64, 9, 64 * 48), (64, 16, 16), (64, 27, 4096 + 16), (128, 48, 2048), (128, 16, 80)])
def test_pixel_proj(C, T, P):
    """dvg_pixel_proj (MFMA 16x16x4, fragments straight from global memory) against a float64 matmul, including
    tile counts that are not a multiple of the 4-tile unroll and T that is not a multiple of 16."""
    from dvg_amd import ops
    x = params.normal(66, 1, P, 1, C).permute(0, 3, 1, 2).contiguous()    # (1,C,P,1)
    w = params.normal(67, T, C, scale=0.1)
    d = ops.pixel_proj(nhwc(x), w.to(dev()))
    ref = x[0, :, :, 0].t().double() @ w.double().t()
    assert d.shape == (P, T) and rel_err(d, ref) < 2e-5


@pytest.mark.parametrize("nc", [1, 3])
def test_last_layers_two_step(nc):
    """The product path of the last layer (projection + gather), with the skip projection cached across calls
    while the skip tensor is unchanged and recomputed when it is modified in place."""
    from dvg_amd import ops
    b = params.normal(62, nc, scale=0.1)
    x = params.normal(60, 2, 64, 40, 64)
    w = params.normal(61, 64, nc, 3, 3, scale=0.05)
    ref = torch.sigmoid(F.conv_transpose2d(x, w, b, 1, 1))
    y = ops.convT_last_two_step(nhwc(x), None, w.to(dev()), b.to(dev()), nc, 3, act=ops.ACT_SIGMOID)
    assert rel_err(y, ref) < 2e-5 and y.is_contiguous()
    x2 = params.normal(64, 2, 64, 32, 32)
    w4 = params.normal(65, 128, nc, 4, 4, scale=0.05).to(dev())
    sk = nhwc(x2)
    ops.clear_skip_proj_cache()
    for seed in (63, 68, 69):
        x1 = params.normal(seed, 2, 64, 32, 32)
        ref = torch.tanh(F.conv_transpose2d(torch.cat([x1, x2], 1), w4.cpu(), b, 2, 1))
        y = ops.convT_last_two_step(nhwc(x1), sk, w4, b.to(dev()), nc, 4, act=ops.ACT_TANH)
        assert rel_err(y, ref) < 2e-5
    assert len(ops._SKIP_PROJ_CACHE) == 1
    sk.mul_(0.5)                                         # in-place change: the cached projection must not be reused
    ref = torch.tanh(F.conv_transpose2d(torch.cat([x1, 0.5 * x2], 1), w4.cpu(), b, 2, 1))
    y = ops.convT_last_two_step(nhwc(x1), sk, w4, b.to(dev()), nc, 4, act=ops.ACT_TANH)
    assert rel_err(y, ref) < 2e-5


@pytest.mark.parametrize("M,N,K,splitk,period", [(64, 90, 8192, 32, 90), (64, 8192, 90, 1, 512), (5, 256, 90, 1, 256),
                                                 (50, 90, 256, 1, 90), (7, 33, 1000, 4, 11)])
def test_gemm_nt(M, N, K, splitk, period):
    from dvg_amd import ops
    a = params.normal(70, M, K, scale=1 / np.sqrt(K))
    w = params.normal(71, N, K)
    sc, sh = 1 + 0.1 * params.normal(72, period), 0.1 * params.normal(73, period)
    idx = torch.arange(N) % period
    ref = torch.tanh((a.double() @ w.double().t()) * sc.double()[idx] + sh.double()[idx])
    y = ops.gemm_nt(a.to(dev()), w.to(dev()), sc.to(dev()), sh.to(dev()), act=ops.ACT_TANH, period=period,
                    splitk=splitk)
    assert rel_err(y, ref) < 2e-5


@pytest.mark.parametrize("B,H", [(64, 256), (5, 256), (50, 128), (33, 64)])
def test_lstm_cell(B, H):
    from dvg_amd import ops
    x, h, c = params.normal(80, B, H, scale=0.5), params.normal(81, B, H, scale=0.5), params.normal(82, B, H, scale=0.5)
    sd = {"l.weight_ih": params.normal(83, 4 * H, H, scale=1 / np.sqrt(H)),
          "l.weight_hh": params.normal(84, 4 * H, H, scale=1 / np.sqrt(H)),
          "l.bias_ih": params.normal(85, 4 * H, scale=0.1), "l.bias_hh": params.normal(86, 4 * H, scale=0.1)}
    h_ref, c_ref = orc.lstm_cell(x.double(), (h.double(), c.double()), {k: v.double() for k, v in sd.items()}, "l")
    d = dev()
    h2, c2, gates = ops.lstm_cell(x.to(d), h.to(d), c.to(d), sd["l.weight_ih"].to(d), sd["l.weight_hh"].to(d),
                                  sd["l.bias_ih"].to(d), sd["l.bias_hh"].to(d), want_gates=True)
    assert rel_err(h2, h_ref) < 1e-5 and rel_err(c2, c_ref) < 1e-5
    from tests.dense_ref import lstm_cell_ref
    g_ref = lstm_cell_ref(x.double(), h.double(), c.double(), *(sd["l." + k].double() for k in
                                                                 ("weight_ih", "weight_hh", "bias_ih", "bias_hh")))["gates"]
    assert gates.shape == (B, 4 * H) and rel_err(gates, g_ref) < 1e-5


def _gp_bars(prec):
    """Parity bars of the GP kernels against the fp64 oracle: (mean rel, (co)variance / sample as a fraction of the
    largest covariance entry, KL rel).  fp64-internal kernels (ABI 6, the product path for every shape of BASELINE.json's
    configs) are held to BASELINE.json's 1e-4 with a decade to spare on the mean; the fp32 variant that only shapes with
    an over-sized fp64 working set get (M = 64 beyond B ~ 100; the backward kernel beyond B = 71) keeps the r02 bars."""
    return (1e-5, 1e-4, 1e-4) if prec == 64 else (5e-4, 2e-3, 2e-3)


@pytest.mark.parametrize("B,D,M", [(64, 90, 40), (50, 90, 40), (16, 12, 40), (95, 6, 40), (128, 8, 40), (7, 5, 64)])
def test_gp_predict_eval_and_train(B, D, M):
    """generate_frames.py:168-171 (likelihood(gp_layer(h)).rsample(), eval) and train.py:225-232 (train mode + KL).
    Yardstick: the oracle's own fp32 arithmetic (torch CPU) against its fp64 arithmetic on the same seeds - the HIP
    kernel, fp64 inside, must be at least as close to fp64 as that (up to the rounding of its fp32 outputs) AND inside
    the bars."""
    from dvg_amd import ops
    from dvg_amd._lib import lib
    sd, lik = params.gp_state(90, D=D, M=M)
    h = params.normal(91, B, D, scale=0.7).tanh()
    noise = orc.likelihood_noise(lik)
    s, ell, c = orc.gp_hypers(sd)
    eps = params.normal(92, D, B)
    d = dev()
    args = [sd["variational_strategy.inducing_points"], sd["variational_strategy.variational_distribution.variational_mean"],
            sd["variational_strategy.variational_distribution.chol_variational_covar"], c, s, ell]
    args = [t.to(d) for t in args]
    prec = lib().dvg_gp_precision(B, M, 1)
    assert prec == 64            # every shape of this list: B = 128 runs the packed-triangle fp64 variant
    bar_mean, bar_cov, bar_kl = _gp_bars(prec)
    absdiff = lambda a, b: float((a.double().cpu() - b.double()).abs().max())  # noqa: E731
    ulp = 2.0 ** -22     # two fp32 ulps: the outputs are rounded to fp32 once

    ev_ref = orc.gp_predict(h, sd, training=False, noise=noise)
    ev_f32 = orc.gp_predict(h, sd, training=False, noise=noise, dtype=torch.float32)
    r = ops.gp_predict(h.to(d), *args, noise=noise.to(d), eps=eps.to(d), want_cov=True)
    scale, mscale = float(ev_ref["cov"].abs().max()), float(ev_ref["mean"].abs().max())
    e_mean, e_cov, e_var = absdiff(r["mean"], ev_ref["mean"]), absdiff(r["cov"], ev_ref["cov"]), absdiff(r["var"], ev_ref["var"])
    assert e_mean < bar_mean * mscale and e_cov < bar_cov * scale and e_var < bar_cov * scale, (e_mean, e_cov, e_var)
    smp_ref = orc.gp_rsample(ev_ref["mean"], ev_ref["cov"], eps.double())
    e_smp = absdiff(r["sample"], smp_ref)
    assert e_smp < bar_cov * float(smp_ref.abs().max()), e_smp
    # the sample must also be consistent with the kernel's OWN covariance: mean + chol(cov) eps
    own = orc.gp_rsample(r["mean"].double().cpu(), r["cov"].double().cpu(), eps.double())
    assert absdiff(r["sample"], own) < (1e-4 if prec == 64 else 2e-3)
    if prec == 64:
        y_mean, y_cov = absdiff(ev_f32["mean"], ev_ref["mean"]), absdiff(ev_f32["cov"], ev_ref["cov"])
        assert e_mean <= max(y_mean, ulp * mscale), (e_mean, y_mean)
        assert e_cov <= max(y_cov, ulp * scale), (e_cov, y_cov)

    tr_ref = orc.gp_predict(h, sd, training=True)
    tr_f32 = orc.gp_predict(h, sd, training=True, dtype=torch.float32)
    t = ops.gp_predict(h.to(d), *args, want_kl=True, train_mode=True)
    prec_t = lib().dvg_gp_precision(B, M, 0)
    assert prec_t == 64          # without a covariance every B <= 128 fits in fp64
    bar_mean, bar_cov, bar_kl = _gp_bars(prec_t)
    e_mean, e_var = absdiff(t["mean"], tr_ref["mean"]), absdiff(t["var"], tr_ref["var"])
    e_kl = float(((t["kl"].double().cpu() - tr_ref["kl"]).abs() / tr_ref["kl"].abs()).max())
    assert e_mean < bar_mean * mscale and e_var < bar_cov * scale and e_kl < bar_kl, (e_mean, e_var, e_kl)
    y_var = absdiff(tr_f32["var"], tr_ref["var"])
    y_kl = float(((tr_f32["kl"].double() - tr_ref["kl"]).abs() / tr_ref["kl"].abs()).max())
    assert e_var <= max(y_var, ulp * scale) and e_kl <= max(y_kl, ulp), (e_var, y_var, e_kl, y_kl)


def test_gp_raw_hyper_parameters_in_kernel():
    """Inference hands the RAW hyper-parameters to the kernel (flag bit 1): soft-plus and the 1e-4 noise floor applied in
    the kernel must give what the soft-plus'ed call gives (fp64 soft-plus of an fp32 raw value vs torch's fp32 one: the
    1-ulp difference in s / ell moves the outputs by ~1e-6 of their scale, measured on the oracle)."""
    from dvg_amd import ops
    B, D, M = 50, 90, 40
    sd, lik = params.gp_state(93, D=D, M=M)
    h = params.normal(94, B, D, scale=0.7).tanh()
    eps = params.normal(95, D, B)
    s, ell, c = orc.gp_hypers(sd)
    d = dev()
    com = [sd["variational_strategy.inducing_points"], sd["variational_strategy.variational_distribution.variational_mean"],
           sd["variational_strategy.variational_distribution.chol_variational_covar"], c]
    com = [t.to(d) for t in com]
    a = ops.gp_predict(h.to(d), *com, s.to(d), ell.to(d), noise=orc.likelihood_noise(lik).to(d), eps=eps.to(d), want_cov=True)
    b = ops.gp_predict(h.to(d), *com, sd["covar_module.raw_outputscale"].to(d), sd["covar_module.base_kernel.raw_lengthscale"].to(d),
                       noise=lik["noise_covar.raw_noise"].to(d), eps=eps.to(d), want_cov=True, raw_hypers=True)
    scale = float(a["cov"].abs().max())
    assert float((a["mean"] - b["mean"]).abs().max()) < 1e-5 * float(a["mean"].abs().max())
    assert float((a["cov"] - b["cov"]).abs().max()) < 1e-5 * scale
    assert float((a["sample"] - b["sample"]).abs().max()) < 1e-5 * float(a["sample"].abs().max())


@pytest.mark.parametrize("terms", [1, 2])
def test_gp_first_call_initialisation_on_the_device(terms):
    """gp_models.INIT_JITTER_TERMS (DESIGN.md 3.3's open point, both readings behind one constant): an UNTRAINED layer's first
    train-mode call initialises L_S <- chol((K_zz + terms * 1e-3 I)^-1) and the kernel's KL / variance of that state equal the
    oracle's for the same reading (terms = 1: KL = 0 - the GP starts at its prior; 2: KL ~ 0.5 nats per latent dim); a TRAINED
    state (variational_params_initialized = 1) gives identical predictions whatever the constant says."""
    from dvg_amd.models import gp_models as gm
    D, M, B = 12, 40, 16
    h = params.normal(97, B, D, scale=0.7).tanh()
    old = gm.INIT_JITTER_TERMS
    try:
        gm.INIT_JITTER_TERMS = terms
        sd, _ = params.gp_state(96, D=D, M=M, trained=False)
        layer = gm.GPRegressionLayer1(D, M)
        layer.load_state_dict(sd)
        layer.to(dev()).train()
        with torch.no_grad():
            pred = layer(h.to(dev()))
            kl, var = pred.kl.double().cpu(), pred.variance.double().cpu()
        ref = {k: v.clone() for k, v in sd.items()}
        orc.gp_prior_init(ref, jitter_terms=terms)
        tr = orc.gp_predict(h, ref, training=True)
        assert float((var - tr["var"]).abs().max()) < 1e-4 * float(tr["var"].abs().max())
        if terms == 1:
            assert float(kl.abs().max()) < 2e-3 and float(tr["kl"].abs().max()) < 2e-3       # zero up to the fp32 storage of L_S
        else:
            assert float(((kl - tr["kl"]).abs() / tr["kl"]).max()) < 1e-3 and float(tr["kl"].min()) > 0.05
        sdt, _ = params.gp_state(98, D=D, M=M, trained=True)
        outs = []
        for t_ in (1, 2):
            gm.INIT_JITTER_TERMS = t_
            trained = gm.GPRegressionLayer1(D, M)
            trained.load_state_dict(sdt)
            trained.to(dev()).train()
            with torch.no_grad():
                p_ = trained(h.to(dev()))
                outs.append((p_.mean.clone(), p_.variance.clone(), p_.kl.clone()))
        assert all(torch.equal(a, b) for a, b in zip(*outs))
    finally:
        gm.INIT_JITTER_TERMS = old


def test_gp_index_bookkeeping_is_exact():
    """(B,D) <-> (D,B,1) view bookkeeping (train.py:225): GP d must see column d of h, bit-exactly."""
    from dvg_amd.models.gp_models import GPRegressionLayer1
    D, B = 6, 9
    gp = GPRegressionLayer1(D, 8).to(dev()).eval()
    h = params.normal(95, B, D).to(dev())
    a = gp(h.transpose(0, 1).view(D, B, 1))
    b = gp(h)
    assert torch.equal(a.mean, b.mean) and a.mean.shape == (D, B)
    # permuting the batch permutes the prediction columns and nothing else
    perm = torch.randperm(B, device=dev())
    assert torch.allclose(gp(h[perm]).mean, a.mean[:, perm], atol=1e-5)


@pytest.mark.parametrize("B,C,H,W", [(3, 1, 64, 64), (2, 3, 128, 128), (2, 2, 9, 23)])
def test_eval_frames(B, C, H, W):
    """dvg_eval_frames (SSIM + PSNR of utils.eval_seq) against the oracle's float64 restatement of skimage."""
    from dvg_amd import ops
    gt = [(0.5 + 0.25 * params.normal(80 + t, B, C, H, W)).clamp(0, 1) for t in range(2)]
    pred = [(g + 0.1 * params.normal(90 + t, B, C, H, W)).clamp(0, 1) for t, g in enumerate(gt)]
    pred[1][0] = gt[1][0] * 0.5            # a structured error too
    s_ref, p_ref = orc.eval_seq(gt, pred)
    for t in range(2):
        s, p = ops.eval_frames(gt[t].to(dev()), pred[t].to(dev()))
        np.testing.assert_allclose(s.cpu().numpy(), s_ref[:, t], rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(p.cpu().numpy(), p_ref[:, t], rtol=2e-5, atol=2e-5)
    neg = (gt[0] - 0.5).to(dev())          # negative ground truth -> data range 2 (dcgan Tanh frames)
    s, p = ops.eval_frames(neg, neg + 0.01)
    assert abs(float(p[0]) - 10 * np.log10(4 / 1e-4)) < 1e-2


def test_moving_mnist_device_compositing_is_bit_exact():
    """SyntheticMovingMNIST.batch_device (host trajectories + dvg_moving_mnist_compose, normalize_data layout fused)
    == utils.normalize_data(host batch), bit for bit, for the same generator state."""
    import utils
    from dvg_amd.data import SyntheticMovingMNIST
    for kw in (dict(seq_len=20, num_digits=2, seed=1), dict(seq_len=7, num_digits=3, seed=5, deterministic=True)):
        host = SyntheticMovingMNIST(**kw)
        devg = SyntheticMovingMNIST(**kw)
        ref, _ = utils.normalize_data(None, torch.cuda.FloatTensor, host.batch(5))
        got = devg.batch_device(5, dev())
        assert len(got) == len(ref) == kw["seq_len"]
        for a, b in zip(ref, got):
            assert a.shape == b.shape == (5, 1, 64, 64) and torch.equal(a, b)
        # the generator state advanced identically: the next batches agree as well
        ref2, _ = utils.normalize_data(None, torch.cuda.FloatTensor, host.batch(2))
        assert all(torch.equal(a, b) for a, b in zip(ref2, devg.batch_device(2, dev())))


@pytest.mark.parametrize("H,C1,C2,Cout,up", [(16, 64, 64, 64, True), (8, 32, 48, 128, False), (8, 512, 512, 256, True)])
def test_conv3x3_addend_equals_concat_conv(H, C1, C2, Cout, up):
    """conv(cat([up(x), skip])) == conv(up(x), W[:, :C1]) + conv(skip, W[:, C1:]) with the second term passed as the
    raw `addend` of dvg_conv3x3_bn_act_v2 (incl. a split-K shape where the finish kernel adds it)."""
    from dvg_amd import ops
    N = 4
    hx = H // 2 if up else H
    x, sk = params.normal(100, N, C1, hx, hx), params.normal(101, N, C2, H, H)
    w = params.normal(102, Cout, C1 + C2, 3, 3, scale=0.05)
    sc, sh = 1 + 0.1 * params.normal(103, Cout), 0.1 * params.normal(104, Cout)
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    ref = F.leaky_relu(F.conv2d(torch.cat([xin, sk], 1).double(), w.double(), padding=1) * sc.double().view(1, -1, 1, 1) +
                       sh.double().view(1, -1, 1, 1), 0.2)
    wd = w.to(dev())
    S = ops.conv3x3(nhwc(sk), None, ops.pack_igemm_weight(wd[:, C1:].contiguous()), None, None, act=ops.ACT_NONE)
    y = ops.conv3x3(nhwc(x), None, ops.pack_igemm_weight(wd[:, :C1].contiguous()), sc.to(dev()), sh.to(dev()),
                    upsample=up, addend=S)
    assert rel_err(y, ref) < 2e-5
    with pytest.raises(RuntimeError):
        ops.conv3x3(nhwc(x), None, ops.pack_igemm_weight(wd[:, :C1].contiguous()), None, None, upsample=up,
                    addend=S[:, :, :-1])


@pytest.mark.parametrize("H,C1,Cout,N", [(4, 512, 512, 4), (8, 256, 256, 3), (16, 128, 128, 2), (32, 64, 64, 2)])
def test_upsample_conv3x3_as_transposed_conv(H, C1, Cout, N):
    """conv3x3(nearest_up2(x), W, pad 1) == convT4x4s2(x, K4) with K4 = W (*) ones(2x2) (weights.k4_packed): the
    x half of the decoder blocks' first convs runs with 4/9 of the MACs.  Checked against the fp64 reference,
    including the raw `addend` and the folded scale / shift, at the four decoder shapes."""
    import torch.nn as nn
    from dvg_amd import ops, weights
    x = params.normal(140, N, C1, H, H)
    w = params.normal(141, Cout, C1 + 64, 3, 3, scale=0.05)          # a concat conv: only W[:, :C1] is the x half
    sc, sh = 1 + 0.1 * params.normal(142, Cout), 0.1 * params.normal(143, Cout)
    S = params.normal(144, N, Cout, 2 * H, 2 * H)
    conv = nn.Conv2d(C1 + 64, Cout, 3, 1, 1).to(dev())
    with torch.no_grad():
        conv.weight.copy_(w)
    ref = F.leaky_relu((F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest").double(), w[:, :C1].double(), padding=1) +
                        S.double()) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1), 0.2)
    y = ops.convT4x4s2(nhwc(x), None, weights.k4_packed(conv.weight, C1), sc.to(dev()), sh.to(dev()), addend=nhwc(S))
    assert rel_err(y, ref) < 2e-5
    y2 = ops.conv3x3(nhwc(x), None, ops.pack_igemm_weight(conv.weight.detach()[:, :C1].contiguous()), sc.to(dev()),
                     sh.to(dev()), upsample=True, addend=nhwc(S))
    assert rel_err(y2, ref) < 2e-5


_PRECISION_PROBE = r"""
import json, sys, torch, torch.nn.functional as F
sys.path.insert(0, %r)
from dvg_amd import ops
dev = torch.device("cuda:0")
out = {}
for (N, H, C, Cout) in [(8, 64, 64, 64), (16, 32, 128, 128), (32, 16, 256, 256), (64, 8, 512, 512)]:
    g = torch.Generator(device="cpu").manual_seed(1000 + H)
    xn = torch.randn(N, C, H, H, generator=g).to(dev)
    w = (torch.randn(Cout, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).to(dev)
    ref = F.conv2d(xn.double(), w.double(), padding=1)
    one, zero = torch.ones(Cout, device=dev), torch.zeros(Cout, device=dev)
    x = ops.to_nhwc(xn)
    forms = {"direct": ops.conv3x3(x, None, ops.pack_igemm_weight(w), one, zero, act=ops.ACT_NONE)}
    if ops.winograd_ok(N, C, H, H, Cout, 4):
        forms["f4"] = ops.conv3x3_winograd(x, ops.winograd_weight(w, 4), one, zero, act=ops.ACT_NONE)
    k4 = torch.zeros((Cout, C, 4, 4), device=dev)
    for ty in range(3):
        for tx in range(3):
            k4[:, :, 2 - ty:4 - ty, 2 - tx:4 - tx] += w[:, :, ty:ty + 1, tx:tx + 1]
    xs = ops.to_nhwc(xn[:, :, ::2, ::2].contiguous())
    refT = F.conv2d(F.interpolate(xs.double(), scale_factor=2, mode="nearest"), w.double(), padding=1)
    yT = ops.convT4x4s2(xs, None, ops.pack_igemm_weight(k4.permute(1, 0, 2, 3).contiguous(), transposed=True), one, zero,
                        act=ops.ACT_NONE)
    for name, y, r in [(k, v, ref) for k, v in forms.items()] + [("convT", yT, refT)]:
        d = y.double() - r
        out[f"{name}/{H}"] = [float(d.abs().max() / r.abs().max()), float(d.pow(2).mean().sqrt() / r.pow(2).mean().sqrt()),
                             float(d.mean() / r.abs().mean())]
print("PROBE " + json.dumps(out))
"""


def test_bf16_triple_products_are_as_accurate_as_the_f32_mfma():
    """ABI 7: the implicit-GEMM kernels of the default library form fp32 products as six bf16 MFMAs on exact bf16 triples.
    Against an fp64 convolution, per layer form (direct 3x3, Winograd F(4x4), the 4-tap transposed form of the upsample convs)
    and per vgg_64 layer shape, their error must not exceed the native f32-MFMA build's (libdvg_hip_f32mfma.so, run in a child
    process on the same inputs): max and rms within 1.25x of it (the measured ratio is 0.8-1.0: the split drops less than one
    fp32 product rounding and the bf16 MFMA rounds its sum once per 16 products, the f32 MFMA once per 2) and a mean error
    (bias) below 5e-7 of the mean magnitude."""
    import json
    import os
    import subprocess
    import sys
    from dvg_amd import _lib
    if os.environ.get("DVG_HIP_LIB"):
        pytest.skip("an alternative build of the library is loaded (DVG_HIP_LIB): this test compares the product build")
    assert _lib.lib().dvg_mfma_mode() == 1, "the product library must be the bf16-triple build"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    native = os.path.join(root, "dvg_amd", "csrc", "libdvg_hip_f32mfma.so")
    assert os.path.exists(native)

    def probe(lib_path):
        env = dict(os.environ)
        env.pop("DVG_HIP_LIB", None)
        if lib_path:
            env["DVG_HIP_LIB"] = lib_path
        r = subprocess.run([sys.executable, "-c", _PRECISION_PROBE % root], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-1500:]
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("PROBE ")][-1][6:])

    x3, f32 = probe(None), probe(native)
    assert set(x3) == set(f32) and len(x3) >= 10
    for k in x3:
        (mx, rms, bias), (mx0, rms0, _) = x3[k], f32[k]
        assert mx < 1.25 * mx0 + 1e-7 and rms < 1.25 * rms0 + 1e-8 and abs(bias) < 5e-7, (k, x3[k], f32[k])
        assert mx < 3e-5 and rms < 1e-5, (k, x3[k])          # the F(4x4) transforms' own rounding dominates: 1-2e-5 max


@pytest.mark.parametrize("N,C,H,Cout", [(4, 64, 16, 128), (3, 128, 8, 64)])
def test_integration_snippet_runs_verbatim(N, C, H, Cout):
    """The binding example of INTEGRATION.md ("What a maintainer of the reference would add"), extracted from the document
    and executed VERBATIM against the library under test: `vgg_layer_eval` must reproduce the reference's eval-mode
    `vgg_layer` (vgg_64.py:5-15: Conv2d(3,1,1) + BatchNorm2d + LeakyReLU(0.2)) as torch composes it in fp64.  Pins the
    document to include/dvg_hip.h's 23-argument dvg_conv3x3_bn_act_v2 and to the packed-weight size."""
    import os
    import torch.nn as nn
    from dvg_amd import _lib
    from tests.test_abi import integration_snippet
    ns, old = {}, os.environ.get("DVG_HIP_LIB")
    os.environ["DVG_HIP_LIB"] = _lib.LIB_PATH
    try:
        exec(compile(integration_snippet(), "INTEGRATION.md", "exec"), ns)
    finally:
        if old is None:
            del os.environ["DVG_HIP_LIB"]
        else:
            os.environ["DVG_HIP_LIB"] = old
    g = torch.Generator().manual_seed(4200 + C)
    conv, bn = nn.Conv2d(C, Cout, 3, 1, 1), nn.BatchNorm2d(Cout)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (9 * C)) ** 0.5)
        conv.bias.copy_(torch.randn(Cout, generator=g) * 0.1)
        bn.weight.copy_(1 + 0.2 * torch.randn(Cout, generator=g))
        bn.bias.copy_(0.1 * torch.randn(Cout, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(Cout, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(Cout, generator=g))
    x = torch.randn(N, C, H, H, generator=g)
    mods = nn.Sequential(conv, bn, nn.LeakyReLU(0.2)).eval()
    with torch.no_grad():
        ref = mods.double()(x.double())
    conv.float().to(dev()), bn.float().to(dev())
    y = ns["vgg_layer_eval"](nhwc(x), conv, bn)
    torch.cuda.synchronize()
    assert y.shape == (N, Cout, H, H) and rel_err(y, ref) < 1e-5, rel_err(y, ref)
