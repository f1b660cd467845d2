"""The decoder's last projection inside the K4 launch that makes its input (dvg_convT4x4s2_bn_act_proj, fused.LAST_PROJ_FUSED)
and the frozen skip halves in F(4x4) form: against fp64 restatements and against the two launches they replace.

The bar of the projection tests: the fused path's max-norm error against fp64 is at most TWICE that of the two-step path
(ops.convT4x4s2 + ops.pixel_proj) on the same inputs.  The kernel repeats pixel_proj's MFMA sequence on the values the K4
launch would have stored, so the two are expected to agree bit for bit; that is asserted as well (docs/DESIGN_NOTES_last_proj.md
has the measured figures)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import params
from tests.common import dev, nhwc, rel_err

pytestmark = pytest.mark.gpu


def _maxerr(a, ref64):
    return float((a.detach().double().cpu() - ref64).abs().max())


@functools.lru_cache(maxsize=None)
def _op_case(N, H, nc, energy):
    """K4 conv + addend + folded BN (scales of both signs) + LeakyReLU + projection (+ gather, bias, Sigmoid): fp64, the two-step
    path and the fused path on the same inputs, computed once per case."""
    from dvg_amd import ops
    from dvg_amd._lib import lib
    T = 9 * nc
    x = params.normal(5000, N, 64, H, H)
    k4 = params.normal(5001, 64, 64, 4, 4, scale=1.0 / 16)              # ConvTranspose2d layout (Cin, Cout, 4, 4)
    S = params.normal(5002, N, 64, 2 * H, 2 * H, scale=0.3)
    sign = torch.where(torch.arange(64) % 3 == 1, -1.0, 1.0)
    sc, sh = (1 + 0.1 * params.normal(5003, 64)) * sign, 0.1 * params.normal(5004, 64)
    w_last = params.normal(5005, 64, nc, 3, 3, scale=1.0 / 24)
    bias = 0.1 * params.normal(5006, nc)
    act64 = F.leaky_relu((F.conv_transpose2d(x.double(), k4.double(), stride=2, padding=1) + S.double()) *
                         sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1), 0.2)
    wm64 = w_last.double().permute(2, 3, 1, 0).reshape(T, 64)
    d64 = act64.permute(0, 2, 3, 1).reshape(-1, 64) @ wm64.t()
    frame64 = torch.sigmoid(F.conv_transpose2d(act64, w_last.double(), stride=1, padding=1) + bias.double().view(1, -1, 1, 1))
    d = lambda t: t.to(dev())   # noqa: E731
    wl, bd = d(w_last), d(bias)
    wm = ops._last_wmat(wl, T)
    wp = ops.pack_igemm_weight(d(k4), transposed=True)
    with ops.tile_policy(energy):
        rows = lib().dvg_conv_stats_rows_v2(ops.MODE_CONVT4S2, N, H, H, 64, 64, 0, 0)       # = workgroups of the launch
        y = ops.convT4x4s2(nhwc(x), None, wp, d(sc), d(sh), addend=nhwc(S))
        d_two = ops.pixel_proj(y, wm)
        d_fused = ops.convT4x4s2_proj(nhwc(x), wp, d(sc), d(sh), wm, addend=nhwc(S))
    f_two = ops.convT_last_two_step(y, None, wl, bd, nc, 3, act=ops.ACT_SIGMOID)
    f_fused = ops.convT_last_two_step(ops.LastProj(d_fused, y.shape, wl), None, wl, bd, nc, 3, act=ops.ACT_SIGMOID)
    torch.cuda.synchronize()
    return dict(rows=rows, d64=d64, frame64=frame64, d_two=d_two.cpu(), d_fused=d_fused.cpu(), f_two=f_two.cpu(),
                f_fused=f_fused.cpu())


# (N, H, energy policy): 8 x 8 -> 16 x 16 takes the 8 x 8 tile, four tiles per image and all four parities at the image borders;
# N = 32 at 16 x 16 under the energy policy is 256 workgroups of the 8 x 16 tile, the threshold at which tile2 picks it
_SHAPES = {"tile8x8": (2, 8, False), "tile8x16": (32, 16, True)}


@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("shape", list(_SHAPES))
def test_fused_projection_against_fp64_and_the_two_step_path(shape, nc):
    N, H, energy = _SHAPES[shape]
    c = _op_case(N, H, nc, energy)
    # the tile that ran: workgroups = N * (H / 8) * (H / tw) * 4 parities
    assert c["rows"] == N * (H // 8) * (H // (16 if shape == "tile8x16" else 8)) * 4, c["rows"]
    assert c["d_fused"].shape == (N * 4 * H * H, 9 * nc)
    e_two, e_fused = _maxerr(c["d_two"], c["d64"]), _maxerr(c["d_fused"], c["d64"])
    print(f"last_proj {shape} nc={nc}: max |d - fp64| two-step {e_two:.3e} fused {e_fused:.3e} (max |d| {float(c['d64'].abs().max()):.3f})")
    assert e_fused <= 2 * e_two, (e_fused, e_two)
    assert torch.equal(c["d_fused"], c["d_two"])


@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("shape", list(_SHAPES))
def test_frame_gathered_from_the_fused_projection(shape, nc):
    N, H, energy = _SHAPES[shape]
    c = _op_case(N, H, nc, energy)
    assert c["f_fused"].shape == (N, nc, 2 * H, 2 * H)
    e_two, e_fused = _maxerr(c["f_two"], c["frame64"]), _maxerr(c["f_fused"], c["frame64"])
    print(f"last_proj frame {shape} nc={nc}: max |frame - fp64| two-step {e_two:.3e} fused {e_fused:.3e}")
    assert e_fused <= 2 * e_two, (e_fused, e_two)
    assert torch.equal(c["f_fused"], c["f_two"])


def _launch_names(fn):
    from dvg_amd import ops
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ops.set_timer(None)
    return out, [r[0] for r in timer.records]


def test_decoder_with_the_switch_on_against_off(monkeypatch):
    """vgg_64 decoder, eval mode, B = 4, frozen skips, two steps.  Bound on |frame_on - frame_off|: both paths hold the bar of the
    op-level test, i.e. each d is within 2 eps |d|_max of fp64 with eps the two-step path's relative error measured there;
    |d|_max <= max |activation| x the projection's largest row 1-norm; a frame value sums 9 taps of d and Sigmoid's slope is at
    most 1/4."""
    from dvg_amd import fused
    from dvg_amd.ops import edge
    from tests.test_gpu_configs import _build
    (enc, dec, *_), _ = _build("vgg", 64, 1, 4, 5100)
    enc.to(dev()).eval(), dec.to(dev()).eval()
    x = params.frames(5110, 4, 1, 64).to(dev())
    vecs = [params.normal(5111 + i, 4, 90, scale=0.5).tanh().to(dev()) for i in range(2)]
    seen = {}
    real_proj = edge.pixel_proj

    def recording_proj(act, wm):
        seen["act"], seen["wm"] = float(act.abs().max()), float(wm.abs().sum(1).max())
        return real_proj(act, wm)
    with torch.no_grad():
        _, skips = enc(x)
        fused.declare_frozen_skips(skips)
        assert fused.LAST_PROJ_FUSED
        dec([vecs[0], skips])       # the first call with frozen skips also computes the hoisted skip halves: not a step to count
        on, names_on = zip(*[_launch_names(lambda v=v: dec([v, skips])) for v in vecs])
        monkeypatch.setattr(fused, "LAST_PROJ_FUSED", False)
        monkeypatch.setattr(edge, "pixel_proj", recording_proj)
        off, names_off = zip(*[_launch_names(lambda v=v: dec([v, skips])) for v in vecs])
    for names in names_on:      # a step: no projection launch, one gather; the K4 launch keeps its name
        assert names.count("pixel_proj") == 0 and names.count("convT_gather") == 1 and names[-2:] == ["convT4x4s2_igemm", "convT_gather"], names
    for a, b in zip(names_on, names_off):
        assert b.count("pixel_proj") == 1 and len(b) == len(a) + 1, (a, b)
    c = _op_case(2, 8, 1, False)
    eps = _maxerr(c["d_two"], c["d64"]) / float(c["d64"].abs().max())
    tol = 0.25 * 9 * 2 * (2 * eps) * seen["act"] * seen["wm"]
    for t, (a, b) in enumerate(zip(on, off)):
        err = float((a - b).abs().max())
        print(f"last_proj decoder step {t}: max |on - off| {err:.3e} (bound {tol:.3e})")
        assert a.shape == (4, 1, 64, 64) and err <= tol, (t, err, tol)
        assert torch.equal(a, b)


def test_eager_rollout_equals_its_captured_graph_bit_for_bit():
    """vgg_64, B = 4, two conditioning and two predicted frames: the eager launch sequence (which takes the fused launch once
    the skips are frozen) and one hipGraph of it."""
    from dvg_amd import fused
    from dvg_amd.rollout import GraphedRollout, sample_rollout
    from tests.test_gpu_configs import _build
    n_past, n_eval = 2, 4
    mods, _ = _build("vgg", 64, 1, 4, 5200)
    for m in mods:
        m.to(dev()).eval()
    xd = [params.frames(5210 + t, 4, 1, 64).to(dev()) for t in range(n_eval)]
    assert fused.LAST_PROJ_FUSED
    with torch.no_grad():
        eager, names = _launch_names(lambda: [f.clone() for f in sample_rollout(*mods, xd, n_past=n_past, n_eval=n_eval)])
        graphed = GraphedRollout(*mods, xd, n_past, n_eval)(xd)
    assert names.count("pixel_proj") == 0 and names.count("convT_gather") == n_eval - n_past, names
    assert len(graphed) == len(eager) == n_eval
    for t in range(n_eval):
        assert torch.equal(graphed[t], eager[t]), t


def test_frozen_skip_half_in_winograd_form_against_fp64():
    """S = conv(skip, W_skip) of the 8 x 8 x 512 -> 512 decoder block at N = 32, the smallest batch at which winograd_tile gives 4
    there (T = 4 N tiles must be a multiple of 128): fused.precompute_skip_half takes F(4x4); its error against fp64 is at most
    twice that of ops.conv3x3_winograd on the 8 x 8, 512 -> 512 layer of tests/test_gpu_winograd.py (same inputs, same bar form:
    rel_err against fp64)."""
    from dvg_amd import fused, ops
    N, C, H = 32, 512, 8
    assert fused.winograd_tile(N, C, H, H, C) == 4 and fused.winograd_tile(N - 1, C, H, H, C) != 4
    x = params.normal(2300, N, C, H, H)
    w = params.normal(2301, C, C, 3, 3, scale=1.2 / (3 * C ** 0.5))
    sc, sh = 1 + 0.1 * params.normal(2302, C), 0.1 * params.normal(2303, C)
    raw64 = F.conv2d(x.double(), w.double(), padding=1)
    ref_layer = F.leaky_relu(raw64 * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1), 0.2)
    y = ops.conv3x3_winograd(nhwc(x), ops.winograd_weight(w.to(dev()), 4), sc.to(dev()), sh.to(dev()))
    e_layer = rel_err(y, ref_layer)
    conv = torch.nn.Conv2d(2 * C, C, 3, 1, 1).to(dev()).eval()
    with torch.no_grad():
        conv.weight[:, :C].copy_(params.normal(2304, C, C, 3, 3, scale=1.2 / (3 * C ** 0.5)))
        conv.weight[:, C:].copy_(w)
        skip = nhwc(x)
        _, names = _launch_names(lambda: fused.precompute_skip_half(conv, skip, "conv3"))
    assert "conv3x3_igemm" not in names and "winograd_gemm" in names, names        # the Winograd launches, not the direct kernel
    S = fused._skip_seen[(id(conv), id(skip))][4]
    e_s = rel_err(S, raw64)
    print(f"skip half F(4x4) 8x8 512->512 N=32: rel err S vs fp64 {e_s:.3e} | conv3x3_winograd layer vs fp64 {e_layer:.3e}")
    assert S.shape == (N, C, H, H) and e_s <= 2 * e_layer, (e_s, e_layer)
