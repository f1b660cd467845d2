"""GPU: the live-only form of the F(4x4,3x3) layers that read their input through nearest-x2 upsampling
(docs/DESIGN_NOTES_upconv_live.md).  The 11 transform positions with a == 2 or b == 2 are exactly zero for such an input, so the
producers leave them out of V, the batched GEMM runs 25 of 36 products on the tile of the 36, and the consumers read +0 in their
place.  Everything is bit equality (torch.equal; +-0 compare equal) against the dense kernels, which the precondition test holds
to the identity first; the layer is also held to fp64 at the bar tests/test_gpu_winograd.py uses for the dense form."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import params
from tests import upconv_live_ref as ulr
from tests.common import dev, nhwc, rel_err

pytestmark = pytest.mark.gpu
ACT_LRELU = 1


def _lib():
    from dvg_amd._lib import lib
    return lib()


def _call(fn, *args):
    from dvg_amd._lib import check
    check(fn(*args, torch.cuda.current_stream().cuda_stream), fn.__name__)


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(*shape):
    """What nobody wrote stays NaN, and NaN equals nothing."""
    return torch.full(shape, float("nan"), device=dev())


def _affine(c, seed):
    return (1 + 0.1 * params.normal(seed, c)).to(dev()), (0.1 * params.normal(seed + 1, c)).to(dev())


# ---- the three producers: (dense V, compact V) of one input ---------------------------------------------------------------
# input transform through the upsampling: (N, low-res side, C) - every tile on a border / interior tiles (channels per thread 1),
# then the f32x2 and f32x4 forms (tiles * C / 2, tiles * C / 4 >= 1024 * 256: dvg_winograd_transform_width)
INPUT_CASES = {"border": (32, 4, 64, 1), "interior": (8, 8, 64, 1), "f32x2": (64, 8, 512, 2), "f32x4": (128, 8, 512, 4)}
# hand-over through the upsampling: (N, side of layer L, C) - 8 -> 16 (odd N, two channel blocks per image) and 16 -> 32
UP_CHAIN_CASES = {"8to16": (3, 8, 128), "16to32": (2, 16, 64)}
# decoder stem: samples M (3: the bb >= mrows guard of the last 8-sample workgroup; 17: three workgroups along M)
STEM_CASES = {"m3": 3, "m17": 17}


def _input_pair(name):
    n, h, c, width = INPUT_CASES[name]
    lib = _lib()
    t = n * (2 * h // 4) ** 2
    assert lib.dvg_winograd_transform_width(t, c) == width
    x = ulr.mixed((n, h, h, c), 8700 + n, dev())
    dense, compact = _nan(36, t, c), _nan(25, t, c)
    _call(lib.dvg_winograd_input, _p(x), _p(dense), n, 2 * h, 2 * h, c, 4, 1)
    _call(lib.dvg_winograd_input_up_live, _p(x), _p(compact), n, 2 * h, 2 * h, c)
    return dense, compact


def _up_chain_pair(name):
    n, h, c = UP_CHAIN_CASES[name]
    lib = _lib()
    t = n * (h // 4) ** 2
    mm = ulr.mixed((36, t, c), 8720 + h, dev())
    sc, sh = _affine(c, 8730)
    dense, compact = _nan(36, 4 * t, c), _nan(25, 4 * t, c)
    _call(lib.dvg_winograd_output_up_input, _p(mm), _p(sc), _p(sh), _p(dense), n, h, h, c, ACT_LRELU, 0.2)
    _call(lib.dvg_winograd_output_up_input_live, _p(mm), _p(sc), _p(sh), _p(compact), n, h, h, c, ACT_LRELU, 0.2)
    return dense, compact


def _stem_pair(name):
    m, k, kp, c = STEM_CASES[name], 90, 96, 32
    lib = _lib()
    vec = ulr.mixed((m, k), 8740 + m, dev())
    wt = torch.zeros(kp, 16 * c, device=dev())
    wt[:k] = ulr.mixed((k, 16 * c), 8741, dev())
    sc, sh = _affine(c, 8742)
    dense, compact = _nan(36, 4 * m, c), _nan(25, 4 * m, c)
    _call(lib.dvg_stem_up_winograd_input, _p(vec), k, _p(wt), kp, _p(sc), _p(sh), _p(dense), m, c, k, ACT_LRELU, 0.2)
    _call(lib.dvg_stem_up_winograd_input_live, _p(vec), k, _p(wt), kp, _p(sc), _p(sh), _p(compact), m, c, k, ACT_LRELU, 0.2)
    return dense, compact


PRODUCERS = ([("input", k) for k in INPUT_CASES] + [("up_chain", k) for k in UP_CHAIN_CASES] + [("stem", k) for k in STEM_CASES])
_PAIRS = {}


def _pair(kind, name):
    """(dense V, compact V) of a producer case, computed once and left unchanged (tests 1 and 2 and the planted defect share it)."""
    if (kind, name) not in _PAIRS:
        _PAIRS[kind, name] = {"input": _input_pair, "up_chain": _up_chain_pair, "stem": _stem_pair}[kind](name)
        torch.cuda.synchronize()
    return _PAIRS[kind, name]


@pytest.mark.parametrize("kind,name", PRODUCERS)
def test_precondition_the_dense_kernels_write_exact_zeros_at_the_eleven_positions(kind, name):
    """On the PARENT kernels: inputs of both signs with magnitudes 1e-3 ... 1e3; the 11 dead positions of the dense V are
    exactly zero and no live position is all-zero."""
    dense, _ = _pair(kind, name)
    assert torch.isfinite(dense).all()
    dead = ulr.dead_positions()
    assert not dense[dead].any(), [p for p in dead if dense[p].any()]
    empty = [p for p in range(36) if p not in dead and not dense[p].any()]
    assert not empty, empty


@pytest.mark.parametrize("kind,name", PRODUCERS)
def test_producers_write_the_live_slices_of_the_dense_v(kind, name):
    dense, compact = _pair(kind, name)
    assert torch.equal(compact, ulr.live_slices(dense))


@pytest.mark.parametrize("kind,name", [("input", "interior"), ("up_chain", "8to16"), ("stem", "m3")])
def test_planted_defect_fails_the_producer_check(kind, name):
    dense, compact = _pair(kind, name)
    assert not torch.equal(compact, ulr.live_slices(dense, ulr.PLANTED))


# ---- compact U ------------------------------------------------------------------------------------------------------------
def test_compact_u_is_the_live_slabs_of_the_packed_u():
    from dvg_amd import weights
    w = torch.nn.Parameter(params.normal(8750, 128, 192, 3, 3, scale=0.1).to(dev()))
    for lo, hi in ((0, 64), (None, None)):
        u36, u25 = weights.winograd(w, 4, lo, hi), weights.winograd_live(w, lo, hi)
        assert u25.shape == (25,) + tuple(u36.shape[1:]) and u25.is_contiguous()
        assert torch.equal(u25, ulr.live_slices(u36))
        assert weights.winograd_live(w, lo, hi) is u25          # once per weight version
    with torch.no_grad():
        w.mul_(2.0)
    assert torch.equal(weights.winograd_live(w, 0, 64), ulr.live_slices(weights.winograd(w, 4, 0, 64)))


# ---- the three consumers --------------------------------------------------------------------------------------------------
# (kernel, N, H, C): winograd4_out_in_kernel<8>; the two 16 x 16 chain forms (N * C / 64 below / from 1024 on) and the 32 x 32 one;
# winograd4_output_kernel<false> at 1, 2 and 4 channels per thread
CONSUMER_CASES = {"out_in8": ("chain", 5, 8, 128), "chain16_float": ("chain", 3, 16, 128), "chain16_f32x2": ("chain", 128, 16, 512),
                  "chain32": ("chain", 2, 32, 64), "output_w1": ("output", 8, 16, 64), "output_w2": ("output", 64, 16, 512),
                  "output_w4": ("output", 128, 16, 512)}


def _consumer(name, addend, dead=ulr.DEAD):
    """(dense form on the zero-filled M, compact form on the compact M) of a consumer case."""
    kind, n, h, c = CONSUMER_CASES[name]
    lib = _lib()
    t = n * (h // 4) ** 2
    m25 = ulr.mixed((25, t, c), 8760 + n + h, dev())
    m36 = ulr.zero_filled(m25, dead)
    sc, sh = _affine(c, 8770)
    add = ulr.mixed((n, h, h, c), 8772, dev()) if addend else None
    if kind == "chain":
        a, b = _nan(36, t, c), _nan(36, t, c)
        _call(lib.dvg_winograd_output_input, _p(m36), _p(sc), _p(sh), _p(a), n, h, h, c, ACT_LRELU, 0.2, _p(add))
        _call(lib.dvg_winograd_output_input_live, _p(m25), _p(sc), _p(sh), _p(b), n, h, h, c, ACT_LRELU, 0.2, _p(add))
    else:
        width = {"output_w1": 1, "output_w2": 2, "output_w4": 4}[name]
        assert lib.dvg_winograd_transform_width(t, c) == width
        a, b = _nan(n, h, h, c), _nan(n, h, h, c)
        _call(lib.dvg_winograd_output, _p(m36), _p(sc), _p(sh), _p(a), None, n, h, h, c, ACT_LRELU, 0.2, 4, _p(add), 0)
        _call(lib.dvg_winograd_output_live, _p(m25), _p(sc), _p(sh), _p(b), n, h, h, c, ACT_LRELU, 0.2, _p(add))
    torch.cuda.synchronize()
    return a, b


@pytest.mark.parametrize("addend", [False, True])
@pytest.mark.parametrize("name", sorted(CONSUMER_CASES))
def test_consumers_on_compact_m_equal_the_dense_form_on_zero_filled_m(name, addend):
    a, b = _consumer(name, addend)
    assert torch.isfinite(a).all()
    assert torch.equal(b, a)


@pytest.mark.parametrize("name", ["out_in8", "chain16_float", "output_w1"])
def test_planted_defect_fails_the_consumer_check(name):
    a, b = _consumer(name, True, ulr.PLANTED)
    assert not torch.equal(b, a)


# ---- the layer --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("energy", [False, True])
@pytest.mark.parametrize("N,H,C1,Cout", [(32, 4, 64, 64), (8, 8, 64, 128)])
def test_layer_live_only_equals_dense_and_matches_fp64(N, H, C1, Cout, energy):
    """conv3x3_winograd(upsample=True, addend=...) on the 25 live positions against the dense form (plain output and the
    hand-over to the next layer, both tile policies) and against fp64 interpolate + conv2d at the dense form's bar (1e-4 of
    the output's largest magnitude, tests/test_gpu_winograd.py)."""
    from dvg_amd import ops
    x = params.normal(8800, N, C1, H, H)
    w = params.normal(8801, Cout, C1, 3, 3, scale=1.2 / (3 * C1 ** 0.5))
    sc, sh = 1 + 0.1 * params.normal(8803, Cout), 0.1 * params.normal(8804, Cout)
    S = params.normal(8805, N, Cout, 2 * H, 2 * H, scale=0.3)
    d = lambda t: t.to(dev())   # noqa: E731
    up = F.interpolate(x, scale_factor=2, mode="nearest").double()
    ref = F.leaky_relu((F.conv2d(up, w.double(), padding=1) + S.double()) * sc.double().view(1, -1, 1, 1) +
                       sh.double().view(1, -1, 1, 1), 0.2)
    assert ops.winograd_ok(N, C1, 2 * H, 2 * H, Cout, 4) and ops.winograd_chain_ok(N, Cout, 2 * H, 2 * H)
    u36 = ops.winograd_weight(d(w), 4)
    u25 = u36[list(ops.LIVE_POSITIONS)].contiguous()
    xd, Sd = nhwc(x), nhwc(S)
    with ops.tile_policy(energy):
        y36 = ops.conv3x3_winograd(xd, u36, d(sc), d(sh), upsample=True, addend=Sd)
        y25 = ops.conv3x3_winograd(xd, u25, d(sc), d(sh), upsample=True, addend=Sd, live=True)
        v36 = ops.conv3x3_winograd(xd, u36, d(sc), d(sh), upsample=True, addend=Sd, to_v=True)
        v25 = ops.conv3x3_winograd(xd, u25, d(sc), d(sh), upsample=True, addend=Sd, to_v=True, live=True)
        y25n = ops.conv3x3_winograd(xd, u25, d(sc), d(sh), upsample=True, live=True)         # no addend
        y36n = ops.conv3x3_winograd(xd, u36, d(sc), d(sh), upsample=True)
    assert torch.equal(y25, y36) and torch.equal(y25n, y36n)
    assert isinstance(v25, ops.WinoV) and not v25.up and not v25.live and v25.v.shape == v36.v.shape
    assert torch.equal(v25.v, v36.v)
    e = rel_err(y25, ref)
    print(f"upconv live layer N={N} {H}->{2 * H} {C1}->{Cout} energy={energy}: rel err vs fp64 {e:.3e}")
    assert e < 1e-4, e
    with pytest.raises(RuntimeError):
        ops.conv3x3_winograd(xd, u36, d(sc), d(sh), upsample=True, live=True)               # live needs the 25 slabs
    with pytest.raises(RuntimeError):
        ops.conv3x3_winograd(xd, u25, d(sc), d(sh), upsample=True)                          # ... and only then


def test_layer_takes_a_live_winov_from_the_layer_before():
    """8 x 8 layer -> (hand-over through the upsampling, live) -> 16 x 16 x half: equal to the dense hand-over."""
    from dvg_amd import ops
    N, C, Cmid, Cout, H = 32, 64, 64, 64, 8
    x = params.normal(8810, N, C, H, H)
    w1 = params.normal(8811, Cmid, C, 3, 3, scale=1.2 / (3 * C ** 0.5))
    w2 = params.normal(8812, Cout, Cmid, 3, 3, scale=1.2 / (3 * Cmid ** 0.5))
    d = lambda t: t.to(dev())   # noqa: E731
    s1, b1 = _affine(Cmid, 8813)
    s2, b2 = _affine(Cout, 8815)
    add = nhwc(params.normal(8817, N, Cout, 2 * H, 2 * H, scale=0.3))
    u1, u2 = ops.winograd_weight(d(w1), 4), ops.winograd_weight(d(w2), 4)
    u2l = u2[list(ops.LIVE_POSITIONS)].contiguous()
    v36 = ops.conv3x3_winograd(nhwc(x), u1, s1, b1, to_v="up")
    v25 = ops.conv3x3_winograd(nhwc(x), u1, s1, b1, to_v="up", up_live=True)
    assert v25.up and v25.live and v25.v.shape[0] == 25 and torch.equal(v25.v, ulr.live_slices(v36.v))
    y36 = ops.conv3x3_winograd(v36, u2, s2, b2, upsample=True, addend=add)
    y25 = ops.conv3x3_winograd(v25, u2l, s2, b2, upsample=True, addend=add, live=True)
    assert torch.equal(y25, y36)
    with pytest.raises(RuntimeError):      # a live WinoV needs the live form
        ops.conv3x3_winograd(v25, u2, s2, b2, upsample=True, addend=add)


# ---- tile pinning -----------------------------------------------------------------------------------------------------------
def test_gemm_of_25_on_the_tile_of_36_gives_the_live_slices_of_the_dense_m():
    """(NB 25 as 36, H 16, W 16, 512 -> 512), T = 256, ENERGY: the smallest shape at which the tile would otherwise flip
    (36 * 2 * 4 = 288 >= 256 workgroups of the 128 x 128 tile, 25 * 2 * 4 = 200 < 256)."""
    from dvg_amd import ops
    lib = _lib()
    t, cin, cout = 256, 512, 512
    v36 = ulr.mixed((36, t, cin), 8820, dev())
    u36 = ops.winograd_weight(params.normal(8821, cout, cin, 3, 3, scale=0.05).to(dev()), 4)
    v25, u25 = ulr.live_slices(v36), ulr.live_slices(u36)
    m36, m25 = _nan(36, t, cout), _nan(25, t, cout)
    with ops.tile_policy(True):
        tw, nt, ni = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert lib.dvg_gemm_batched_plan_as(25, 36, t // 16, 16, cin, cout, ctypes.byref(tw), ctypes.byref(nt), ctypes.byref(ni)) == 0
        if lib.dvg_mfma_mode() == 1:
            assert (tw.value, nt.value) == (16, 2)
        _call(lib.dvg_gemm_batched_k16, _p(v36), _p(u36), _p(m36), 36, t // 16, 16, cin, cout)
        _call(lib.dvg_gemm_batched_k16_as, _p(v25), _p(u25), _p(m25), 25, 36, t // 16, 16, cin, cout)
    torch.cuda.synchronize()
    assert torch.isfinite(m36).all()
    assert torch.equal(m25, ulr.live_slices(m36))


# ---- the rollout ------------------------------------------------------------------------------------------------------------
LIVE_ENTRY_POINTS = ("dvg_stem_up_winograd_input_live", "dvg_winograd_output_up_input_live", "dvg_gemm_batched_k16_as",
                     "dvg_winograd_output_input_live")


@pytest.mark.parametrize("energy", [False, True])
@pytest.mark.parametrize("B,wino_max", [(4, 16), (32, 16), (32, 32)])
def test_rollout_frames_with_the_switch_on_equal_frames_with_it_off(B, wino_max, energy, monkeypatch):
    """vgg_64, two conditioning and two predicted frames, frames with fused.UPCONV_WINO_LIVE on equal frames with it off under
    both tile policies.  B = 4 is the batch of the other rollout tests (tests/test_gpu_conv3_wx.py); the Winograd form of these layers needs whole 128-row GEMM tiles
    (ops.winograd_ok: T % 128 == 0, a requirement of the GEMM kernel and not a floor that a test can lower), which B = 4 does
    not give (16 and 64 tiles), so nothing live runs there and the frames are equal because the launches are the same.  B = 32
    is the smallest batch at which both layers take the form (128 and 512 tiles): there the entry points the launches went
    through show that the live-only kernels ran - stem -> upc2 and upc2 -> upc3 hand-overs, both 25-position GEMMs and both
    consumers - and that none ran with the switch off.  wino_max = 32: fused._UPCONV_WINO_MAX raised, so that upc4's first conv
    (32 x 32) takes the form too, fed by the 16 -> 32 hand-over and read by the 32 x 32 consumer."""
    from dvg_amd import fused, ops
    from tests.test_gpu_configs import _build
    (enc, dec, *_), _ = _build("vgg", 64, 1, B, 8900)
    enc.to(dev()).eval(), dec.to(dev()).eval()
    frames = [params.frames(8910 + i, B, 1, 64).to(dev()) for i in range(2)]
    vecs = [params.normal(8920 + i, B, 90, scale=0.5).tanh().to(dev()) for i in range(2)]

    def rollout():
        fused.clear_skip_hoist_cache()
        ops.clear_skip_proj_cache()
        out = []
        timer = ops.KernelTimer()
        with torch.no_grad(), ops.tile_policy(energy):
            for f in frames:
                _, skips = enc(f)
            fused.declare_frozen_skips(skips)
            ops.set_timer(timer)
            try:
                for v in vecs:
                    x = dec([v, skips])
                    out.append(x)
                    enc(x)
            finally:
                ops.set_timer(None)
        torch.cuda.synchronize()
        return [o.cpu() for o in out], timer.entry_points(), len(timer.records)

    monkeypatch.setattr(fused, "_UPCONV_WINO_MAX", wino_max)
    monkeypatch.setattr(fused, "UPCONV_WINO_LIVE", False)
    off, ep_off, n_off = rollout()
    monkeypatch.setattr(fused, "UPCONV_WINO_LIVE", True)
    on, ep_on, n_on = rollout()
    fused.clear_skip_hoist_cache()
    ops.clear_skip_proj_cache()
    assert all(torch.equal(a, b) for a, b in zip(on, off))
    assert n_on == n_off                                        # no launch more
    assert not any(ep_off.get(k) for k in LIVE_ENTRY_POINTS + ("dvg_winograd_output_live", "dvg_winograd_input_up_live"))
    if B == 32 and fused.WINOGRAD == 4 and fused.WINOGRAD_CHAIN and fused.SKIP_HOIST and fused.UPCONV_WINOGRAD and fused._CHAIN_LEVEL >= 3:
        stem, up, gemm, oi = (ep_on.get(k, 0) for k in LIVE_ENTRY_POINTS)
        # per decoder call: stem -> upc2 and upc2 -> upc3 (wino_max = 32: and upc3 -> upc4) hand over a live V, each feeds one
        # 25-position GEMM, each of those one live consumer; and every launch of these families that was dense with the switch off is a live one now
        assert (stem, up, gemm, oi) == ((2, 2, 4, 4) if wino_max == 16 else (2, 4, 6, 6)), dict(ep_on)
        assert ep_off["dvg_stem_up_winograd_input"] == stem and not ep_on.get("dvg_stem_up_winograd_input")
        assert ep_off["dvg_winograd_output_up_input"] == up and not ep_on.get("dvg_winograd_output_up_input")
        assert ep_off["dvg_gemm_batched_k16"] == ep_on["dvg_gemm_batched_k16"] + gemm
        assert ep_off["dvg_winograd_output_input"] == ep_on["dvg_winograd_output_input"] + oi
    elif B == 4:
        assert not any(ep_on.get(k) for k in LIVE_ENTRY_POINTS), dict(ep_on)
