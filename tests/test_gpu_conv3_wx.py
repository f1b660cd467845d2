"""The WX form of the direct 3x3 conv (dvg_conv3x3_bn_act_wx, dvg_conv3x3_first_pair_wx: 1-D Winograd F(2,3) along x inside the
kernel) against fp64 restatements and against the entry points it stands in for.

The bar: on the same inputs the max-norm error against fp64 of the WX kernel is at most TWICE that of the direct kernel
(dvg_conv3x3_bn_act_v2 / dvg_conv3x3_first_pair) - the fused-vs-two-step rule of tests/test_gpu_last_proj.py.  The planted
defect (v1 and v2 exchanged in the fp64 restatement of the WX algorithm, tests/test_conv3_wx_host.py: wx_conv) must fail the same
bar.  docs/DESIGN_NOTES_conv3_wx.md has the measured figures."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import params
from tests.common import dev, nhwc
from tests.test_conv3_wx_host import pack_wx_numpy, wx_conv

pytestmark = pytest.mark.gpu


def _maxerr(a, ref64):
    return float((a.detach().double().cpu() - ref64).abs().max())


def _holds_bar(out, parent, ref64):
    return _maxerr(out, ref64) <= 2 * _maxerr(parent, ref64)


def _affine(cout, seed):
    sign = torch.where(torch.arange(cout) % 3 == 1, -1.0, 1.0)
    return (1 + 0.1 * params.normal(seed, cout)) * sign, 0.1 * params.normal(seed + 1, cout)


def _post(conv64, sc, sh, S=None):
    v = conv64 if S is None else conv64 + S.double()
    return F.leaky_relu(v * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1), 0.2)


# (N, H, W, Cin, Cout): one tile and one chunk; four tiles per image (every halo edge and corner) and four chunks (the A planes
# are rewritten three times); two Cout blocks
_CASES = {"one_tile": (1, 8, 16, 16, 64), "four_tiles": (2, 16, 32, 64, 64), "two_cout_blocks": (1, 8, 16, 64, 128)}


@functools.lru_cache(maxsize=None)
def _case(name):
    from dvg_amd import ops
    N, H, W, Cin, Cout = _CASES[name]
    x = params.normal(7200, N, Cin, H, W)
    w = params.normal(7201, Cout, Cin, 3, 3, scale=1.0 / (3 * Cin ** 0.5))
    S = params.normal(7202, N, Cout, H, W, scale=0.3)
    sc, sh = _affine(Cout, 7203)
    conv64 = F.conv2d(x.double(), w.double(), padding=1)
    d = lambda t: t.to(dev())   # noqa: E731
    wd = d(w)
    wp, wx = ops.pack_igemm_weight(wd), ops.pack_wx_weight(wd)
    out = {"conv64": conv64, "plain64": _post(conv64, sc, sh), "add64": _post(conv64, sc, sh, S),
           "wx_packed": wx.cpu(), "w": w, "x": x, "sc": sc, "sh": sh}
    with ops.tile_policy(True):
        out["plain_direct"] = ops.conv3x3(nhwc(x), None, wp, d(sc), d(sh)).cpu()
        out["add_direct"] = ops.conv3x3(nhwc(x), None, wp, d(sc), d(sh), addend=nhwc(S)).cpu()
        out["plain_wx"] = ops.conv3x3_wx(nhwc(x), wx, d(sc), d(sh)).cpu()
        out["add_wx"] = ops.conv3x3_wx(nhwc(x), wx, d(sc), d(sh), addend=nhwc(S)).cpu()
        out["plain_wx_again"] = ops.conv3x3_wx(nhwc(x), wx, d(sc), d(sh)).cpu()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(_CASES))
def test_device_packer_writes_the_numpy_image(name):
    c = _case(name)
    got = c["wx_packed"].contiguous().numpy().view(np.uint16)
    assert np.array_equal(got.reshape(-1), pack_wx_numpy(c["w"].numpy()).reshape(-1))


@pytest.mark.parametrize("form", ["plain", "add"])
@pytest.mark.parametrize("name", list(_CASES))
def test_wx_against_fp64_and_the_direct_kernel(name, form):
    c = _case(name)
    ref = c[form + "64"]
    e_dir, e_wx = _maxerr(c[form + "_direct"], ref), _maxerr(c[form + "_wx"], ref)
    print(f"conv3_wx {name} {form}: max |y - fp64| direct {e_dir:.3e} wx {e_wx:.3e} (max |y| {float(ref.abs().max()):.3f})")
    assert c[form + "_wx"].shape == ref.shape
    assert _holds_bar(c[form + "_wx"], c[form + "_direct"], ref), (e_wx, e_dir)


@pytest.mark.parametrize("name", list(_CASES))
def test_planted_defect_fails_the_bar(name):
    c = _case(name)
    bad = wx_conv(c["x"].double().numpy(), c["w"].double().numpy(), swap_v12=True)
    good = wx_conv(c["x"].double().numpy(), c["w"].double().numpy())
    assert _holds_bar(_post(torch.from_numpy(good), c["sc"], c["sh"]).float(), c["plain_direct"], c["plain64"])
    assert not _holds_bar(_post(torch.from_numpy(bad), c["sc"], c["sh"]).float(), c["plain_direct"], c["plain64"])


# FIRST: (N, H, W, y_from)
_FIRST = {"frames2_from0": (2, 16, 32, 0), "frames2_from1": (2, 16, 32, 1), "frame1": (1, 8, 16, 0)}


@functools.lru_cache(maxsize=None)
def _first_case(name):
    from dvg_amd import ops
    from dvg_amd._lib import lib
    N, H, W, y_from = _FIRST[name]
    pool = name != "frame1"
    fr = params.frames(7300, N, 1, max(H, W))[:, :, :H, :W].contiguous()
    w0 = params.normal(7301, 64, 1, 3, 3, scale=1.0 / 3)
    w1 = params.normal(7302, 64, 64, 3, 3, scale=1.0 / 24)
    sc0, sh0 = _affine(64, 7303)
    sc1, sh1 = _affine(64, 7305)
    a64 = _post(F.conv2d(fr.double(), w0.double(), padding=1), sc0, sh0)
    y64 = _post(F.conv2d(a64, w1.double(), padding=1), sc1, sh1)
    d = lambda t: t.to(dev())   # noqa: E731
    w0t = d(w0).reshape(64, 9).t().contiguous()
    wp, wx = ops.pack_igemm_weight(d(w1)), ops.pack_wx_weight(d(w1))
    # the direct entry point below its 512-workgroup floor is called through the library: the floor is a choice of tile, not a
    # limit of the kernel, and the WX kernel's small cases need their counterpart
    y_d = ops.nhwc_empty(N - y_from, 64, H, W, dev())
    yp_d = ops.nhwc_empty(N, 64, H // 2, W // 2, dev()) if pool else None
    keep = [d(fr), d(sc0), d(sh0), d(sc1), d(sh1)]
    args = lambda wgt, y, yp: (keep[0].data_ptr(), w0t.data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), wgt.data_ptr(),   # noqa: E731
                               keep[3].data_ptr(), keep[4].data_ptr(), y.data_ptr(), None if yp is None else yp.data_ptr(),
                               N, H, W, 64, ops.ACT_LRELU, 0.2, y_from, torch.cuda.current_stream().cuda_stream)
    out = {"y64": y64[y_from:], "yp64": F.max_pool2d(y64, 2) if pool else None, "direct": None}
    with ops.tile_policy(True):
        code = lib().dvg_conv3x3_first_pair(*args(wp, y_d, yp_d))
        if code == 0:
            out["direct"] = (y_d.cpu(), None if yp_d is None else yp_d.cpu())
        res = ops.conv3x3_first_pair_wx(keep[0], w0t, keep[1], keep[2], wx, keep[3], keep[4], pool=pool, y_from=y_from)
        # the two-launch direct path on the same inputs: what the WX kernel replaces where the fused direct one refuses the shape
        a = ops.conv3x3_first(keep[0], d(w0), keep[1], keep[2])
        two = ops.conv3x3(a, None, wp, keep[3], keep[4], pool=pool)
    torch.cuda.synchronize()
    y, yp = res if pool else (res, None)
    ty, typ = two if pool else (two, None)
    out["wx"] = (y.cpu(), None if yp is None else yp.cpu())
    out["two"] = (ty.cpu()[y_from:], None if typ is None else typ.cpu())
    return out


@pytest.mark.parametrize("name", list(_FIRST))
def test_first_pair_wx_against_fp64_and_the_direct_first_pair(name):
    c = _first_case(name)
    parent = c["direct"] if c["direct"] is not None else c["two"]
    which = "first_pair" if c["direct"] is not None else "first + conv3x3 (first_pair refuses fewer than 512 workgroups)"
    for k, ref in ((0, c["y64"]), (1, c["yp64"])):
        if ref is None:
            continue
        e_dir, e_wx = _maxerr(parent[k], ref), _maxerr(c["wx"][k], ref)
        print(f"conv3_wx first {name} {'pool' if k else 'y'}: max |y - fp64| {which} {e_dir:.3e} wx {e_wx:.3e}")
        assert c["wx"][k].shape == ref.shape
        assert _holds_bar(c["wx"][k], parent[k], ref), (name, k, e_wx, e_dir)


def test_two_runs_are_bit_equal_and_eager_equals_graph_replay():
    from dvg_amd import ops
    c = _case("four_tiles")
    assert torch.equal(c["plain_wx"], c["plain_wx_again"])
    N, H, W, Cin, Cout = _CASES["four_tiles"]
    x, sc, sh = nhwc(c["x"]), c["sc"].to(dev()), c["sh"].to(dev())
    wx = c["wx_packed"].to(dev())
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), ops.tile_policy(True):
        ops.conv3x3_wx(x, wx, sc, sh)                     # warm-up: the kernel's attributes are set outside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            y = ops.conv3x3_wx(x, wx, sc, sh)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), c["plain_wx"])


def test_rollout_with_the_variant_on_against_off(monkeypatch):
    """vgg_64, B = 4, n_past = 2, two predicted steps, ENERGY policy: frames agree to the cross-policy bound (5e-6 max-norm,
    DESIGN.md 3.1e).  B = 4 is below the chooser's workgroup floor, so the floor is lowered for the test; the launches are
    counted to make sure the variant ran."""
    from dvg_amd import fused, ops
    from tests.test_gpu_configs import _build
    (enc, dec, *_), _ = _build("vgg", 64, 1, 4, 7400)
    enc.to(dev()).eval(), dec.to(dev()).eval()
    frames = [params.frames(7410 + i, 4, 1, 64).to(dev()) for i in range(2)]
    vecs = [params.normal(7420 + i, 4, 90, scale=0.5).tanh().to(dev()) for i in range(2)]
    calls = []
    real_wx = ops.conv3x3_wx

    def counting_wx(*a, **k):
        calls.append(1)
        return real_wx(*a, **k)

    def rollout():
        out = []
        with torch.no_grad(), ops.tile_policy(True):
            for f in frames:                              # n_past = 2 conditioning frames; the last one's skips are kept
                _, skips = enc(f)
            fused.declare_frozen_skips(skips)
            for v in vecs:                                # two predicted steps on the frozen skips, each frame encoded again
                x = dec([v, skips])
                out.append(x)
                enc(x)
        torch.cuda.synchronize()
        return [o.cpu() for o in out]

    monkeypatch.setattr(fused, "CONV3_WX", False)
    off = rollout()
    assert not calls
    monkeypatch.setattr(fused, "CONV3_WX", True)
    monkeypatch.setattr(fused, "CONV3_WX_MIN_WGS", 1)
    monkeypatch.setattr(ops, "conv3x3_wx", counting_wx)
    on = rollout()
    assert calls, "the WX variant did not run"
    err = max(float((a - b).abs().max()) for a, b in zip(on, off))
    print(f"conv3_wx rollout on / off: max |frame_on - frame_off| {err:.3e}")
    assert err <= 5e-6, err
