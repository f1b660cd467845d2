"""dvg_amd/weights.py without a GPU: the eval / no-grad blocks and the autograd Functions get ONE object per weight form, built
once per parameter version.  The packers and the conv launches are stubs; the call sites are the real ones."""
import torch


def test_both_paths_get_one_object_per_form_built_once_per_parameter_version(monkeypatch):
    from dvg_amd import autograd as ag
    from dvg_amd import fused, graphs, ops, weights
    graphs.drop_version_keyed_caches()
    packs, seen = [], []
    monkeypatch.setattr(ops, "pack_igemm_weight", lambda w, transposed=False: packs.append(transposed) or torch.zeros(2))
    monkeypatch.setattr(ops, "winograd_weight", lambda w, m: torch.zeros(2))
    for name, arg in (("conv3x3", 2), ("convT4x4s2", 2), ("conv3x3_winograd", 1), ("bn_act_apply", 0)):
        monkeypatch.setattr(ops, name, lambda *a, _i=arg, **k: seen.append(a[_i]) or torch.zeros(1, 4, 2, 2))
    monkeypatch.setattr(fused, "UPCONV_WINOGRAD", False)          # (the K4 form is the one both paths have)
    monkeypatch.setattr(fused, "winograd_tile", lambda *a: 0)
    conv, convt, bn = torch.nn.Conv2d(8, 4, 3, 1, 1), torch.nn.ConvTranspose2d(8, 4, 4, 2, 1), torch.nn.BatchNorm2d(4).eval()
    w, wt = conv.weight, convt.weight

    def forms():
        return [weights.packed(w), *weights.split_packed(w, 4), weights.k4_packed(w, 4), weights.packed(wt, True),
                *weights.split_packed(wt, 4, True), weights.k4_packed(w, 4, adjoint=True), weights.packed(w, True, 0, 4, 1)]
    first = forms()
    assert len(packs) == len(first) == 9 and len({id(f) for f in first}) == 9
    order = [id(first[i]) for i in (0, 2, 1, 3, 4, 6, 5)]     # whole, skip half, x half, K4 forward; transposed: whole, skip half, x half
    x8, x4, sk = torch.zeros(1, 8, 2, 2), torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 2, 2)
    with torch.no_grad():                                     # what fused.py's eval blocks hand to the kernels
        fused.conv3_bn_act(conv, bn, x8)
        fused.precompute_skip_half(conv, sk, "conv3")
        fused.conv3_bn_act(conv, bn, x4, sk)
        fused.conv3_bn_act(conv, bn, x4, sk, upsample=True)
        fused.convT4s2_bn_act(convt, bn, x4)
        fused.precompute_skip_half(convt, sk, "convT4s2")
        fused.convT4s2_bn_act(convt, bn, x4, sk)
    assert [id(f) for f in seen] == order
    seen.clear()
    cfg = {"kind": "conv3", "act": 0, "slope": 0.2, "ds_holder": {"ds": None}, "c1": 4, "bn": bn}

    def block(x, skip, weight, addend, **kw):                 # what autograd.py's Functions hand to the kernels
        return ag._ConvBlock.apply(x, skip, weight, None, bn.weight, bn.bias, addend, dict(cfg, **kw))
    block(x8, None, w, None, upsample=True)
    s_half = ag._SkipHalf.apply(sk, w, cfg)
    block(x4, None, w, s_half)
    block(x4, None, w, s_half, upsample=True)
    block(x4, sk, wt, None, kind="convT4s2")
    ag._SkipHalf.apply(sk, wt, dict(cfg, kind="convT4s2"))
    block(x4, None, wt, s_half, kind="convT4s2")
    assert [id(f) for f in seen if f.dim() == 1] == order     # (the 4-D entries: u handed to the bn_act_apply stub)
    monkeypatch.setattr(fused, "winograd_tile", lambda *a: 4)
    seen.clear()
    with torch.no_grad():
        fused.conv3_bn_act(conv, bn, x8)
        ag._conv3_raw(x8, w, None, False)
    assert seen[0] is seen[1] is weights.winograd(w, 4) is weights.winograd(w, 4, 0, 8)      # U for m = 4; a whole-axis slice is no slice
    assert weights.winograd(w, 4, 0, 4) is not weights.winograd(w, 4, 0, 4, dgrad=True)
    assert weights.packed(w, False, 0, 8, 1) is first[0] and weights.packed(wt, True, 0, 8, 0) is first[4]
    assert all(a is b for a, b in zip(forms(), first)) and len(packs) == 9
    with torch.no_grad():
        w.add_(1)
        wt.add_(1)
    second = forms()
    assert all(a is b for a, b in zip(forms(), second)) and not any(a is b for a, b in zip(first, second))
    assert len(packs) == 18                                   # every form rebuilt exactly once
    graphs.drop_version_keyed_caches()
