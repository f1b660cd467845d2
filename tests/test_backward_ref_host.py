"""CPU-only checks of tests/backward_ref.py, for every case tests/test_gpu_wgrad.py runs on the device: the fp32 yardstick
passes its own bar, every planted defect fails it, the bar is not vacuous, the packed slab layout is right (against an
explicit loop over taps that shares no code with the reference), and each case still has the edge it was chosen for
(dvg_conv_wgrad_splits_multi is host-only code).  Also: the sizing calls and the dispatcher of dvg_conv_wgrad_multi agree
on which (mode, map) has a kernel."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import params
from tests import backward_ref as br
from tests.backward_ref import MODE_CONV3, MODE_CONV4S2, MODE_CONVT4S2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from dvg_amd._lib import lib
    return lib()


# ---- the bar ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", br.CASE_NAMES)
def test_yardstick_passes_and_the_bar_is_not_vacuous(name):
    """The fp32 yardstick is within its own bar, and max(1.5 e32, worst e32 of the kind) <= 0.5 e_plane: the cap never bites, so
    the bar is set by the yardstick AND rejects a lost bf16 plane."""
    f = br.case_figures(name)
    worst = br.kind_worst_e32(br.CASE_BY_NAME[name]["mode"])
    b = br.case_bar(name)
    print(f"{name}: e32 {f['e32']:.2e} worst-of-kind {worst:.2e} e_plane {f['e_plane']:.2e} bar {b:.2e}")
    assert f["e32"] <= b
    assert max(br.YARDSTICK_RATIO * f["e32"], worst) <= 0.5 * f["e_plane"], (f["e32"], worst, f["e_plane"])
    assert b == max(br.YARDSTICK_RATIO * f["e32"], worst)
    assert f["e_plane"] > b


@pytest.mark.parametrize("name", br.CASE_NAMES)
def test_every_planted_defect_fails_the_bar(name):
    case = br.CASE_BY_NAME[name]
    xs, skips, dus = br.wgrad_inputs(case)
    ref, b = br.case_figures(name)["ref"], br.case_bar(name)
    ti = case["tile"][0]
    for kind in br.PLANTS:
        if kind == "plane":
            e = br.case_figures(name)["e_plane"]
        elif kind == "tail" and case["n"] % ti == 0:
            with pytest.raises(ValueError):      # whole tiles only: nothing to drop
                br.plant(kind, case["mode"], xs, skips, dus, case["up"], ti=ti)
            continue
        else:
            e = br.blockwise_err(br.plant(kind, case["mode"], xs, skips, dus, case["up"], ti=ti), ref)
        print(f"{name}: planted {kind}: {e:.2e} (bar {b:.2e})")
        assert e > b, (kind, e, b)


def test_bar_formula():
    assert br.bar(1e-6, 1.2e-6, 8e-6) == 1.5e-6          # 1.5 x the case's own yardstick
    assert br.bar(1e-7, 1.2e-6, 8e-6) == 1.2e-6          # floored at the kind's worst
    assert br.bar(4e-6, 1.2e-6, 8e-6) == 4e-6            # capped at half the lost plane


def test_blockwise_err_is_not_diluted_by_other_blocks():
    ref = torch.ones(9, 128, 192, dtype=torch.float64)
    ref[0] *= 1000.0                                     # one loud tap
    a = ref.clone()
    a[5, 70, 130] += 0.01                                # a 1 % error in a quiet block
    assert abs(br.blockwise_err(a, ref) - 0.01) < 1e-12
    from tests.common import rel_err
    assert rel_err(a, ref) < 2e-5                        # the tensor-wide figure does not see it
    a[3, 0, 0] = float("nan")
    assert br.blockwise_err(a, ref) == float("inf")
    # partial tiles (thin-layer shapes)
    r2 = torch.arange(1, 1 + 9 * 3 * 4, dtype=torch.float64).reshape(9, 3, 4)
    a2 = r2.clone()
    a2[8, 2, 3] *= 1.5
    assert abs(br.blockwise_err(a2, r2) - 0.5) < 1e-12


def test_round16_keeps_sixteen_significant_bits():
    x = params.normal(11, 4096)
    r = br.round16(x)
    assert bool(((r.view(torch.int32) & 0xFF) == 0).all())
    rel = ((r.double() - x.double()).abs() / x.double().abs()).max()
    assert 2.0 ** -19 < float(rel) <= 2.0 ** -16
    assert torch.equal(br.round16(r), r)


# ---- the slab layout, independently ----------------------------------------------------------------------------------------
def _wgrad_by_tap_loop(mode, inp, du):
    """The packed slab by an explicit loop over taps, from the convolutions' index formulas (fp64):
      conv3:    out[y][x]   += W[co][ci][a][b] in[y + a - 1][x + b - 1]        slab[a * 3 + b][co][ci] = dW[co][ci][a][b]
      conv4s2:  out[y][x]   += W[co][ci][a][b] in[2 y + a - 1][2 x + b - 1]    slab[a * 4 + b][co][ci] = dW[co][ci][a][b]
      convT4s2: out[2 i - 1 + k][2 j - 1 + l] += W[ci][co][k][l] in[i][j]      slab[(3 - k) * 4 + (3 - l)][co][ci] = dW[ci][co][k][l]"""
    inp, du = inp.double(), du.double()
    n, cin, h, w = inp.shape
    cout = du.shape[1]
    k = br.KSIZE[mode]
    slab = torch.zeros(k * k, cout, cin, dtype=torch.float64)
    if mode == MODE_CONVT4S2:
        dup = F.pad(du, (1, 1, 1, 1))                    # dup[y + 1] = du[y]
        for kk in range(4):
            for ll in range(4):
                win = dup[:, :, kk:kk + 2 * h:2, ll:ll + 2 * w:2]          # du[2 i - 1 + k][2 j - 1 + l]
                slab[(3 - kk) * 4 + (3 - ll)] = torch.einsum("noyx,niyx->oi", win, inp)
        return slab
    s = 2 if mode == MODE_CONV4S2 else 1
    ho, wo = du.shape[2:]
    ip = F.pad(inp, (1, 1, 1, 1))
    for a in range(k):
        for b in range(k):
            win = ip[:, :, a:a + s * ho:s, b:b + s * wo:s]
            slab[a * k + b] = torch.einsum("noyx,niyx->oi", du, win)
    return slab


@pytest.mark.parametrize("mode", [MODE_CONV3, MODE_CONV4S2, MODE_CONVT4S2])
@pytest.mark.parametrize("concat_up", [False, True])
def test_slab_layout_against_an_explicit_tap_loop(mode, concat_up):
    """2 images, 4x4, 4 channels (and, for the concat / upsampling forms, x and a skip of 4 channels each)."""
    up = concat_up and mode == MODE_CONV3
    x = params.normal(21, 2, 4, 2 if up else 4, 2 if up else 4)
    skip = params.normal(22, 2, 4, 4, 4) if concat_up else None
    ho = {MODE_CONV3: 4, MODE_CONV4S2: 2, MODE_CONVT4S2: 8}[mode]
    dus = [params.normal(23 + i, 2, 6, ho, ho) for i in range(2)]
    ref = br.wgrad_ref(mode, [x, x * 0.5], None if skip is None else [skip, skip], dus, up)
    inp = br.conv_input(x, skip, up)
    loop = _wgrad_by_tap_loop(mode, inp, dus[0]) + _wgrad_by_tap_loop(mode, inp * 0.5 if skip is None else
                                                                      br.conv_input(x * 0.5, skip, up), dus[1])
    assert ref.shape == loop.shape == (br.KSIZE[mode] ** 2, 6, 4 + (4 if concat_up else 0))
    assert float((ref - loop).abs().max()) <= 1e-12 * float(loop.abs().max())
    # and back to the nn layout through the finish reference (kind 0 / kind 1 addressing with a channel slice)
    kind = 1 if mode == MODE_CONVT4S2 else 0
    k = br.KSIZE[mode]
    cin = ref.shape[2]
    w = torch.zeros(br.weight_shape(mode, cin, 6), dtype=torch.float64, requires_grad=True)
    sum((br.conv_forward(mode, i_.double(), w) * d.double()).sum() for i_, d in
        ((inp, dus[0]), (br.conv_input(x * 0.5, skip, up), dus[1]))).backward()
    wide = torch.zeros(br.weight_shape(mode, cin + 3, 6), dtype=torch.float64)
    out, _, mask = br.wgrad_finish_ref(ref[None], wide, kind, k, k, cin + 3, 2, 0.0)
    got = out[2:2 + cin] if kind == 1 else out[:, 2:2 + cin]
    assert float((got - w.grad).abs().max()) <= 1e-12 * float(w.grad.abs().max())
    assert float(out[~mask].abs().max()) == 0.0 and int(mask.sum()) == w.grad.numel()


def test_small_references_are_adjoints_of_their_forwards():
    # upsample: <up(x), g> == <x, up_bwd(g)>
    x, g = params.normal(31, 2, 3, 4, 5).double(), params.normal(32, 2, 3, 8, 10).double()
    dx, mag = br.upsample2x_bwd_ref(g)
    lhs = (F.interpolate(x, scale_factor=2, mode="nearest") * g).sum()
    assert abs(float(lhs - (x * dx).sum())) < 1e-10 and bool((mag >= dx.abs()).all())
    # K4: <dK4, K4(W)> == <k4_to_w3(dK4), W>, and K4 really is upsample + conv3x3 as a transposed conv
    w, dk4p = params.normal(33, 5, 4, 3, 3).double(), params.normal(34, 16, 5, 4).double()
    dw, _ = br.k4_to_w3_ref(dk4p)
    assert abs(float((br.k4_unpack(dk4p) * br.k4_of_w3(w)).sum() - (dw * w).sum())) < 1e-10
    xi = params.normal(35, 2, 4, 3, 3).double()
    a = F.conv2d(F.interpolate(xi, scale_factor=2, mode="nearest"), w, None, 1, 1)
    b = F.conv_transpose2d(xi, br.k4_of_w3(w).permute(1, 0, 2, 3), None, 2, 1)
    assert float((a - b).abs().max()) < 1e-12
    # the packed dK4 slab is the kind-1 slab of that transposed conv
    g2 = params.normal(36, 2, 5, 6, 6).double()
    slab = br.wgrad_ref(MODE_CONVT4S2, [xi], None, [g2])
    w3 = torch.zeros(5, 4, 3, 3, dtype=torch.float64, requires_grad=True)
    (F.conv2d(F.interpolate(xi, scale_factor=2, mode="nearest"), w3, None, 1, 1) * g2).sum().backward()
    assert float((br.k4_to_w3_ref(slab)[0] - w3.grad).abs().max()) < 1e-11
    # group sum
    src = params.normal(37, 10, 3, 2, 2)
    out, mag, counts = br.group_sum_ref(src, (2, 0, 2, 1, 0), 4)
    assert counts == [2, 1, 2, 0] and float(out[6:8].abs().max()) == 0.0
    assert torch.equal(out[4:6], src[0:2].double() + src[4:6].double())
    # thin layers: stride-2 4x4 and 3x3 against the tap loop
    for ks, hi in ((3, 5), (4, 6)):
        inp, do = params.normal(38, 2, 3, hi, hi + 2), None
        ho, wo = ((hi, hi + 2) if ks == 3 else (hi // 2, (hi + 2) // 2))
        do = params.normal(39, 2, 4, ho, wo)
        ref = br.wgrad_thin_ref(inp, do, ks)
        loop = _wgrad_by_tap_loop(MODE_CONV3 if ks == 3 else MODE_CONV4S2, inp, do)     # [tap][c][ci]
        assert float((ref.permute(2, 3, 0, 1).reshape(loop.shape) - loop).abs().max()) < 1e-12


def test_ulp32_and_act_reference():
    t = torch.tensor([1.0, 1.5, 2.0, 0.75, 0.0, -3.0], dtype=torch.float64)
    assert br.ulp32(t).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24, 2.0 ** -149, 2.0 ** -22]
    y = torch.tensor([0.5, -0.25], dtype=torch.float32)
    dy = torch.tensor([2.0, 4.0], dtype=torch.float32)
    assert br.act_bwd_ref(dy, y, br.ACT_TANH).tolist() == [1.5, 3.75]
    assert br.act_bwd_ref(dy, y, br.ACT_SIGMOID).tolist() == [0.5, -1.25]
    assert br.act_bwd_ref(dy, y, br.ACT_LRELU, 0.5).tolist() == [2.0, 2.0]
    assert br.act_bwd_ref(dy, y, br.ACT_NONE).tolist() == [2.0, 4.0]


# ---- the edges the cases were chosen for ------------------------------------------------------------------------------------
def _tile_rule(mode, hg, wg, bf16x3):
    """wgrad_tile's documented rules on the iteration grid (Hg, Wg) - the output grid of MODE_CONV3 / MODE_CONV4S2, the input
    grid of MODE_CONVT4S2."""
    if mode == MODE_CONV4S2:
        if hg >= 4 and wg >= 8 and hg % 4 == 0 and wg % 8 == 0:
            return (1, 4, 8)
        return (2, 4, 4) if (hg, wg) == (4, 4) else None
    if not bf16x3 and hg % 8 == 0 and wg % 16 == 0:
        return (1, 8, 16)
    if hg % 8 == 0 and wg % 8 == 0:
        return (1, 8, 8)
    if mode == MODE_CONVT4S2 and (hg, wg) == (4, 4):
        return (4, 4, 4)
    return None


def _geometry(case, bf16x3):
    mode, n, h = case["mode"], case["n"], case["h"]
    hg = h // 2 if mode == MODE_CONV4S2 else h
    tile = _tile_rule(mode, hg, hg, bf16x3)
    ti, th, tw = tile
    tiles_item = -(-n // ti) * (hg // th) * (hg // tw)
    return tile, tiles_item, tiles_item * case["items"]


@pytest.mark.parametrize("name", br.CASE_NAMES)
def test_case_still_has_the_edge_it_was_chosen_for(name):
    case = br.CASE_BY_NAME[name]
    lib = _lib()
    bf16x3 = lib.dvg_mfma_mode() == 1
    tile, tiles_item, tiles = _geometry(case, bf16x3)
    s = lib.dvg_conv_wgrad_splits_multi(case["mode"], case["n"], case["h"], case["h"], case["c1"] + case["c2"], case["cout"],
                                        case["items"])
    assert s >= 1
    tps = -(-tiles // s)
    assert -(-tiles // tps) == s, "every split owns at least one tile"
    split_tail = tiles % tps != 0
    straddle = any((k * tps) // tiles_item != (min((k + 1) * tps, tiles) - 1) // tiles_item for k in range(s))
    print(f"{name}: tile {tile} tiles {tiles} ({tiles_item} per item) splits {s} x {tps} tail {split_tail} straddle {straddle}")
    if not bf16x3:
        return          # the comparison build tiles 8x16 where it can: the table below is the product build's
    assert tile == case["tile"]
    assert s == case["splits"]
    assert split_tail == case["split_tail"]
    assert straddle == case["straddle"]
    ti = tile[0]
    if "tail of" in case["why"]:
        assert case["n"] % ti == int(case["why"].split("tail of ")[1][0])
    if "single image" in case["why"]:
        assert case["n"] == 1 and ti > 1
    if "exact fit" in case["why"]:
        assert case["n"] == ti
    if "item boundary" in case["why"]:
        assert case["items"] > 1 and case["n"] % ti != 0
    if "crosses" in case["why"]:
        assert case["c1"] == 64 and case["c2"] >= 128       # ci tile 0 from x, tile 1 the first of several from skip


def test_the_case_list_is_the_issue_s():
    key = lambda c: (c["mode"], c["n"], c["h"], c["c1"], c["c2"], c["cout"], c["up"], c["items"])      # noqa: E731
    assert [key(c) for c in br.WGRAD_CASES] == [
        (0, 3, 8, 64, 0, 64, False, 1), (0, 2, 16, 64, 64, 64, True, 1), (0, 1, 8, 64, 192, 128, False, 1),
        (0, 9, 8, 512, 0, 512, False, 1), (0, 5, 8, 512, 0, 512, False, 3),
        (1, 3, 8, 64, 0, 128, False, 1), (1, 1, 8, 128, 0, 64, False, 1), (1, 2, 16, 64, 0, 64, False, 1),
        (1, 2, 32, 64, 0, 128, False, 2),
        (2, 5, 4, 128, 0, 64, False, 1), (2, 2, 4, 64, 64, 64, False, 1), (2, 1, 4, 64, 0, 64, False, 1),
        (2, 4, 4, 64, 0, 64, False, 1), (2, 3, 8, 64, 64, 128, False, 1), (2, 7, 4, 64, 0, 64, False, 3)]


# ---- the sizing calls and the dispatcher agree ----------------------------------------------------------------------------
def _dispatcher_kernels():
    """{mode: set of (TI, TH, TW)} read from the W_DISPATCH lines of dvg_conv_wgrad_multi."""
    src = open(os.path.join(ROOT, "dvg_amd", "csrc", "wgrad.hip")).read()
    body = src[src.index('extern "C" int dvg_conv_wgrad_multi(int mode, int items, const float* const* xs'):]
    names = {"W_CONV3": MODE_CONV3, "W_CONV4S2": MODE_CONV4S2, "W_CONVT4S2": MODE_CONVT4S2}
    out = {m: set() for m in names.values()}
    for m, ti, th, tw in re.findall(r"W_DISPATCH\((W_\w+), (\d+), (\d+), (\d+)\)", body):
        out[names[m]].add((int(ti), int(th), int(tw)))
    assert all(out.values())
    return out


@pytest.mark.parametrize("mode", [MODE_CONV3, MODE_CONV4S2, MODE_CONVT4S2])
def test_splits_answer_minus_one_exactly_where_the_dispatcher_has_no_kernel(mode):
    """dvg_conv_wgrad_splits* sizes the partial buffer of a launch: a positive answer for a (mode, map) that
    dvg_conv_wgrad_multi then refuses ("no kernel for tile") is a contradiction - (4,4,4) was offered to MODE_CONV3."""
    lib = _lib()
    bf16x3 = lib.dvg_mfma_mode() == 1
    kernels = _dispatcher_kernels()[mode]
    seen = set()
    for side in (2, 4, 8, 12, 16, 32):           # side of the iteration grid
        h = 2 * side if mode == MODE_CONV4S2 else side       # the forward INPUT grid the calls take
        tile = _tile_rule(mode, side, side, bf16x3)
        has_kernel = tile is not None and tile in kernels
        assert tile is None or tile in kernels, (mode, side, tile)      # the tile rule offers nothing the dispatcher lacks
        for items in (1, 3):
            s = lib.dvg_conv_wgrad_splits_multi(mode, 3, h, h, 128, 64, items)
            assert (s >= 1) if has_kernel else (s == -1), (mode, side, items, s, tile)
        s1 = lib.dvg_conv_wgrad_splits(mode, 3, h, h, 128, 64)
        assert s1 == lib.dvg_conv_wgrad_splits_multi(mode, 3, h, h, 128, 64, 1)
        seen.add(has_kernel)
    assert seen == {True, False}
    if mode == MODE_CONV3:
        assert lib.dvg_conv_wgrad_splits(mode, 4, 4, 4, 64, 64) == -1
    # channel counts and item counts the kernels do not take
    h = 16
    assert lib.dvg_conv_wgrad_splits_multi(mode, 3, h, h, 96, 64, 1) == -1
    assert lib.dvg_conv_wgrad_splits_multi(mode, 3, h, h, 64, 64, 9) == -1
