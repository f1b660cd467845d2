"""CPU-only checks of tests/forward_ref.py, for every case tests/test_gpu_forward_igemm.py runs on the device: each case still
has the tile and the K split it was chosen for under both tile policies (dvg_conv_splitk_v2 / dvg_conv_stats_rows_v2 are
host-only code), the fp32 yardsticks pass the bar and every planted defect fails it, the bar is not vacuous, tilewise_err
measures what it says, the reference's layout is right (against an explicit loop over taps that shares no code with it), and the
emulation of the kernel's summation order computes the same convolution."""
import pytest
import torch

from oracle import params
from tests import forward_ref as fr
from tests.backward_ref import MODE_CONV3, MODE_CONV4S2, MODE_CONVT4S2, YARDSTICK_RATIO
from tests.forward_ref import ENERGY, LATENCY


def _lib():
    from dvg_amd._lib import lib
    return lib()


# ---- the dispatch of every case ---------------------------------------------------------------------------------------------
def _geometry(case, policy):
    """(tile, workgroups per split, tiles, splits the launch runs, chunks per split) from the rules restated in forward_ref.plan."""
    g = fr.plan(case["mode"], case["n"], case["h"], case["w"], case["c1"] + case["c2"], case["cout"], policy)
    return g["tile"], g["wgs"], g["tiles"], g["splits"], g["cps"]


@pytest.mark.parametrize("name", fr.CASE_NAMES)
def test_case_still_has_the_tile_and_the_split_it_was_chosen_for(name):
    from dvg_amd import ops
    case, lib = fr.CASE_BY_NAME[name], _lib()
    mode, n, h, w, cin, cout = case["mode"], case["n"], case["h"], case["w"], case["c1"] + case["c2"], case["cout"]
    before = lib.dvg_tile_policy()
    for policy in (LATENCY, ENERGY):
        tile, wgs, tiles, s, cps = _geometry(case, policy)
        with ops.tile_policy(policy == ENERGY):
            s_lib = lib.dvg_conv_splitk_v2(mode, n, h, w, cin, cout)
            rows = lib.dvg_conv_stats_rows_v2(mode, n, h, w, cin, cout, int(case["pool"]), 0)
        print(f"{name} policy {policy}: tile {tile} workgroups {wgs} tiles {tiles} splits {s_lib} x {cps} chunks")
        assert tile == case["tile"][policy]
        assert s_lib == s == case["splits"][policy]          # the count the launch runs: no empty split
        assert len(fr.split_chunks(cin // 16, s_lib)) == s_lib
        assert rows == tiles
    assert lib.dvg_tile_policy() == before
    # the edge named in `why`
    why, ti = case["why"], case["tile"][LATENCY][0]
    sizes = [b - a for a, b in fr.split_chunks(cin // 16, case["splits"][LATENCY])]
    if "splits of" in why:
        assert sizes == [int(v) for v in why.split("splits of ")[1].split(";")[0].split(" straddling")[0].split(" / ")]
    if "tail of" in why:
        assert case["n"] % ti == int(why.split("tail of ")[1][0])
    if "one image in" in why:
        assert case["n"] == 1 and ti == 4
    if "exact fit" in why:
        assert case["n"] == ti == 4
    if "one chunk" in why:
        assert cin == 16
    if "straddling" in why or "split 0 holds" in why:
        lo, hi = fr.split_chunks(cin // 16, case["splits"][LATENCY])[0]
        assert 16 * lo < case["c1"] < 16 * hi
    if "spans two groups" in why:
        assert case["addend"][0] < ti
    if "finish kernel" in why:
        assert case["splits"][LATENCY] > 1
    if "main kernel" in why:
        assert case["splits"][LATENCY] == 1


def test_the_case_list_is_the_issue_s():
    key = lambda c: (c["mode"], c["n"], c["h"], c["w"], c["c1"], c["c2"], c["cout"], c["up"], c["pool"], c["addend"])   # noqa: E731
    add = (2, (0, 1, 0))
    assert [key(c) for c in fr.FWD_CASES] == [
        (0, 1, 8, 8, 16, 0, 64, False, False, None), (0, 2, 8, 16, 48, 0, 64, False, True, None),
        (0, 1, 8, 8, 16, 16, 64, True, False, None), (0, 2, 8, 8, 208, 0, 64, False, True, None),
        (0, 1, 16, 16, 48, 96, 128, True, False, None), (0, 16, 32, 32, 32, 0, 128, False, True, None),
        (0, 6, 8, 8, 32, 0, 64, False, False, add), (0, 6, 8, 8, 128, 0, 64, False, False, add),
        (1, 1, 16, 16, 16, 0, 64, False, False, None), (1, 1, 8, 8, 32, 0, 64, False, False, None),
        (1, 4, 8, 8, 32, 0, 64, False, False, None), (1, 5, 8, 8, 32, 0, 64, False, False, None),
        (1, 3, 8, 8, 144, 0, 64, False, False, None), (1, 1, 16, 48, 16, 0, 64, False, False, None),
        (1, 3, 16, 16, 64, 0, 64, False, False, None), (1, 32, 32, 32, 16, 0, 256, False, False, None),
        (2, 1, 8, 8, 16, 0, 64, False, False, None), (2, 5, 4, 4, 16, 16, 64, False, False, None),
        (2, 3, 4, 4, 48, 96, 64, False, False, None), (2, 6, 4, 4, 32, 0, 64, False, False, add),
        (2, 2, 8, 8, 256, 0, 64, False, False, None), (2, 16, 16, 16, 16, 0, 128, False, False, None),
        (0, 1, 8, 8, 400, 0, 64, False, False, None), (0, 1, 8, 8, 528, 0, 64, False, False, None),
        (1, 1, 16, 16, 400, 0, 64, False, False, None), (2, 1, 4, 4, 400, 0, 64, False, False, None)]
    assert [n for n, p in fr.VARIANTS if p == ENERGY] == [
        "conv3-n16-32x32-c32+0-o128-pool", "conv4s2-n32-32x32-c16+0-o256", "convT4s2-n16-16x16-c16+0-o128"]
    assert all(fr.CASE_BY_NAME[n]["tile"][ENERGY] == (1, 8, 16) for n, p in fr.VARIANTS if p == ENERGY)


# ---- the bar ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,policy", fr.VARIANTS, ids=fr.VARIANT_IDS)
def test_yardsticks_pass_and_the_bar_is_not_vacuous(name, policy):
    """torch's fp32 result and the mode's yardstick are within the bar, and max(1.5 e_y, worst e_y of the mode) <= 0.5 e_plane:
    the cap never bites, so the bar is set by the yardstick AND rejects a lost bf16 plane of either operand."""
    f, mode = fr.case_figures(name, policy), fr.CASE_BY_NAME[name]["mode"]
    worst, b = fr.mode_worst(mode), fr.case_bar(name, policy)
    print(f"{name} policy {policy} yardstick {fr.YARDSTICK[mode]}: e32 {f['e32']:.2e} e_ord {f['e_ord']:.2e} e_mfma "
          f"{f['e_mfma']:.2e} worst-of-mode {worst:.2e} e_plane w {f['e_plane_w']:.2e} x {f['e_plane_x']:.2e} bar {b:.2e}")
    assert f["e32"] <= b and f["e_y"] <= b
    assert max(YARDSTICK_RATIO * f["e_y"], worst) <= 0.5 * f["e_plane"], (f["e_y"], worst, f["e_plane"])
    assert b == max(YARDSTICK_RATIO * f["e_y"], worst)
    assert min(f["e_plane_w"], f["e_plane_x"]) > b


@pytest.mark.parametrize("name,policy", fr.VARIANTS, ids=fr.VARIANT_IDS)
def test_every_planted_defect_fails_the_bar(name, policy):
    case = fr.CASE_BY_NAME[name]
    args, b, ti = fr.case_args(case), fr.case_bar(name, policy), case["tile"][policy][0]
    applies = {"seam": case["c2"] > 0, "tail": case["n"] % ti != 0,
               "addend_tile": case["addend"] is not None and case["addend"][0] < ti}
    for kind in fr.PLANTS:
        if not applies.get(kind, True):
            with pytest.raises(ValueError):
                fr.plant(kind, *args, ti=ti)
            continue
        if kind in ("plane_w", "plane_x"):
            e = fr.case_figures(name, policy)["e_" + kind]
        else:
            e = fr.case_err(name, policy, fr.plant(kind, *args, ti=ti))
        print(f"{name} policy {policy}: planted {kind}: {e:.2e} (bar {b:.2e})")
        assert e > b, (kind, e, b)


def test_every_kind_of_defect_applies_to_some_case():
    ti = lambda c: c["tile"][LATENCY][0]                                                # noqa: E731
    assert any(c["c2"] for c in fr.FWD_CASES)                                           # "seam"
    assert any(c["n"] % ti(c) for c in fr.FWD_CASES)                                    # "tail"
    assert any(c["addend"] and c["addend"][0] < ti(c) for c in fr.FWD_CASES)            # "addend_tile"
    with pytest.raises(ValueError):
        fr.plant("no such defect", *fr.case_args(fr.FWD_CASES[0]))


# ---- tilewise_err itself ---------------------------------------------------------------------------------------------------
def test_tilewise_err_is_not_diluted_and_pads_the_image_tail():
    from tests.common import rel_err
    ref = torch.ones(5, 128, 16, 16, dtype=torch.float64)
    ref[0, :64, :8, :8] *= 1000.0                        # one loud tile
    a = ref.clone()
    a[3, 70, 9, 12] += 0.01                              # a 1 % error in a quiet tile
    assert abs(fr.tilewise_err(a, ref, 1, 8, 8) - 0.01) < 1e-12
    assert abs(fr.tilewise_err(a, ref, 1, 8, 16) - 0.01) < 1e-12
    assert rel_err(a, ref) < 2e-5                        # the tensor-wide figure does not see it
    # an error in the loud tile's run of images is measured against the loud magnitude ...
    assert abs(fr.tilewise_err(a, ref, 4, 8, 8) - 0.01) < 1e-12           # image 3, channel block 1: still quiet
    a2 = ref.clone()
    a2[3, 5, 1, 1] += 1.0
    assert abs(fr.tilewise_err(a2, ref, 1, 8, 8) - 1.0) < 1e-12 and abs(fr.tilewise_err(a2, ref, 4, 8, 8) - 1e-3) < 1e-12
    # ... and the image tail (image 4 alone in the second run of four) against its own
    a3 = ref.clone()
    a3[4, 5, 1, 1] += 0.5
    assert abs(fr.tilewise_err(a3, ref, 4, 8, 8) - 0.5) < 1e-12
    # parity blocks of the transposed conv: a loud parity does not hide a quiet one's error
    r4 = torch.ones(1, 64, 16, 16, dtype=torch.float64)
    r4[:, :, 0::2, 0::2] *= 1000.0
    a4 = r4.clone()
    a4[0, 3, 5, 2] += 0.01                               # parity (1, 0)
    assert abs(fr.tilewise_err(a4, r4, 1, 8, 8, parity=True) - 0.01) < 1e-12
    assert fr.tilewise_err(a4, r4, 1, 8, 8) < 2e-5
    a4[0, 0, 0, 0] = float("nan")
    assert fr.tilewise_err(a4, r4, 1, 8, 8, parity=True) == float("inf")
    a[1, 2, 3, 4] = float("inf")
    assert fr.tilewise_err(a, ref, 4, 8, 8) == float("inf")
    # fewer than 64 channels
    r5 = torch.arange(1, 1 + 2 * 3 * 4 * 4, dtype=torch.float64).reshape(2, 3, 4, 4)
    a5 = r5.clone()
    a5[1, 2, 3, 3] *= 1.5
    assert abs(fr.tilewise_err(a5, r5, 4, 4, 4) - 0.5) < 1e-12


# ---- the reference's layout, independently ---------------------------------------------------------------------------------
def _forward_by_tap_loop(mode, inp, w):
    """The convolution by an explicit loop over taps and pixels, from the index formulas (fp64):
      conv3:    out[co][y][x] += W[co][ci][a][b] in[ci][y + a - 1][x + b - 1]
      conv4s2:  out[co][y][x] += W[co][ci][a][b] in[ci][2 y + a - 1][2 x + b - 1]
      convT4s2: out[co][2 i - 1 + k][2 j - 1 + l] += W[ci][co][k][l] in[ci][i][j]"""
    inp, w = inp.double(), w.double()
    n, cin, h, wd = inp.shape
    if mode == MODE_CONVT4S2:
        out = torch.zeros(n, w.shape[1], 2 * h, 2 * wd, dtype=torch.float64)
        for i in range(h):
            for j in range(wd):
                for k in range(4):
                    for l in range(4):
                        oy, ox = 2 * i - 1 + k, 2 * j - 1 + l
                        if 0 <= oy < 2 * h and 0 <= ox < 2 * wd:
                            out[:, :, oy, ox] += inp[:, :, i, j] @ w[:, :, k, l]
        return out
    s, ks = (2, 4) if mode == MODE_CONV4S2 else (1, 3)
    out = torch.zeros(n, w.shape[0], h // s, wd // s, dtype=torch.float64)
    for y in range(h // s):
        for x in range(wd // s):
            for a in range(ks):
                for b in range(ks):
                    iy, ix = s * y + a - 1, s * x + b - 1
                    if 0 <= iy < h and 0 <= ix < wd:
                        out[:, :, y, x] += inp[:, :, iy, ix] @ w[:, :, a, b].t()
    return out


@pytest.mark.parametrize("mode", [MODE_CONV3, MODE_CONV4S2, MODE_CONVT4S2])
@pytest.mark.parametrize("concat_up", [False, True])
def test_reference_layout_against_an_explicit_tap_loop(mode, concat_up):
    """2 images, a 4 x 4 map, 4 (+ 4) channels, 6 outputs; the concat forms with an addend shared in blocks of one image."""
    up = concat_up and mode == MODE_CONV3
    x = params.normal(41, 2, 4, 2 if up else 4, 2 if up else 4)
    skip = params.normal(42, 2, 4, 4, 4) if concat_up else None
    w = params.normal(43, *fr.weight_shape(mode, 8 if concat_up else 4, 6))
    ho = {MODE_CONV3: 4, MODE_CONV4S2: 2, MODE_CONVT4S2: 8}[mode]
    addend = (params.normal(44, 2, 6, ho, ho), 1, (1, 0)) if concat_up else None
    ref = fr.forward_ref(mode, x, skip, w, up, addend)
    xin = x.repeat_interleave(2, 2).repeat_interleave(2, 3) if up else x
    loop = _forward_by_tap_loop(mode, xin if skip is None else torch.cat([xin, skip], 1), w)
    if addend is not None:
        loop = loop + addend[0][[1, 0]].double()
    assert ref.shape == loop.shape == (2, 6, ho, ho)
    assert float((ref - loop).abs().max()) <= 1e-12 * float(loop.abs().max())


# ---- the emulation of the kernel's order -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["conv3-n1-16x16-c48+96-o128-up", "conv3-n6-8x8-c128+0-o64-add", "conv4s2-n3-8x8-c144+0-o64",
                                  "convT4s2-n3-4x4-c48+96-o64", "convT4s2-n6-4x4-c32+0-o64-add"])
def test_ordered_emulation_is_the_same_convolution(name):
    """ordered_fp32_ref walks chunks, taps, parities and splits in the kernel's order; it must still BE the convolution: both
    grains agree with fp64 at fp32 noise level (far below any planted defect), the partial sums of the splits add up to the
    unsplit sum, and the bf16 planes it multiplies are an exact split."""
    case = fr.CASE_BY_NAME[name]
    args, ref = fr.case_args(case), fr.case_ref(name)["ref"]
    s = case["splits"][LATENCY]
    for per_mfma in (False, True):
        tot, parts = fr.ordered_fp32_ref(*args, splits=s, per_mfma=per_mfma)
        assert len(parts) == s
        assert fr.case_err(name, LATENCY, tot) < 2e-6
        one, _ = fr.ordered_fp32_ref(*args, splits=1, per_mfma=per_mfma)
        assert fr.case_err(name, LATENCY, one) < 2e-6
        a = fr.addend_images(args[5], case["n"])
        total = sum(p.double() for p in parts) + (0 if a is None else a.double())
        assert fr.case_err(name, LATENCY, total) < 2e-6
    t = params.normal(45, 4096)
    h, m, l = fr.bf16_planes(t)
    assert torch.equal(h + m + l, t.double())
    for p in (h, m, l):
        assert torch.equal(p.float().bfloat16().double(), p)
