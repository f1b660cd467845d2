"""Host side of dvg_amd/csrc/conv_igemm2.hip, without a GPU.  (1) The return code of every entry point for a bad argument, and
that dvg_last_error() names the entry point that was called: fake pointers (16: aligned, 8: misaligned), never dereferenced -
every check returns before anything is launched (the pattern of tests/test_winograd_launchers_host.py).  The codes are NOT
symmetric across entry points and the table pins them as they are (docs/DESIGN_NOTES_igemm_launchers.md).  (2) The launch plan:
dvg_conv_splitk_v2 and dvg_conv_stats_rows_v2 against the rules restated in tests/forward_ref.py, swept under both tile
policies."""
import itertools

import pytest

from tests import forward_ref as fr

SHAPE, NULL, ALIGN = 1, 2, 4      # DVG_ERR_SHAPE, DVG_ERR_NULL, DVG_ERR_ALIGN (include/dvg_hip.h)
A, M = 16, 8                      # fake pointers: aligned, misaligned

# entry point -> (argument names, a call in which every argument is valid); a case replaces arguments by name
_PAIR = "frame w0 scale0 shift0 w1 scale1 shift1 y y_pool N H W Cout act slope y_from stream"
BASE = {
    "dvg_conv3x3_bn_act_v2": ("x skip w scale shift y y_pool stats N H W C1 C2 Cout up act slope ws ws_floats addend map block stream",
                              (A, None, A, None, None, A, None, None, 4, 8, 8, 64, 0, 64, 0, 1, 0.2, None, 0, None, None, 0, None)),
    "dvg_convT4x4s2_bn_act_v2": ("x skip w scale shift y stats N H W C1 C2 Cout act slope ws ws_floats addend map block stream",
                                 (A, None, A, None, None, A, None, 4, 8, 8, 64, 0, 64, 1, 0.2, None, 0, None, None, 0, None)),
    "dvg_conv4x4s2_bn_act_v2": ("x w scale shift y stats N H W Cin Cout act slope ws ws_floats stream",
                                (A, A, None, None, A, None, 4, 16, 16, 64, 64, 1, 0.2, None, 0, None)),
    "dvg_conv3x3_first_pair": (_PAIR, (A, A, A, A, A, None, None, A, None, 32, 64, 64, 64, 1, 0.2, 0, None)),
    "dvg_conv3x3_first_pair_wx": (_PAIR, (A, A, A, A, A, None, None, A, None, 32, 64, 64, 64, 1, 0.2, 0, None)),
    "dvg_conv3x3_bn_act_wx": ("x skip w scale shift y y_pool N H W C1 C2 Cout up act slope addend map block stream",
                              (A, None, A, None, None, A, None, 4, 8, 16, 64, 0, 64, 0, 1, 0.2, None, None, 0, None)),
    "dvg_convT4x4s2_bn_act_proj": ("x w scale shift proj_w proj_out T N H W C1 Cout act slope addend map block stream",
                                   (A, A, None, None, A, A, 16, 4, 8, 8, 64, 64, 1, 0.2, None, None, 0, None)),
    "dvg_gemm_batched_k16": ("x w y NB H W Cin Cout stream", (A, A, A, 16, 8, 8, 64, 64, None)),
    "dvg_gemm_batched_k16_as": ("x w y NB NB_as H W Cin Cout stream", (A, A, A, 25, 36, 8, 8, 64, 64, None)),
    "dvg_pack_conv_weight_k16": ("w w_packed cout cin kh kw transposed stream", (A, A, 64, 16, 3, 3, 0, None)),
    "dvg_pack_conv_weight_wx": ("w w_packed cout cin stream", (A, A, 64, 16, None)),
}
BAD = {
    "dvg_conv3x3_bn_act_v2": [
        ("NULL x", dict(x=None), NULL), ("skip with C2 = 0", dict(skip=A), SHAPE), ("C1 = 40", dict(C1=40), SHAPE),
        ("Cout = 96", dict(Cout=96), SHAPE), ("misaligned y", dict(y=M), ALIGN), ("act = 4", dict(act=4), SHAPE),
        ("misaligned addend", dict(addend=M), SHAPE), ("addend with y_pool", dict(addend=A, y_pool=A), SHAPE),
        ("addend + map with block 3", dict(addend=A, map=A, block=3), SHAPE), ("12x12 map", dict(H=12, W=12), SHAPE)],
    "dvg_convT4x4s2_bn_act_v2": [
        ("NULL w", dict(w=None), NULL), ("misaligned addend", dict(addend=M), ALIGN), ("12x12 map", dict(H=12, W=12), SHAPE),
        ("addend + map with block 3", dict(addend=A, map=A, block=3), SHAPE)],
    "dvg_conv4x4s2_bn_act_v2": [
        ("H = 9", dict(H=9), SHAPE), ("N = 40000 at 128x128", dict(N=40000, H=128, W=128), SHAPE),
        ("24x24 map", dict(H=24, W=24), SHAPE), ("misaligned x", dict(x=M), ALIGN)],
    "dvg_conv3x3_first_pair": [
        ("NULL scale0", dict(scale0=None), NULL), ("y_from = 2 without y_pool", dict(y_from=2), SHAPE),
        ("NULL y with y_from 0", dict(y=None), SHAPE), ("NULL w1", dict(w1=None), NULL), ("W = 8", dict(W=8), SHAPE),
        ("N = 1: 32 workgroups", dict(N=1), SHAPE), ("misaligned w1", dict(w1=M), ALIGN)],
    "dvg_conv3x3_first_pair_wx": [
        ("NULL w1", dict(w1=None), NULL), ("misaligned w0", dict(w0=M), ALIGN), ("y_from = 2 without y_pool", dict(y_from=2), SHAPE),
        ("W = 8", dict(W=8), SHAPE)],
    "dvg_conv3x3_bn_act_wx": [
        ("NULL y", dict(y=None), NULL), ("skip with C2 = 16", dict(skip=A, C2=16), SHAPE), ("upsample", dict(up=1), SHAPE),
        ("addend with y_pool", dict(addend=A, y_pool=A), SHAPE), ("misaligned addend", dict(addend=M), ALIGN),
        ("W = 8", dict(W=8), SHAPE)],
    "dvg_convT4x4s2_bn_act_proj": [
        ("NULL proj_out", dict(proj_out=None), NULL), ("Cout = 128", dict(Cout=128), SHAPE), ("T = 49", dict(T=49), SHAPE),
        ("misaligned proj_w", dict(proj_w=M), ALIGN), ("4x4 map", dict(H=4, W=4), SHAPE),
        ("addend + map with block 3", dict(addend=A, map=A, block=3), SHAPE)],
    "dvg_gemm_batched_k16": [("NULL y", dict(y=None), NULL), ("Cin = 48", dict(Cin=48), SHAPE), ("W = 12", dict(W=12), SHAPE)],
    "dvg_gemm_batched_k16_as": [("NB 36 as 25", dict(NB=36, NB_as=25), SHAPE), ("Cin = 48", dict(Cin=48), SHAPE)],
    "dvg_pack_conv_weight_k16": [("NULL w", dict(w=None), NULL), ("cin = 24", dict(cin=24), SHAPE)],
    "dvg_pack_conv_weight_wx": [("misaligned w_packed", dict(w_packed=M), ALIGN), ("cout = 32", dict(cout=32), SHAPE)],
}
CASES = [(entry, what, bad, code) for entry, rows in BAD.items() for what, bad, code in rows]
# the _as entry shares the dense one's body, which reports under the dense name: either is accepted there
NAMES = {"dvg_gemm_batched_k16_as": ("dvg_gemm_batched_k16_as", "dvg_gemm_batched_k16")}


def test_the_table_has_the_fifty_calls():
    assert len(CASES) == 50 and set(BAD) == set(BASE)


@pytest.mark.parametrize("entry,what,bad,code", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_bad_argument_gives_its_code_and_names_the_entry_point(entry, what, bad, code):
    from dvg_amd import _lib
    lib = _lib.lib()
    names, base = BASE[entry][0].split(), BASE[entry][1]
    assert len(names) == len(base) == len(_lib.SIGNATURES[entry][1]) and set(bad) <= set(names)
    rc = getattr(lib, entry)(*[bad.get(n, v) for n, v in zip(names, base)])
    msg = lib.dvg_last_error().decode()
    assert rc == code, (entry, what, rc, msg)
    assert msg.split(":")[0].split(" ")[0] in NAMES.get(entry, (entry,)), (entry, what, msg)


# ---- the plan, swept -------------------------------------------------------------------------------------------------------
GRIDS = [(4, 4), (8, 8), (8, 16), (16, 16), (16, 48), (32, 32), (64, 64)]       # the grid the tiles cover
SWEEP = list(itertools.product((0, 1, 2), (1, 3, 4, 5, 7, 10, 16, 64), GRIDS, (16, 64, 128, 144, 208, 400, 512, 528, 576),
                               (64, 128, 256, 512)))


def sweep_mismatches(lib, set_policy):
    """[(policy, mode, n, h, w, cin, cout, what, library's answer, restated answer)] over SWEEP under both tile policies."""
    out = []
    for policy in (fr.LATENCY, fr.ENERGY):
        set_policy(policy)
        for mode, n, (gh, gw), cin, cout in SWEEP:
            h, w = (2 * gh, 2 * gw) if mode == fr.MODE_CONV4S2 else (gh, gw)
            got = {("splits", 0, 1): lib.dvg_conv_splitk_v2(mode, n, h, w, cin, cout)}
            for pool, ws in itertools.product((0, 1) if mode == fr.MODE_CONV3 else (0,), (0, 1)):
                got[("rows", pool, ws)] = lib.dvg_conv_stats_rows_v2(mode, n, h, w, cin, cout, pool, ws)
            for (what, pool, ws), v in got.items():
                want = fr.plan(mode, n, h, w, cin, cout, policy, pool=bool(pool), with_ws=bool(ws))[what]
                if v != want:
                    out.append((policy, mode, n, h, w, cin, cout, f"{what} pool {pool} ws {ws}", v, want))
    return out


def test_split_count_and_statistics_rows_follow_the_restated_plan():
    from dvg_amd import _lib
    lib = _lib.lib()
    before = lib.dvg_tile_policy()
    try:
        bad = sweep_mismatches(lib, lib.dvg_set_tile_policy)
    finally:
        lib.dvg_set_tile_policy(before)
    assert lib.dvg_tile_policy() == before
    assert not bad, (len(bad), bad[:10])
