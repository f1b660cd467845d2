"""Host side of the F(4x4,3x3) launchers in dvg_amd/csrc/winograd.hip, without a GPU: the return code of every entry point
for a bad argument, and that dvg_last_error() names the entry point that was called.  The pointers are fakes (16: aligned,
8: misaligned) and never dereferenced: every check below returns before anything is launched (the pattern of
tests/test_abi.py::test_host_side_checks_reject_bad_shapes_without_gpu).  The dense / live pairs are NOT symmetric in their
codes - a misaligned addend is a shape error to dvg_winograd_output and an alignment error to dvg_winograd_output_live - and
the table pins them as they are (docs/DESIGN_NOTES_winograd_launchers.md)."""
import pytest

SHAPE, NULL, ALIGN = 1, 2, 4      # DVG_ERR_SHAPE, DVG_ERR_NULL, DVG_ERR_ALIGN (include/dvg_hip.h)
A, M = 16, 8                      # fake pointers: aligned, misaligned


def _out_in(name):
    # (mm, scale, shift, v_next, N, H, W, C, act, slope, addend, stream)
    return [
        (name, "NULL mm", (None, None, None, A, 4, 16, 16, 64, 1, 0.2, None, None), NULL),
        (name, "12x12 map", (A, None, None, A, 4, 12, 12, 64, 1, 0.2, None, None), SHAPE),
        (name, "C = 48", (A, None, None, A, 4, 16, 16, 48, 1, 0.2, None, None), SHAPE),
        (name, "act = 4", (A, None, None, A, 4, 16, 16, 64, 4, 0.2, None, None), SHAPE),
        (name, "misaligned mm", (M, None, None, A, 4, 16, 16, 64, 1, 0.2, None, None), ALIGN),
        (name, "misaligned addend", (A, None, None, A, 4, 16, 16, 64, 1, 0.2, M, None), ALIGN),
    ]


def _out_up_in(name):
    # (mm, scale, shift, v_next, N, H, W, C, act, slope, stream)
    return [
        (name, "NULL v_next", (A, None, None, None, 4, 8, 8, 64, 1, 0.2, None), NULL),
        (name, "32x32 map", (A, None, None, A, 4, 32, 32, 64, 1, 0.2, None), SHAPE),
        (name, "misaligned v_next", (A, None, None, M, 4, 8, 8, 64, 1, 0.2, None), ALIGN),
    ]


def _stem(name):
    # (vec, ldv, w_kn, KP, scale, shift, v_next, M, C, K, act, slope, stream)
    return [
        (name, "NULL v_next", (A, 90, A, 96, None, None, None, 4, 64, 90, 1, 0.2, None), NULL),
        (name, "KP = 100", (A, 90, A, 100, None, None, A, 4, 64, 90, 1, 0.2, None), SHAPE),
        (name, "C = 40", (A, 90, A, 96, None, None, A, 4, 40, 90, 1, 0.2, None), SHAPE),
    ]


CASES = (
    _out_in("dvg_winograd_output_input") + _out_in("dvg_winograd_output_input_live")
    + _out_up_in("dvg_winograd_output_up_input") + _out_up_in("dvg_winograd_output_up_input_live")
    + _stem("dvg_stem_up_winograd_input") + _stem("dvg_stem_up_winograd_input_live")
    + [
        # (x, v, N, H, W, C, m, upsample, stream)
        ("dvg_winograd_input", "C = 62", (A, A, 4, 8, 8, 62, 4, 1, None), SHAPE),
        ("dvg_winograd_input", "6x6 map", (A, A, 4, 6, 6, 64, 4, 1, None), SHAPE),
        # (x, v, N, H, W, C, stream)
        ("dvg_winograd_input_up_live", "C = 62", (A, A, 4, 8, 8, 62, None), SHAPE),
        ("dvg_winograd_input_up_live", "6x6 map", (A, A, 4, 6, 6, 64, None), SHAPE),
        ("dvg_winograd_input_up_live", "misaligned v", (A, M, 4, 8, 8, 64, None), ALIGN),
        # (m, scale, shift, y, y_pool, N, H, W, C, act, slope, mt, addend, y_from, stream)
        ("dvg_winograd_output", "C = 62", (A, None, None, A, None, 4, 8, 8, 62, 1, 0.2, 4, None, 0, None), SHAPE),
        ("dvg_winograd_output", "misaligned addend", (A, None, None, A, None, 4, 8, 8, 64, 1, 0.2, 4, M, 0, None), SHAPE),
        # (m, scale, shift, y, N, H, W, C, act, slope, addend, stream)
        ("dvg_winograd_output_live", "C = 62", (A, None, None, A, 4, 8, 8, 62, 1, 0.2, None, None), SHAPE),
        ("dvg_winograd_output_live", "misaligned addend", (A, None, None, A, 4, 8, 8, 64, 1, 0.2, M, None), ALIGN),
        # (mm, scale, shift, y, v_next, N, H, W, C, act, slope, y_from, stream)
        ("dvg_winograd_output_pool_input", "8x8 map", (A, None, None, A, A, 4, 8, 8, 64, 1, 0.2, 0, None), SHAPE),
        ("dvg_winograd_output_pool_input", "NULL y, y_from < N", (A, None, None, None, A, 4, 16, 16, 64, 1, 0.2, 2, None), NULL),
        # (x, dy, v, dm, N, H, W, Cin, Cout, t_total, t_off, stream): 16 tiles into a buffer of 10
        ("dvg_winograd_wgrad_operands", "16 tiles, buffer of 10", (A, A, A, A, 1, 16, 16, 64, 64, 10, 0, None), SHAPE),
    ])

# the live stem entry shares the dense one's body and reports under the dense name: either is accepted there
NAMES = {"dvg_stem_up_winograd_input_live": ("dvg_stem_up_winograd_input_live", "dvg_stem_up_winograd_input")}


@pytest.mark.parametrize("entry,what,args,code", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_bad_argument_gives_its_code_and_names_the_entry_point(entry, what, args, code):
    from dvg_amd import _lib
    lib = _lib.lib()
    assert len(args) == len(_lib.SIGNATURES[entry][1])
    rc = getattr(lib, entry)(*args)
    msg = lib.dvg_last_error().decode()
    assert rc == code, (entry, what, rc, msg)
    called = msg.split(":")[0].split(" ")[0]
    assert called in NAMES.get(entry, (entry,)), (entry, what, msg)


def test_transform_width_follows_the_1024_workgroup_rule():
    """dvg_winograd_transform_width: the widest form (4, 2, 1 channels per thread) with >= 1024 workgroups of 256 threads."""
    from dvg_amd import _lib
    lib = _lib.lib()
    assert [lib.dvg_winograd_transform_width(t, 64) for t in (16384, 8192, 2048)] == [4, 2, 1]
    assert lib.dvg_winograd_transform_width(16384, 62) == 0
