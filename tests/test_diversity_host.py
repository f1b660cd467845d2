"""CPU: the sample-diversity feature's host side - the entry point is exported and bound as the header declares it, the command
lines accept --diversity, and the fp64 reference the GPU tests compare against (tests/diversity_ref.py) gives hand-computed
numbers."""
import ctypes
import os

import numpy as np

from tests import diversity_ref as ref
from tests.common import header_declaration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_entry_point_and_the_header_agrees_with_the_binding():
    from dvg_amd import _lib
    for name in ("libdvg_hip.so", "libdvg_hip_f32mfma.so"):
        h = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), name))
        assert hasattr(h, "dvg_pairwise_frame_mse"), name
    ret, params = header_declaration("dvg_pairwise_frame_mse")     # tests/test_abi.py holds every declaration's binding
    assert ret == "int" and _lib.SIGNATURES["dvg_pairwise_frame_mse"][0] is ctypes.c_int and len(params) == 8
    assert _lib.lib().dvg_abi_version() == 9


def test_argument_checks_fire_before_any_launch():
    from dvg_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(16)               # never dereferenced: every call fails in the checks
    assert lib.dvg_pairwise_frame_mse(None, one, 2, 16, 1, 16, 16, None) == 2
    assert lib.dvg_pairwise_frame_mse(one, None, 2, 16, 1, 16, 16, None) == 2
    for s, ss, f, fs, d in ((0, 16, 1, 16, 16), (2, 16, 0, 16, 16), (2, 16, 1, 16, 0), (2, 8, 1, 16, 16), (2, 16, 1, 8, 16)):
        assert lib.dvg_pairwise_frame_mse(one, one, s, ss, f, fs, d, None) == 1, (s, ss, f, fs, d)
    assert b"dvg_pairwise_frame_mse" in lib.dvg_last_error()


def test_command_lines_accept_the_flag():
    import importlib.util
    import generate_frames
    p = generate_frames.build_parser()
    assert p.parse_args(["--diversity"]).diversity is True and p.parse_args([]).diversity is False
    spec = importlib.util.spec_from_file_location("bench_make_gifs", os.path.join(ROOT, "tools", "bench_make_gifs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.build_parser().parse_args(["--diversity"]).diversity is True
    import utils
    assert callable(utils.sample_diversity)


def test_reference_on_hand_computed_cases():
    # two samples, one frame of four pixels: differences (1, 0, -2, 0.5) -> (1 + 0 + 4 + 0.25) / 4
    x = np.zeros((2, 1, 1, 1, 2, 2), dtype=np.float32)
    x[0, 0, 0, 0] = [[1.0, 0.5], [0.0, 0.75]]
    x[1, 0, 0, 0] = [[0.0, 0.5], [2.0, 0.25]]
    m = ref.pairwise_frame_mse(x)
    assert m.shape == (1, 1, 2, 2) and m.dtype == np.float64
    assert np.array_equal(m[0, 0], [[0.0, 1.3125], [1.3125, 0.0]])
    # three samples, T = 2, B = 2, one pixel; the step range picks step 1 only
    x = np.zeros((3, 2, 2, 1, 1, 1), dtype=np.float32)
    x[:, 0] = 9.0                                       # step 0 must not enter
    x[:, 1, 0, 0, 0, 0] = [0.0, 1.0, 3.0]
    x[:, 1, 1, 0, 0, 0] = [2.0, 2.0, -1.0]
    m = ref.pairwise_frame_mse(x, 1, 2)
    assert m.shape == (1, 2, 3, 3)
    assert np.array_equal(m[0, 0], [[0, 1, 9], [1, 0, 4], [9, 4, 0]])
    assert np.array_equal(m[0, 1], [[0, 0, 9], [0, 0, 9], [9, 9, 0]])
    pair, psnr, distinct = ref.diversity(m)
    assert pair.shape == (2, 1) and np.allclose(pair[:, 0], [14 / 3, 6.0], rtol=1e-15)
    assert np.allclose(psnr[:, 0], [10 * np.log10(3 / 14), 10 * np.log10(1 / 6)], rtol=1e-15)
    assert distinct.tolist() == [[3], [2]]
    assert np.array_equal(ref.pairwise_frame_mse(x, 0, 1), np.zeros((1, 2, 3, 3)))
    assert np.isposinf(ref.diversity(ref.pairwise_frame_mse(x, 0, 1))[1]).all()


def test_distinct_rule_on_a_matrix_with_repeated_rows():
    # samples 0 = 2 = 5, 1 = 4, 3 alone: three different frames
    groups = [0, 1, 0, 2, 1, 0]
    m = np.array([[0.0 if a == b else 1.0 + abs(a - b) for b in groups] for a in groups])
    assert ref.distinct(m) == 3
    assert ref.distinct(np.zeros((4, 4))) == 1 and ref.distinct(np.ones((4, 4)) - np.eye(4)) == 4
    assert ref.distinct(np.zeros((1, 1))) == 1
    assert ref.distinct(np.stack([m, np.zeros((6, 6))])).tolist() == [3, 1]
