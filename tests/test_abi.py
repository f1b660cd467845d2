"""CPU: the binding dvg_amd/_lib.py derives from include/dvg_hip.h - its parser on a synthetic header and on every refusal, the
derived table against an independent reading of every declaration, the header's integer codes - and the built libraries, which
export exactly what the header declares (no compute)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from tests.common import ROOT, header_declaration, header_symbols, header_text


def test_header_declares_entry_points():
    syms = header_symbols()
    assert len(syms) >= 25
    for must in ("dvg_conv3x3_bn_act_v2", "dvg_lstm_cell", "dvg_gp_predict", "dvg_gemm_nt_bias_act"):
        assert must in syms


SYNTHETIC_HEADER = """\
/* a block comment that holds a declaration:
 *   int dvg_fake(int);                                  */
#ifndef DVG_SYNTHETIC_H
#define DVG_SYNTHETIC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
// a line comment that holds one: int dvg_fake_too(void);
#define DVG_OK 0
#define DVG_ERR_ALIGN 4   /* pointer not 16-byte aligned */
#define DVG_MASK 0x1F     // hexadecimal
#define DVG_NONE -1
#define DVG_OK 0
int dvg_version(void);
const char* dvg_error(void);
const char *dvg_info( void );
long dvg_capture(void* stream);
size_t dvg_bytes(int, long, int64_t);
void dvg_hook(void* buf, unsigned records, unsigned int more);
int dvg_three_lines(const float* x, float *y, const float* const* items, long n,
                    float slope, double count, /* a comment between parameters */ int64_t frames,
                    const uint8_t* mask, long long* cnt, const unsigned char** rows, void* stream);
int dvg_unnamed(const float*, float, double, unsigned, unsigned int, const int* const*, float* const);
#ifdef __cplusplus
}
#endif
#endif /* DVG_SYNTHETIC_H */
"""


def test_parser_reads_every_accepted_construct_of_a_synthetic_header():
    from dvg_amd import _lib
    p, i, l, f, d, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double, ctypes.c_uint
    signatures, constants = _lib.parse_header(SYNTHETIC_HEADER)
    assert constants == {"OK": 0, "ERR_ALIGN": 4, "MASK": 31, "NONE": -1}
    expected = {
        "dvg_version": (i, []),
        "dvg_error": (ctypes.c_char_p, []),
        "dvg_info": (ctypes.c_char_p, []),
        "dvg_capture": (l, [p]),
        "dvg_bytes": (ctypes.c_size_t, [i, l, ctypes.c_int64]),
        "dvg_hook": (None, [p, u, u]),
        "dvg_three_lines": (i, [p, p, p, l, f, d, ctypes.c_int64, p, p, p, p]),
        "dvg_unnamed": (i, [p, f, d, u, u, p, p]),
    }
    assert signatures == expected and list(signatures) == list(expected)
    for name, (restype, argtypes) in expected.items():            # == on ctypes classes is identity; say so
        assert signatures[name][0] is restype and all(a is b for a, b in zip(signatures[name][1], argtypes)), name
    assert _lib.parse_header("") == ({}, {}) and _lib.parse_header("int dvg_bare(int n);") == ({"dvg_bare": (i, [i])}, {})


REFUSALS = {    # case -> (header text, the offending text the message must quote)
    "short": ("int dvg_a(const float* x, short n);", "int dvg_a(const float* x, short n)"),
    "char by value": ("int dvg_a(char c);", "int dvg_a(char c)"),
    "bool": ("int dvg_a(bool flag);", "int dvg_a(bool flag)"),
    "long long by value": ("int dvg_a(long long n);", "int dvg_a(long long n)"),
    "unnamed long long": ("int dvg_a(long long);", "int dvg_a(long long)"),
    "struct": ("int dvg_a(struct dvg_shape s);", "int dvg_a(struct dvg_shape s)"),
    "const scalar": ("int dvg_a(const int n);", "int dvg_a(const int n)"),
    "array": ("int dvg_a(float v[4]);", "int dvg_a(float v[4])"),
    "pointer array": ("int dvg_a(float* v[4]);", "int dvg_a(float* v[4])"),
    "function pointer": ("int dvg_a(int (*done)(int));", "int dvg_a(int (*done)(int))"),
    "variadic": ("int dvg_a(int n, ...);", "int dvg_a(int n, ...)"),
    "empty parameter list": ("int dvg_a();", "int dvg_a()"),
    "return type": ("float dvg_a(int n);", "float dvg_a(int n)"),
    "non-dvg name": ("int dvg_a(int n);\nint other_b(int n);", "int other_b(int n)"),
    "declared twice": ("int dvg_a(int n);\nint dvg_b(void);\nint dvg_a(int n);", "int dvg_a(int n)"),
    "typedef": ("typedef int dvg_status;", "typedef int dvg_status"),
    "missing semicolon": ("int dvg_a(int n);\nint dvg_b(void)", "int dvg_b(void)"),
    "unclosed comment": ("int dvg_a(int n); /* int dvg_b(void);", "/* int dvg_b(void)"),
    "float define": ("#define DVG_EPS 1.5", "#define DVG_EPS 1.5"),
    "suffixed define": ("#define DVG_N 8u", "#define DVG_N 8u"),
    "expression define": ("#define DVG_N (1 << 3)", "#define DVG_N (1 << 3)"),
    "octal define": ("#define DVG_N 010", "#define DVG_N 010"),
    "macro with parameters": ("#define DVG_MAX(a, b) 1", "#define DVG_MAX(a, b) 1"),
    "valueless define that is no guard": ("#ifndef DVG_H\n#define DVG_H\n#define DVG_FLAG\n#endif", "#define DVG_FLAG"),
    "non-DVG define": ("#define OTHER 3", "#define OTHER 3"),
    "define given twice with different values": ("#define DVG_N 1\n#define DVG_M 2\n#define DVG_N 3", "#define DVG_N 3"),
    "conditional": ("#if 0\nint dvg_a(int n);\n#endif", "#if 0"),
    "pragma": ("#pragma once", "#pragma once"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_parser_refuses_what_it_does_not_understand(case):
    from dvg_amd import _lib
    text, offending = REFUSALS[case]
    with pytest.raises(_lib.DvgLibraryError) as e:
        _lib.parse_header("int dvg_before(void);\n" + text + "\n", "synthetic.h")
    assert offending in str(e.value) and str(e.value).startswith("synthetic.h: "), str(e.value)


def test_a_missing_header_raises_with_its_path(tmp_path):
    from dvg_amd import _lib
    missing = str(tmp_path / "include" / "dvg_hip.h")
    with pytest.raises(_lib.DvgLibraryError) as e:
        _lib._read_header(missing)
    assert missing in str(e.value)
    assert os.path.samefile(_lib.HEADER_PATH, os.path.join(ROOT, "include", "dvg_hip.h"))


def _classify(param):
    """A parameter's ctypes class, read off the header's spelling without the parser: a star is a pointer, else the first word."""
    if "*" in param:
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "long": ctypes.c_long, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "double": ctypes.c_double, "unsigned": ctypes.c_uint}[param.split()[0]]


def test_binding_agrees_with_an_independent_reading_of_every_declaration():
    """What four feature tests used to check for six names, for all of them: argument by argument and the return type."""
    from dvg_amd import _lib
    returns = {"int": ctypes.c_int, "long": ctypes.c_long, "void": None, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}
    assert sorted(_lib.SIGNATURES) == header_symbols() and len(header_symbols()) == len(_lib.SIGNATURES)
    for name in header_symbols():
        ret, params = header_declaration(name)
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is returns[ret.replace(" *", "*")], (name, ret, restype)
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        for k, (a, t) in enumerate(zip(params, argtypes)):
            assert t is _classify(a), (name, k, a, t)


def test_library_exports_every_declared_symbol():
    from dvg_amd import _lib
    for so in ("libdvg_hip.so", "libdvg_hip_f32mfma.so"):
        path = os.path.join(os.path.dirname(_lib.LIB_PATH), so)
        assert os.path.exists(path), f"{so} not built (python -c 'import __graft_entry__ as g; g.build()')"
        handle = ctypes.CDLL(path)
        for s in header_symbols():
            assert hasattr(handle, s), f"{s} declared in include/dvg_hip.h but not exported by {so}"


def test_library_exports_no_entry_point_the_header_does_not_declare():
    from dvg_amd import _lib
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("no nm on this machine")
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(w[-1] for w in map(str.split, out.splitlines()) if w and w[-1].startswith("dvg_"))
    assert exported == header_symbols(), sorted(set(exported) ^ set(header_symbols()))


def test_binding_table_covers_header():
    from dvg_amd import _lib
    assert sorted(_lib.SIGNATURES) == header_symbols()
    lib = _lib.lib()
    assert lib.dvg_abi_version() == 9
    for name, (restype, argtypes) in _lib.SIGNATURES.items():              # lib() bound what the header gave
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_both_builds_of_the_library_load_and_say_which_arithmetic_they_run():
    """libdvg_hip.so forms the implicit-GEMM kernels' fp32 products as exact bf16 triples on the bf16 MFMA (packed weight
    rows of 3 x 16 bf16 = 24 floats), libdvg_hip_f32mfma.so (make f32mfma; built by __graft_entry__.build()) with the native
    f32 MFMA (rows of 16 floats); both export the same ABI."""
    from dvg_amd import _lib
    assert _lib.lib().dvg_mfma_mode() == 1 and _lib.lib().dvg_packed_row_floats() == 24
    native = os.path.join(os.path.dirname(_lib.LIB_PATH), "libdvg_hip_f32mfma.so")
    assert os.path.exists(native), "libdvg_hip_f32mfma.so not built (make -C dvg_amd/csrc f32mfma)"
    h = ctypes.CDLL(native)
    for s in header_symbols():
        assert hasattr(h, s), f"{s} missing from the f32-MFMA build"
    assert h.dvg_abi_version() == 9 and h.dvg_mfma_mode() == 0 and h.dvg_packed_row_floats() == 16


def test_build_info_identifies_the_knob_free_product_build():
    """dvg_build_info() (ABI 9): both shipped libraries say which arithmetic they run, carry no variant name and were built
    from THIS tree (src = sha256 over the sources, as `make srcid` computes it); the sources have no compile-time override
    point but the product / f32-MFMA switch and the build identity, and only `make variant` passes extra defines, so `make
    all` builds exactly the committed kernels."""
    import subprocess
    from dvg_amd import _lib
    info = _lib.build_info()
    assert info["abi"] == 9 and info["bf16x3"] == 1 and info["variant"] == "" and info["product"]
    csrc = os.path.dirname(_lib.LIB_PATH)
    srcid = subprocess.run(["make", "-s", "-C", csrc, "srcid"], capture_output=True, text=True, check=True).stdout.split()[-1]
    assert info["src"] == srcid, "libdvg_hip.so is older than its sources: rebuild (make -C dvg_amd/csrc all f32mfma)"
    h = ctypes.CDLL(os.path.join(csrc, "libdvg_hip_f32mfma.so"))
    h.dvg_build_info.restype = ctypes.c_char_p
    raw = h.dvg_build_info().decode()
    assert "bf16x3=0" in raw and " variant= " in raw and f"src={srcid}" in raw
    overrides = set()
    for name in os.listdir(csrc):
        if name.endswith((".hip", ".h", ".cpp")):
            src = open(os.path.join(csrc, name)).read()
            overrides |= set(re.findall(r"#\s*(?:ifndef\s+|if\s+!\s*defined\s*\(?\s*)(DVG_\w+)", src))
    assert overrides == {"DVG_BF16X3", "DVG_SRC_ID", "DVG_VARIANT_NAME"}, f"compile-time override points: {sorted(overrides)}"
    mk = open(os.path.join(csrc, "Makefile")).read()
    product_rules = mk[:mk.index("# A/B builds")]
    assert "$(DEFS)" not in product_rules, "DEFS must reach the `variant` objects only"


def test_host_side_checks_reject_bad_shapes_without_gpu():
    """Shape validation happens on the host before any launch, so it is testable on CPU."""
    from dvg_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(16)  # fake, never dereferenced: the call must fail in the checks
    rc = lib.dvg_conv3x3_bn_act_v2(one, None, one, None, None, one, None, None, 1, 8, 8, 40, 0, 64, 0, 1, 0.2, None, 0,
                                   None, None, 0, None)
    assert rc == 1 and b"16" in lib.dvg_last_error(), lib.dvg_last_error()
    rc = lib.dvg_lstm_cell(one, one, one, one, one, one, one, one, one, None, 4, 100, None)
    assert rc == 1
    rc = lib.dvg_gp_predict(*([one] * 7), None, None, one, None, None, None, None, 200, 90, 40, 0, 1e-3, 0, 1, None)
    assert rc == 1
    with pytest.raises(RuntimeError):
        _lib.check(rc, "gp")
    assert lib.dvg_conv_stats_rows_v2(0, 64, 64, 64, 64, 64, 0, 0) > 0
    assert lib.dvg_conv_splitk_v2(0, 64, 64, 64, 64, 64) == 1          # 2048 workgroups: no split
    assert lib.dvg_conv_splitk_v2(0, 64, 8, 8, 512, 256) == 2          # 256 workgroups, K = 32 chunks
    assert lib.dvg_conv_splitk_v2(0, 16, 8, 8, 512, 512) == 4          # per-GPU batch 16
    # r06 tile policy: LATENCY (default) = the r05 chooser, ENERGY = the 8 x 16 tile from 256 workgroups on - whose kernels never
    # split K, and the host helpers must say so too (320 workgroups would split on an 8-wide tile)
    assert lib.dvg_tile_policy() == 0
    assert lib.dvg_conv_splitk_v2(0, 10, 64, 64, 64, 64) == 1 and lib.dvg_conv_stats_rows_v2(0, 10, 64, 64, 64, 64, 0, 1) == 640
    lib.dvg_set_tile_policy(1)
    try:
        assert lib.dvg_tile_policy() == 1
        assert lib.dvg_conv_splitk_v2(0, 10, 64, 64, 64, 64) == 1
        assert lib.dvg_conv_stats_rows_v2(0, 10, 64, 64, 64, 64, 0, 1) == lib.dvg_conv_stats_rows_v2(0, 10, 64, 64, 64, 64, 0, 0) == 320
        assert lib.dvg_conv_stats_rows_v2(0, 7, 64, 64, 64, 64, 0, 1) == 448       # 224 < 256 workgroups: 8 x 8 tiles
    finally:
        lib.dvg_set_tile_policy(0)
    assert lib.dvg_tile_policy() == 0
    from dvg_amd import ops
    with ops.tile_policy(True):
        assert lib.dvg_tile_policy() == 1
        with ops.tile_policy(False):
            assert lib.dvg_tile_policy() == 0
        assert lib.dvg_tile_policy() == 1
    assert lib.dvg_tile_policy() == 0
    assert lib.dvg_gp_lds_bytes(64, 40, 1) <= 160 * 1024 and lib.dvg_gp_precision(64, 40, 1) == 64
    # r05 entry points: the checks fire before anything is launched
    assert lib.dvg_gemm_tn(one, one, None, None, None, 8, 8, 8, 8, 8, 8, 0, 0, None) == 2                  # no output (DVG_ERR_NULL)
    assert lib.dvg_gemm_tn(one, one, one, None, one, 8, 8, 8, 8, 8, 8, 0, 0, None) == 2                    # second sink without first
    assert lib.dvg_gemm_tn(one, one, one, None, None, 8, 16, 8, 8, 8, 8, 0, 0, None) == 1                  # lda < M
    assert lib.dvg_conv4x4s2_bn_act_v2(one, one, None, None, one, None, 40000, 128, 128, 64, 64, 0, 0.2, None, 0, None) == 1
    assert b"32-bit offsets" in lib.dvg_last_error()
    gp = [one] * 7 + [None, None, one, one, None, None, one]                # h .. lengthscale, noise, eps, mean, var, sample, cov, kl
    assert lib.dvg_gp_predict(*gp, 16, 990, 40, 1, 1e-3, 90, 12, None) == 1                                 # step_group > S = 11
    assert lib.dvg_gp_predict(*gp, 64, 1710, 40, 1, 1e-3, 90, 4, None) == 1 and b"fp64" in lib.dvg_last_error()   # 256 points: no fp64 fit
    # the host side's choice of steps per workgroup for a time-batched GP call (dvg_gp_step_group: B, S, latent dims, M)
    assert [lib.dvg_gp_step_group(*a) for a in ((16, 11, 90, 40), (4, 15, 90, 40), (64, 19, 90, 40), (16, 2, 90, 40),
                                               (50, 14, 90, 40), (16, 1, 90, 40))] == [6, 8, 1, 1, 1, 1]


def test_product_has_no_cpu_fallback():
    import torch
    from dvg_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.conv3x3_first(torch.zeros(1, 1, 8, 8), torch.zeros(64, 1, 3, 3), None, None)


def integration_snippet() -> str:
    """The fenced python block of INTEGRATION.md ("What a maintainer of the reference would add")."""
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"```python\n(.*?)```", txt, flags=re.S)
    assert m, "INTEGRATION.md lost its binding example"
    return m.group(1)


def test_integration_document_binds_the_header_signature():
    """the example binding in INTEGRATION.md had drifted from include/dvg_hip.h (21 arguments for the
    23-argument dvg_conv3x3_bn_act_v2).  Executed here VERBATIM up to the point where it would need a GPU: the snippet
    loads the library, sets argtypes - which must equal what dvg_amd/_lib.py derives from the header - and defines
    vgg_layer_eval.  tests/test_gpu_parity.py::test_integration_snippet_runs_verbatim calls it on the GPU."""
    from dvg_amd import _lib
    ns = {}
    old = os.environ.get("DVG_HIP_LIB")
    os.environ["DVG_HIP_LIB"] = _lib.LIB_PATH
    try:
        exec(compile(integration_snippet(), "INTEGRATION.md", "exec"), ns)
    finally:
        if old is None:
            del os.environ["DVG_HIP_LIB"]
        else:
            os.environ["DVG_HIP_LIB"] = old
    h = ns["_lib"]
    for name in ("dvg_conv3x3_bn_act_v2", "dvg_pack_conv_weight_k16", "dvg_packed_row_floats"):
        restype, argtypes = _lib.SIGNATURES[name]
        fn = getattr(h, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes), name
    assert callable(ns["vgg_layer_eval"])
    # the number of arguments the document's call passes == the header's parameter count
    call = re.search(r"_lib\.dvg_conv3x3_bn_act_v2\((.*?)\)\)", integration_snippet(), flags=re.S).group(1)
    call = re.sub(r"#[^\n]*", "", call)
    n_args = len([a for a in re.sub(r"\([^()]*\)", "", call).split(",") if a.strip()])
    assert n_args == len(_lib.SIGNATURES["dvg_conv3x3_bn_act_v2"][1]) == 23, n_args


def test_python_constants_match_the_header():
    """Every integer code the Python side takes from include/dvg_hip.h, against literal values: these numbers are baked into the
    built kernels, so a header that renumbers or reorders them must fail here."""
    from dvg_amd import _lib, ops, viz
    codes = {"ACT_NONE": 0, "ACT_LRELU": 1, "ACT_TANH": 2, "ACT_SIGMOID": 3, "MODE_CONV3": 0, "MODE_CONV4S2": 1, "MODE_CONVT4S2": 2,
             "QUANT_TRUNC": 0, "QUANT_NEAREST": 1, "MOSAIC_BLACK": 0, "MOSAIC_RED": 1, "MOSAIC_GREEN": 2, "MOSAIC_SEL_NONE": 0,
             "MOSAIC_SEL_BEST": 1, "MOSAIC_SEL_PICK": 2, "MOSAIC_CELL_INTS": 8}
    for name, v in codes.items():
        assert getattr(ops, name) == v and type(getattr(ops, name)) is int, name
    assert (viz.QUANT_TRUNC, viz.QUANT_NEAREST) == (0, 1) and (viz.BLACK, viz.RED, viz.GREEN) == (0, 1, 2)
    assert (viz.SEL_NONE, viz.SEL_BEST, viz.SEL_PICK) == (0, 1, 2) and viz.CELL_INTS == 8
    assert _lib.CONSTANTS == {**codes, "OK": 0, "ERR_SHAPE": 1, "ERR_NULL": 2, "ERR_HIP": 3, "ERR_ALIGN": 4}
    # and the header read without the parser: every valued define is a constant, the include guard is not
    assert {k: int(v) for k, v in re.findall(r"#define\s+DVG_(\w+)[ \t]+(\d+)", header_text())} == _lib.CONSTANTS
    assert "HIP_H" not in _lib.CONSTANTS
