"""ctypes binding of libdvg_hip.so, derived at import from the one written form of its C ABI, include/dvg_hip.h.

The compiler holds every `extern "C"` definition to its declaration in that header (each .hip file includes it); the strict
parser below turns the same declarations into SIGNATURES and the header's `#define DVG_<NAME> <integer>` lines into CONSTANTS.
An entry point is declared, defined and called: there is no table to keep (docs/DESIGN_NOTES_abi_binding.md).

The product path has NO fallback: if the header or the shared object is missing, a declaration is not understood or a symbol
is absent, this raises.  Nothing in here touches a GPU; loading works on a CPU-only box (the HIP runtime is only initialised
by the first kernel launch).
"""
from __future__ import annotations

import ctypes as C
import os
import re
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# DVG_HIP_LIB: an alternative BUILD of the same library (kernel A/B experiments, `make variant`); still no fallback
LIB_PATH = os.environ.get("DVG_HIP_LIB") or os.path.join(_HERE, "csrc", "libdvg_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "dvg_hip.h")


class DvgLibraryError(RuntimeError):
    pass


# the header's whole vocabulary; a pointer parameter, whatever it points to, binds as c_void_p
_SCALAR = {"int": C.c_int, "long": C.c_long, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double,
           "unsigned": C.c_uint, "unsigned int": C.c_uint}
_RETURN = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "const char*": C.c_char_p, "void": None}
_TYPE_WORDS = frozenset("void char short int long float double signed unsigned const volatile struct union enum".split())
_NAME = r"[A-Za-z_]\w*"
_IDENTIFIER = re.compile(_NAME)
_POINTER = re.compile(rf"{_NAME}(?: {_NAME})* ?(?:\* ?(?:const ?)?)+({_NAME})?")      # words, stars (each may be const), [name]
_DECLARATION = re.compile(rf"(.+?[ *])({_NAME}) ?\(([^()]*)\)")                       # <ret> name(<params>): no nested parentheses
_INTEGER = re.compile(r"[-+]?(?:0[xX][0-9a-fA-F]+|0|[1-9][0-9]*)")                    # no suffix, no octal
_DIRECTIVE = re.compile(rf"# ?(include|ifdef|ifndef|endif|define)\b ?({_NAME})? ?(.*)")
_ENUM = re.compile(r"enum ?\{([^{}]*)\}")                                             # anonymous, no trailing comma
_ENUMERATOR = re.compile(rf"(DVG_\w+) ?= ?({_INTEGER.pattern})")


def _parameter(text: str):
    """The ctypes class of one parameter (its name is optional); None when it is outside the grammar."""
    if "*" in text:
        m = _POINTER.fullmatch(text)
        return C.c_void_p if m and m.group(1) not in _TYPE_WORDS else None
    if text in _SCALAR:
        return _SCALAR[text]
    kind, _, name = text.rpartition(" ")
    return _SCALAR.get(kind) if _IDENTIFIER.fullmatch(name) and name not in _TYPE_WORDS else None


def parse_header(text: str, where: str = "include/dvg_hip.h"):
    """(SIGNATURES, CONSTANTS) of a header made of comments, #include / #ifdef / #ifndef / #endif lines, an include guard,
    `#define DVG_<NAME> <integer literal>` lines, at most one `extern "C" { }` block and statements `<ret> dvg_<name>(<params>);`
    over the types above or `enum { DVG_<NAME> = <integer literal>, ... };` (read by parse_header_enums).  Anything else raises
    DvgLibraryError quoting the text: nothing is skipped."""
    return _parse(text, where)[:2]


def parse_header_enums(text: str, where: str = "include/dvg_hip.h"):
    """ENUMS of the same header: NAME -> value over every enumerator of its anonymous `enum { DVG_<NAME> = <integer literal>, ... };`
    statements - every enumerator with its value written out, the same literals as the defines.  Codes that entered the ABI as
    a family of their own (DVG_GP_KERNEL_*) live here; CONSTANTS stays the set of the defines."""
    return _parse(text, where)[2]


def _parse(text: str, where: str):
    def refuse(why, quote):
        raise DvgLibraryError(f"{where}: {why}: {quote}")
    signatures, constants, enums, code, guard = {}, {}, {}, [], None
    for line in re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S).splitlines():
        line = " ".join(line.split())
        if not line.startswith("#"):
            code.append(line)
            continue
        m = _DIRECTIVE.fullmatch(line)
        if not m:
            refuse("preprocessor line not understood", line)
        directive, name, value = m.groups()
        if directive == "ifndef":
            guard = name
        if directive != "define" or (name == guard and not value):                   # `#ifndef G` + `#define G`: the include guard
            continue
        if not (name or "").startswith("DVG_") or not _INTEGER.fullmatch(value):
            refuse("define is not `DVG_<NAME> <integer literal>`", line)
        if constants.setdefault(name[4:], int(value, 0)) != int(value, 0):
            refuse(f"define given twice with different values ({constants[name[4:]]} before)", line)
    body = " ".join(" ".join(code).split())
    m = re.fullmatch(r'extern "C" \{(.*)\}', body)
    *statements, rest = (m.group(1) if m else body).split(";")
    if rest.strip():
        refuse("text after the last declaration", rest.strip())
    for s in map(str.strip, statements):
        m = _ENUM.fullmatch(s)
        if m:
            for item in map(str.strip, m.group(1).split(",")):
                e = _ENUMERATOR.fullmatch(item)
                if not e or e.group(1)[4:] in enums or e.group(1)[4:] in constants:
                    refuse("enumerator is not a new `DVG_<NAME> = <integer literal>`", s)
                enums[e.group(1)[4:]] = int(e.group(2), 0)
            continue
        m = _DECLARATION.fullmatch(s)
        if m:
            ret, name, params = re.sub(r" ?\* ?", "*", m.group(1)).strip(), m.group(2), m.group(3).strip()
            args = [] if params == "void" else [_parameter(p.strip()) for p in params.split(",")]
        if not m or ret not in _RETURN or not name.startswith("dvg_") or None in args:
            refuse("not a declaration `<ret> dvg_<name>(<params>)` with int / long / int64_t / float / double / unsigned / pointer "
                   "parameters, returning int / long / void / size_t / const char*", s)
        if name in signatures:
            refuse("entry point declared twice", s)
        signatures[name] = (_RETURN[ret], args)
    return signatures, constants, enums


def _read_header(path: str):
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise DvgLibraryError(f"{path}: cannot read the C ABI header, and the binding exists nowhere else ({e})") from e
    return _parse(text, path)


# name -> (restype, [argtypes]) of every entry point the header declares; NAME -> value of every `#define DVG_<NAME> <value>`;
# NAME -> value of every enumerator `DVG_<NAME> = <value>`
SIGNATURES, CONSTANTS, ENUMS = _read_header(HEADER_PATH)

_lock = threading.Lock()
_lib = None


def lib() -> C.CDLL:
    """Load (once) and return the kernel library; raise loudly when unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise DvgLibraryError(
                f"{LIB_PATH} not found: the HIP kernel library has not been built. "
                "Run `python -c 'import __graft_entry__ as g; g.build()'` (or `make -C dvg_amd/csrc`). "
                "There is no CPU/eager fallback for the DVG hot path.")
        # Two HIP runtimes live in a PyTorch-ROCm process: the one torch bundles and the system one this library links
        # (/opt/rocm).  They coexist when torch's comes up FIRST; with the library loaded before torch has initialised its
        # runtime, every launch from here fails with "no ROCm-capable device is detected" (seen with build() and smoke() in
        # one process).  So: bring torch's runtime up before the dlopen.  (No GPU - the cross-compile container, the ABI
        # tests - nothing to initialise.)
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except ImportError:  # pragma: no cover - a host without torch binds the C ABI directly
            pass
        try:
            handle = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise DvgLibraryError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                raise DvgLibraryError(f"{LIB_PATH} lacks symbol {name}; rebuild it") from e
            fn.restype = res
            fn.argtypes = args
        _lib = handle
        return _lib


def build_info() -> dict:
    """dvg_build_info() parsed: {"abi": 9, "bf16x3": 1, "variant": "", "src": "<sha256[:12] of the sources>"} plus "path"
    (the file loaded), "from_env" (DVG_HIP_LIB was set) and "product": True only for the library the repository ships - the
    default path or the in-tree f32-MFMA comparison build, no variant name."""
    raw = lib().dvg_build_info().decode()
    d = {}
    for tok in raw.split():
        k, _, v = tok.partition("=")
        d[k] = int(v) if v.lstrip("-").isdigit() else v
    d["raw"] = raw
    d["path"] = LIB_PATH
    d["from_env"] = bool(os.environ.get("DVG_HIP_LIB"))
    shipped = {os.path.join(_HERE, "csrc", "libdvg_hip.so"), os.path.join(_HERE, "csrc", "libdvg_hip_f32mfma.so")}
    d["product"] = os.path.abspath(LIB_PATH) in shipped and d.get("variant", "") == ""
    return d


def check(code: int, what: str = "") -> None:
    """Translate a DVG_ERR_* status into a RuntimeError (SURVEY.md §8(b) 'Errors')."""
    if code != 0:
        msg = lib().dvg_last_error()
        raise RuntimeError(f"libdvg_hip {what} failed (code {code}): {msg.decode() if msg else '?'}")
