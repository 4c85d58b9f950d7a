"""ctypes binding of libsrk_gfx950.so, derived from include/srk.h (the C ABI) when this module is imported.

Nothing of the header is repeated here.  parse_header() reads it once and gives
  - a ctypes.Structure per `typedef struct { ... } srk_x_args;`, published as STRUCTS["srk_x_args"] and as the module attribute
    XArgs (drop `srk_`, capitalise each `_`-separated part: srk_wgrad_fin_args -> WgradFinArgs).  Fields keep the header's names and
    order; every pointer is c_void_p, int / float / double / long long are c_int / c_float / c_double / c_longlong;
  - every enum member and every `#define SRK_NAME <integer>` as a module attribute under its header name;
  - PROTOTYPES[name] = (restype, argtypes) for every declared function, which bind() sets on the loaded library.  LAUNCHERS maps the
    `int f(const srk_x_args* a, srk_stream_t stream)` functions to their struct; OTHER_SYMBOLS names the rest.
Parameter convention: a pointer to an srk_* struct binds as POINTER(Class), so call sites pass a struct, an array of them or byref();
a struct pointer whose NAME contains `table` (table, table_dev, host_table) is an address the caller computed (tensor.data_ptr(),
ctypes.addressof) and binds as c_void_p, like every pointer to a scalar or to void and like srk_stream_t.
The parser knows the few C forms the header uses and raises on any statement it does not understand; it never skips one.

There is NO fallback: if the shared library is missing or a launcher returns non-zero, a RuntimeError
is raised (the product path never routes through the CPU oracle).
"""
import ctypes as C
import os
import re
from types import SimpleNamespace

_HERE = os.path.dirname(os.path.abspath(__file__))
# SRK_LIB_PATH: A/B timing of two builds of the same library (tools/); never a different implementation
# SRK_EXACT_RELU=1: the build of the same sources whose ReLU keeps a NaN like torch.relu (csrc/srk_common.h, `make exact`); default: one
# instruction per value, a NaN pre-activation becomes 0 (fp32) / keeps its payload only with a clear sign bit (16-bit)
EXACT_RELU = os.environ.get("SRK_EXACT_RELU") == "1"
LIB_PATH = os.environ.get("SRK_LIB_PATH") or os.path.join(_HERE, "libsrk_gfx950_exact.so" if EXACT_RELU else "libsrk_gfx950.so")

_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "long long": C.c_longlong}
_RESTYPES = {"int": C.c_int, "long long": C.c_longlong, "const char*": C.c_char_p}
# `[const] type declarator, declarator`: the scalar types, and the types the header only ever points at
_DECL = re.compile(r"(?:const\s+)?(int|float|double|long long|void|signed char|unsigned int|uint8_t|srk_\w+)\b(.*)", re.S)
_NAME = re.compile(r"\s*(\*?)\s*(\w+)\s*")
# preprocessor lines without a value: the include guard, <stdint.h>, and the `extern "C"` wrapper
_CPP_PLAIN = re.compile(r'#\s*(ifndef SRK_H|define SRK_H|endif|include <stdint\.h>|ifdef __cplusplus)')


def _refuse(stmt):
    raise ValueError(f"include/srk.h: statement not understood by the binding's parser: {' '.join(stmt.split())!r}")


def _declarators(stmt):
    """`const float *a, *b` -> ("float", [(True, "a"), (True, "b")]); `int x_pitch, x_coff` -> ("int", [(False, "x_pitch"), ...])."""
    m = _DECL.fullmatch(stmt.strip())
    names = [_NAME.fullmatch(d) for d in m.group(2).split(",")] if m else [None]
    if not all(names):
        _refuse(stmt)
    return m.group(1), [(bool(d.group(1)), d.group(2)) for d in names]


def _statements(text):
    """The top-level statements of `text`: cut at every `;` outside braces."""
    depth = start = 0
    for m in re.finditer(r"[{};]", text):
        if m.group() == ";" and depth == 0:
            yield text[start:m.start()].strip()
            start = m.end()
        depth += {"{": 1, "}": -1, ";": 0}[m.group()]
    if text[start:].strip():
        _refuse(text[start:])


def parse_header(text):
    """structs (C name -> ctypes.Structure), consts (name -> int), protos (name -> (restype, argtypes)) and launchers (name ->
    Structure) of a header written in the forms of include/srk.h; raises ValueError, quoting it, on any other statement."""
    h = SimpleNamespace(structs={}, consts={}, protos={}, launchers={})
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r'^extern "C" \{$|^\}$(?=\s*#\s*endif)', "", text, flags=re.M)       # the two halves of the __cplusplus wrapper
    for line in re.findall(r"^\s*#.*$", text, flags=re.M):
        m = re.fullmatch(r"\s*#\s*define\s+(SRK_\w+)\s+(-?\d+)\s*", line)
        if m:
            h.consts[m.group(1)] = int(m.group(2))
        elif not _CPP_PLAIN.fullmatch(line.strip()):
            _refuse(line)
    for stmt in _statements(re.sub(r"^\s*#.*$", "", text, flags=re.M)):
        if stmt == "typedef void* srk_stream_t":
            continue
        m = re.fullmatch(r"enum\s*\{(.*)\}", stmt, flags=re.S)
        if m:
            for member in m.group(1).split(","):
                mm = re.fullmatch(r"\s*(\w+)\s*=\s*(-?\d+)\s*", member)
                if not mm:
                    _refuse(stmt)
                h.consts[mm.group(1)] = int(mm.group(2))
            continue
        m = re.fullmatch(r"typedef struct(?:\s+\w+)?\s*\{(.*)\}\s*(srk_\w+)", stmt, flags=re.S)
        if m:
            fields = []
            *decls, rest = m.group(1).split(";")
            if rest.strip():
                _refuse(rest)                   # a member without its `;`
            for decl in decls:
                base, names = _declarators(decl)
                for ptr, name in names:
                    if not ptr and base not in _SCALARS:
                        _refuse(decl)
                    fields.append((name, C.c_void_p if ptr else _SCALARS[base]))
            cname = m.group(2)
            h.structs[cname] = type("".join(p.capitalize() for p in cname.split("_")[1:]), (C.Structure,), {"_fields_": fields})
            continue
        m = re.fullmatch(r"(int|long long|const char\*)\s+(srk_\w+)\s*\(([^()]*)\)", stmt)
        if not m:
            _refuse(stmt)
        ret, fname, params = m.groups()
        argtypes = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            if re.fullmatch(r"\s*srk_stream_t\s+\w+\s*", param):
                argtypes.append(C.c_void_p)
                continue
            base, names = _declarators(param)
            (ptr, name), = names
            if not ptr and base in _SCALARS:
                argtypes.append(_SCALARS[base])
            elif ptr and base in h.structs:
                argtypes.append(C.c_void_p if "table" in name else C.POINTER(h.structs[base]))
            elif ptr and not base.startswith("srk_"):
                argtypes.append(C.c_void_p)
            else:
                _refuse(stmt)                   # a struct by value, or one the header has not declared yet
        h.protos[fname] = (_RESTYPES[ret], argtypes)
        m = re.fullmatch(r"\s*const\s+(srk_\w+)\s*\*\s*(\w+)\s*,\s*srk_stream_t\s+\w+\s*", params)
        if ret == "int" and m and "table" not in m.group(2):
            h.launchers[fname] = h.structs[m.group(1)]
    return h


def _read_header():
    path = os.path.join(_HERE, "..", "include", "srk.h")      # the path csrc/Makefile compiles against
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: the ctypes binding is derived from it")
    with open(path, encoding="utf-8") as f:
        return parse_header(f.read())


_H = _read_header()
STRUCTS = _H.structs                    # "srk_conv_args" -> ConvArgs, ...
PROTOTYPES = _H.protos                  # every function include/srk.h declares: name -> (restype, argtypes)
LAUNCHERS = _H.launchers                # the `int f(const srk_x_args* a, srk_stream_t stream)` ones: name -> argument struct
OTHER_SYMBOLS = tuple(n for n in PROTOTYPES if n not in LAUNCHERS)
globals().update(_H.consts)             # SRK_BF16, SRK_E_BADARG, SRK_FLIP_TABLE_FLOATS, ...
globals().update({cls.__name__: cls for cls in STRUCTS.values()})       # ConvArgs, WgradArgs, ...
OUT_NHWC, OUT_NHWC_PS, OUT_PLANAR = SRK_OUT_NHWC, SRK_OUT_NHWC_PS, SRK_OUT_PLANAR                    # noqa: F821
EMA_UPDATE, EMA_SWAP, EMA_STORE, EMA_LOAD = SRK_EMA_UPDATE, SRK_EMA_SWAP, SRK_EMA_STORE, SRK_EMA_LOAD   # noqa: F821
LR_SET, LR_ADVANCE = SRK_LR_SET, SRK_LR_ADVANCE                                                       # noqa: F821  (lr_sched.py: LrSchedArgs)

_lib = None


class _Absent:
    """Stands in for an entry point that an older build of the library does not have yet: calling it raises."""

    def __init__(self, name):
        self.name = name
        self.argtypes = self.restype = None

    def __call__(self, *a, **k):
        raise RuntimeError(f"{self.name} is not exported by {LIB_PATH} (an older build loaded through SRK_LIB_PATH)")


def bind(lib, older):
    """Set argtypes / restype of every declared function on `lib` (any object with attributes).  A function `lib` lacks is an error,
    unless `older`: A/B timing against an OLDER build of this library (tools/ab_lib.sh: SRK_LIB_PATH=tools/ubench/libsrk_prev.so) leaves
    the entry points that build does not have yet as _Absent stubs.  The product library (no SRK_LIB_PATH) must export everything."""
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            if not older:
                raise RuntimeError(f"{name} is declared in include/srk.h but not exported by {LIB_PATH}: "
                                   "rebuild it with `python __graft_entry__.py`")
            fn = _Absent(name)
            setattr(lib, name, fn)
        fn.argtypes, fn.restype = argtypes, restype
    return lib


def load():
    """Load the library once; raise (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the HIP path.")
    _lib = bind(C.CDLL(LIB_PATH), bool(os.environ.get("SRK_LIB_PATH")))
    return _lib


def call(name, args, stream):
    """Invoke launcher `name`; raise RuntimeError with the library's message on failure."""
    lib = load()
    if getattr(args, "N", 1) == 0:
        return          # empty batch: nothing to launch (torch's convs accept it; outputs are empty, sums stay zero)
    rc = getattr(lib, name)(C.byref(args), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError(f"{name} failed (rc={rc}): {lib.srk_last_error().decode(errors='replace')}")


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc}): {load().srk_last_error().decode(errors='replace')}")


def conv_tile(cout):
    return load().srk_conv_tile(int(cout))
