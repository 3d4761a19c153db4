"""ctypes binding of libp3d_amd.so (the C ABI declared in include/p3d_amd.h).

The header is the one description of that ABI: the ctypes signatures and the integer constants of this module are read from it at
import (parse_header), so an entry or a macro added there needs no second copy here.

The wrappers reach every entry that returns a status through call(entry, where, device, *args), which marshals by the header's
types: a tensor goes where a pointer is declared only with the declared element type and on `device`, else it raises before anything
is launched.  The size, count and profile entries are plain calls on load().

There is no fallback: if the HIP library is missing or cannot be loaded, every operator of this
package raises.  Build it with `python -m pytorch3d_amd.build` (hipcc, gfx950).
"""
import ctypes
import os
import re
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# P3D_LIB_PATH selects an ablation build (profiles/ scripts only; see build.py)
LIB_PATH = os.environ.get("P3D_LIB_PATH") or os.path.join(_HERE, "libp3d_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "p3d_amd.h")
# the extension ABI of csrc/implicit.hip, cubify.hip, volume_sample.hip, harmonic.hip, marching_cubes.hip, points_alignment.hip and
# mesh_laplacian.hip: entries p3di_*, declared in a header of their own (see its head)
EXTENSION_HEADER_PATH = os.path.join(_HERE, "csrc", "implicit_abi.h")
EXTENSION_PREFIX = "p3di_"

c_i64 = ctypes.c_int64
c_int = ctypes.c_int
c_uint = ctypes.c_uint
c_f32 = ctypes.c_float
c_f64 = ctypes.c_double
c_ptr = ctypes.c_void_p
c_size = ctypes.c_size_t


class ExtensionMissing(RuntimeError):
    pass


_SCALARS = {"int": c_int, "unsigned": c_uint, "int64_t": c_i64, "size_t": c_size, "float": c_f32, "double": c_f64}
_RETURNS = dict(_SCALARS, **{"void": None, "const char*": ctypes.c_char_p})
_WORDS = set(_SCALARS) | {"void", "char", "long", "short", "signed", "const", "struct"}  # never a parameter's name
_PARAM = re.compile(r"(const )?(\w+)(?: ?(\*))?(?: ?\b(\w+))?(?: ?(\[\d+\]))?")  # const, type, *, name, [n]


def parse_header(text, prefix="p3d_"):
    """({entry: (return type, [parameter types])}, {macro name without P3D_: integer}) of a header in the style of include/p3d_amd.h.
    The types are C spellings without the parameter names: "const float*", "int64_t", "const int64_t[2]", "p3d_stream_t".  Comments
    go first (some hold text of the form p3d_x(...)), then preprocessor lines; every statement left must be the stream typedef or a
    `RET p3d_name(PARAMS)` whose types ctypes_signature knows: anything else raises with the statement's text.  prefix: what the
    entries' names begin with (the extension header's: EXTENSION_PREFIX)."""
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    constants = {m.group(1): int(m.group(2)) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+P3D_(\w+)[ \t]+\(?(-?\d+)u?\)?[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    declarations = {}
    for statement in text.split(";"):
        statement = " ".join(statement.split())
        if statement in ("", "typedef void* p3d_stream_t"):
            continue
        m = re.fullmatch(r"(.+?) ?\b(%s\w+) ?\((.*)\)" % re.escape(prefix), statement)
        if m is None:
            raise ValueError(f"cannot parse the declaration `{statement}`")
        if m.group(2) in declarations:
            raise ValueError(f"{m.group(2)} is declared twice")
        params = []
        for param in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
            p = _PARAM.fullmatch(param.strip())
            if p is None or p.group(4) in _WORDS or (p.group(3) and p.group(5)):
                raise ValueError(f"cannot parse the parameter `{param.strip()}` of the declaration `{statement}`")
            params.append((p.group(1) or "") + p.group(2) + (p.group(3) or "") + (p.group(5) or ""))
        declarations[m.group(2)] = (m.group(1).replace(" *", "*"), params)
        ctypes_signature(*declarations[m.group(2)], where=statement)
    return declarations, constants


def ctypes_signature(ret, params, where=None):
    """(restype, [argtypes]) of a parsed declaration: scalars by _SCALARS, p3d_stream_t and every T* a c_void_p, `const T x[n]` a
    POINTER(T); returns also void and const char*.  A type outside that raises (with the declaration's text): it is never guessed."""
    def fail(ctype):
        raise ValueError(f"no ctypes type for the C type `{ctype}`" + (f" in the declaration `{where}`" if where else ""))

    def arg(ctype):
        base = ctype[len("const "):] if ctype.startswith("const ") else ctype
        if base.endswith("]"):
            base = base[:base.index("[")]
            return ctypes.POINTER(_SCALARS[base]) if base in _SCALARS else fail(ctype)
        if base == "p3d_stream_t" or (base.endswith("*") and base != "*"):
            return c_ptr
        return _SCALARS[base] if base in _SCALARS else fail(ctype)

    return (_RETURNS[ret] if ret in _RETURNS else fail(ret)), [arg(p) for p in params]


try:
    with open(HEADER_PATH) as _f:
        DECLARATIONS, CONSTANTS = parse_header(_f.read())
except OSError as e:
    raise ExtensionMissing(f"{HEADER_PATH} not found ({e}): the package reads the C ABI of libp3d_amd.so from this header") from e

try:
    with open(EXTENSION_HEADER_PATH) as _f:
        EXTENSION_DECLARATIONS, EXTENSION_CONSTANTS = parse_header(_f.read(), EXTENSION_PREFIX)
except OSError as e:
    raise ExtensionMissing(f"{EXTENSION_HEADER_PATH} not found ({e}): the package reads the ABI of csrc/implicit.hip and csrc/cubify.hip from this header") from e
assert not set(EXTENSION_CONSTANTS) & (set(CONSTANTS) | set(globals())), sorted(set(EXTENSION_CONSTANTS) & (set(CONSTANTS) | set(globals())))
globals().update(EXTENSION_CONSTANTS)  # SAMPLE_PDF_ROWS, SAMPLE_PDF_LDS_FLOATS, CUBIFY_BLOCK, CUBIFY_ITEMS, CUBIFY_CARRY_BLOCK

# every `#define P3D_<NAME> <integer>` of the header as <NAME>: ABI_VERSION, MAX_K, OK, ERR_*, the flags (RASTER_*, BWD_*, ...) and the
# launch constants the wrappers and tests size their inputs by (KNN_TILE, BOX3D_MAX_GROUPS, ...)
assert not set(CONSTANTS) & set(globals()), sorted(set(CONSTANTS) & set(globals()))
globals().update(CONSTANTS)
# lanes of one workgroup of csrc/graph_conv.hip (256 / lanes_per_row vertices per round).  The one constant written by hand: the kernel
# spells it as the literal of its launch bounds and launches, so there is no macro to read
NEIGHBOR_SUM_GROUP_LANES = 256

_SIGNATURES = {name: ctypes_signature(*decl) for name, decl in DECLARATIONS.items()}  # name: (restype, [argtypes])
EXPORTED_SYMBOLS = tuple(_SIGNATURES)
_EXTENSION_SIGNATURES = {name: ctypes_signature(*decl) for name, decl in EXTENSION_DECLARATIONS.items()}
EXTENSION_SYMBOLS = tuple(_EXTENSION_SIGNATURES)

# the torch dtypes a tensor may have where the header declares a pointer to this element type (None: any)
_ELEMENTS = {"float": (torch.float32,), "double": (torch.float64,), "int64_t": (torch.int64,), "int32_t": (torch.int32,),
             "uint8_t": (torch.uint8, torch.bool), "void": None}
_HOST = torch.device("cpu")


def _pointer(entry, pos, ctype):
    """Converter of a `T*` parameter: None and an empty tensor are null, an int is an address as it stands, any other tensor its
    data_ptr() after its dtype was checked against T and its device against the call's (None: the host)."""
    element = ctype[len("const "):-1] if ctype.startswith("const ") else ctype[:-1]
    if element not in _ELEMENTS:
        raise ValueError(f"{entry}: no torch dtype for the elements of `{ctype}`")
    dtypes = _ELEMENTS[element]

    def convert(t, device):
        if t is None or t.__class__ is int:
            return t
        if t.numel() == 0:
            return None
        if (dtypes is not None and t.dtype not in dtypes) or t.device != (device or _HOST):
            raise RuntimeError(f"{entry}: argument {pos} is declared `{ctype}` and the call is for {device or 'the host'}; "
                               f"got a {t.dtype} tensor on {t.device}")
        return t.data_ptr()

    return convert


def _array(entry, pos, ctype):
    """Converter of a `const T x[n]` parameter: a sequence of n numbers becomes the ctypes array."""
    base, n = re.fullmatch(r"(?:const )?(\w+)\[(\d+)\]", ctype).groups()
    n, kind = int(n), _SCALARS[base] * int(n)

    def convert(seq, device):
        if len(seq) != n:
            raise ValueError(f"{entry}: argument {pos} is declared `{ctype}`; got {len(seq)} numbers")
        return kind(*seq)

    return convert


def marshaller(entry, ret, params):
    """(converters, takes a stream, returns a status) of a parsed declaration.  converters: one per parameter in header order without
    the stream -- which is the last parameter or absent --, None where the argument goes to ctypes as it is (the scalars).  The entries
    that return a status are the int ones that take a stream or a pointer."""
    stream = params[-1:] == ["p3d_stream_t"]
    taken = params[:-1] if stream else params
    if "p3d_stream_t" in taken:
        raise ValueError(f"{entry}: the p3d_stream_t must be the last parameter and occur once")
    converters = tuple(_array(entry, i, p) if p.endswith("]") else _pointer(entry, i, p) if p.endswith("*") else None
                       for i, p in enumerate(taken))
    return converters, stream, ret == "int" and (stream or any(c is not None for c in converters))


def bind(fn, entry, ret, params):
    """invoke(where, device, *args) for call(): marshals args by the declaration, calls fn (with torch's current stream of `device`
    behind them where the entry takes one, under the device's guard) and hands the code it returns to check(code, where)."""
    converters, stream, _ = marshaller(entry, ret, params)
    count = len(converters)
    device_guard, current_stream = torch.cuda.device, torch.cuda.current_stream

    def invoke(where, device, *args):
        if len(args) != count:
            raise TypeError(f"{entry} takes {count} arguments ({', '.join(params[:count])}), got {len(args)}")
        cargs = [a if c is None else c(a, device) for c, a in zip(converters, args)]
        if stream:
            with device_guard(device):
                code = fn(*cargs, current_stream(device).cuda_stream)
        else:
            code = fn(*cargs)
        if code:
            check(code, where)

    return invoke


_lock = threading.Lock()
_lib = None
_CALLS = {}  # status entry: its invoke, bound when load() installs the signatures
_EXTENSION_CALLS = {}  # the same for the entries of the extension header


def load():
    """Load libp3d_amd.so; raise loudly when it is absent (there is no CPU or eager fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ExtensionMissing(
                f"{LIB_PATH} not found: the HIP extension is not built. Run `python -m pytorch3d_amd.build` "
                "(hipcc --offload-arch=gfx950). pytorch3d_amd has no CPU/eager fallback.")
        try:
            lib = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # e.g. libamdhip64 missing
            raise ExtensionMissing(f"cannot load {LIB_PATH}: {e}") from e
        # the version first: a library of another ABI may lack symbols of this one (or keep removed ones)
        lib.p3d_abi_version.restype, lib.p3d_abi_version.argtypes = c_int, []
        if lib.p3d_abi_version() != ABI_VERSION:
            raise ExtensionMissing(f"{LIB_PATH}: ABI version {lib.p3d_abi_version()} != {ABI_VERSION}; rebuild")
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is missing: fail loudly
            fn.restype = res
            fn.argtypes = args
            if marshaller(name, *DECLARATIONS[name])[2]:
                _CALLS[name] = bind(fn, name, *DECLARATIONS[name])
        for name, (res, args) in _EXTENSION_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
            if marshaller(name, *EXTENSION_DECLARATIONS[name])[2]:
                _EXTENSION_CALLS[name] = bind(fn, name, *EXTENSION_DECLARATIONS[name])
        _lib = lib
    return _lib


def call(entry, where, device, *args):
    """Call a status entry of the library: args are its parameters in header order without the stream, tensors (or None) where it
    declares pointers, sequences where it declares arrays.  device: the torch.device of the tensors and of the launch; None for the
    host entry.  Raises like check(code, where) on a status other than P3D_OK."""
    if _lib is None:
        load()
    (_CALLS.get(entry) or _EXTENSION_CALLS[entry])(where, device, *args)


def check(code, where):
    if code != 0:
        msg = load().p3d_error_string(code).decode()
        raise RuntimeError(f"{where}: {msg} (p3d error {code})")


def profile_snapshot():
    """{kernel name: (launches, total_ms)} since the last reset; synchronises the recorded events."""
    lib = load()
    lib.p3d_profile_collect()
    out = {}
    for i in range(lib.p3d_profile_num_entries()):
        n = c_i64(0)
        ms = ctypes.c_double(0.0)
        name = lib.p3d_profile_entry(i, ctypes.byref(n), ctypes.byref(ms))
        if name is not None and n.value > 0:
            out[name.decode()] = (n.value, ms.value)
    return out
