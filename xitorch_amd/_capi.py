"""ctypes binding of libxitorch_amd.so — the C ABI declared in include/xitorch_amd.h.

The product path has NO fallback: if the HIP library is missing or a call
returns non-zero this raises.  PyTorch is only used for device memory and the
current HIP stream (`torch.cuda.current_stream().cuda_stream`).
"""
import ctypes
import os
import re
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# (XITORCH_AMD_LIB: a measurement build of the same ABI — trial kernels are compared against the shipped library this way)
LIB_PATH = os.environ.get("XITORCH_AMD_LIB") or os.path.join(_HERE, "csrc", "libxitorch_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "xitorch_amd.h")

_lib = None
ABI_VERSION = 2          # xk_abi_version() of the library this package was written against

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_long = ctypes.c_long
c_double = ctypes.c_double


class NativeLibraryError(RuntimeError):
    pass


def lib():
    """Load (once) and return the native library; raise loudly if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                "xitorch_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU/eager fallback." % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        if os.environ.get("XITORCH_AMD_LIB"):
            # a measurement build stands in for the shipped library: say so, and refuse one of another ABI
            # (version entry point + every function the header declares)
            import warnings
            if not hasattr(L, "xk_abi_version") or int(L.xk_abi_version()) != ABI_VERSION:
                raise NativeLibraryError("xitorch_amd: XITORCH_AMD_LIB=%s does not report ABI version %d"
                                         % (LIB_PATH, ABI_VERSION))
            missing = [n for n in header_symbols() if not hasattr(L, n)]
            if missing:
                raise NativeLibraryError("xitorch_amd: XITORCH_AMD_LIB=%s lacks %d of the declared entry points (%s ...)"
                                         % (LIB_PATH, len(missing), ", ".join(missing[:3])))
            warnings.warn("xitorch_amd: native library overridden by XITORCH_AMD_LIB=%s (measurement build)" % LIB_PATH)
        _lib = L
        _declare(_lib)
    return _lib


_SCALARS = {"int": c_int, "unsigned": c_int, "unsigned int": c_int, "long": c_long, "double": c_double}
_PROTOTYPE = re.compile(r"\b(int|long)\s+(xk_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")
_signatures = None


def _param_type(func, param):
    if "*" in param:
        return c_void_p
    words = [w for w in param.split() if w != "const"]
    if len(words) > 1 and words[-1] not in _SCALARS:
        words.pop()                                   # the parameter's name
    try:
        return _SCALARS[" ".join(words)]
    except KeyError:
        raise NativeLibraryError("xitorch_amd: %s: parameter '%s' has no ctypes mapping (pointers, int, unsigned, "
                                 "long and double cross the C ABI)" % (func, param)) from None


def parse_prototypes(text):
    """{name: (restype, [argtypes])} of every `int|long xk_name(params);` in the header text `text`.  Comments and
    preprocessor lines are dropped first; a parameter is a pointer (anything with a `*`) -> c_void_p, `int` /
    `unsigned` / `unsigned int` -> c_int, `long` -> c_long, `double` -> c_double, `(void)` -> no arguments.  Any other
    spelling raises, and so does an `xk_name(` that is not part of a prototype of that shape: nothing goes unbound."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    sigs = {}
    for ret, name, params in _PROTOTYPE.findall(text):
        params = " ".join(params.split())
        args = [] if params == "void" else [_param_type(name, p.strip()) for p in params.split(",")]
        sigs[name] = (_SCALARS[ret], args)
    unparsed = sorted(set(re.findall(r"\b(xk_[a-z0-9_]+)\s*\(", text)) - set(sigs))
    if unparsed:
        raise NativeLibraryError("xitorch_amd: no prototype of the form `int|long xk_name(params);` understood for %s"
                                 % ", ".join(unparsed))
    return sigs


def signatures():
    """The prototypes of include/xitorch_amd.h (parsed once per process): the one place the bindings come from."""
    global _signatures
    if _signatures is None:
        with open(HEADER_PATH) as f:
            _signatures = parse_prototypes(f.read())
    return _signatures


def header_symbols():
    """All function names declared in include/xitorch_amd.h (used by the CPU tests)."""
    return sorted(signatures())


def _declare(L):
    for name, (res, args) in signatures().items():
        f = getattr(L, name, None)
        if f is None:
            continue  # reported by the symbol test, and by fn() at call time
        f.restype = res
        f.argtypes = args


def check(rc, what):
    if rc != 0:
        raise NativeLibraryError("xitorch_amd native call %s failed with code %d" % (what, rc))


def stream_ptr():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    if t is None:
        return c_void_p(0)
    return c_void_p(t.data_ptr())


_SUFFIX = {torch.float64: "f64", torch.float32: "f32", torch.complex128: "c128", torch.complex64: "c64"}


def suffix(dtype):
    try:
        return _SUFFIX[dtype]
    except KeyError:
        raise NativeLibraryError("xitorch_amd native kernels support float64/float32, got %s" % dtype) from None


def require_device(t, what="tensor"):
    if not t.is_cuda:
        raise NativeLibraryError(
            "xitorch_amd: %s must live on a HIP device (got %s); the native path has no CPU fallback"
            % (what, t.device))


def fn(name):
    L = lib()
    if not hasattr(L, name):
        raise NativeLibraryError("xitorch_amd: symbol %s missing from %s" % (name, LIB_PATH))
    return getattr(L, name)


def call(base, dtype, *args, raw=False, what=None):
    """The one way from Python into a stream-ordered entry point: `base` + "_" + the suffix of `dtype` (None: an
    entry point without a type suffix) is called with `args` -- explicit `ptr(...)`, int and float values, converted by
    the header's argtypes -- and the current HIP stream last.  A non-zero code raises through `check`, naming `base`
    (or `what`); raw=True returns the code instead (the tests of the argument checks)."""
    rc = fn(base if dtype is None else base + "_" + suffix(dtype))(*args, stream_ptr())
    if raw:
        return rc
    check(rc, what or base)
