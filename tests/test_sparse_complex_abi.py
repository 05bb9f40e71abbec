"""The complex CSR entry points (xk_csr_mm_c128 / _c64, xk_csr_sddmm_c128 / _c64) across the three places that must
agree: the header's prototypes, the ctypes declarations and the HIP source.  No GPU needed."""
import os
import re
from xitorch_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xk_csr_mm_c128", "xk_csr_mm_c64", "xk_csr_sddmm_c128", "xk_csr_sddmm_c64"]


class _Fn:
    argtypes = None
    restype = None


class _FakeLib:
    def __init__(self, names):
        for n in names:
            setattr(self, n, _Fn())


def _header():
    return re.sub(r"/\*.*?\*/", "", open(_capi.HEADER_PATH).read(), flags=re.S)


def test_header_and_binding_declare_complex_csr_entry_points():
    syms = set(_capi.header_symbols())
    assert set(NAMES) <= syms
    L = _FakeLib(sorted(syms))
    _capi._declare(L)
    txt = _header()
    for name in NAMES:
        f = getattr(L, name)
        assert f.argtypes is not None and f.restype is not None, name
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
        assert len(f.argtypes) == len(proto.split(",")), name


def test_complex_apply_has_one_more_argument_than_the_real_one():
    """int conj_val, in front of the stream; the gradient's prototype is the real one's"""
    txt = _header()
    args = lambda name: [a.strip() for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1).split(",")]
    for c, r in (("c128", "f64"), ("c64", "f32")):
        ac, ar = args("xk_csr_mm_" + c), args("xk_csr_mm_" + r)
        assert len(ac) == len(ar) + 1 and ac[-2] == "int conj_val" and ac[-1] == "void* stream"
        assert ac[:-2] == ar[:-1]
        assert args("xk_csr_sddmm_" + c) == args("xk_csr_sddmm_" + r)


def test_source_defines_the_complex_entry_points():
    src = open(os.path.join(ROOT, "xitorch_amd", "csrc", "xk_sparse.hip")).read()
    body = re.search(r"#define XK_DEFINE_SPARSE_C\(SUF, T\)(.*?)\n\n", src, flags=re.S).group(1)
    assert "xk_csr_mm_##SUF" in body and "xk_csr_sddmm_##SUF" in body and "int conj_val" in body
    assert re.search(r"^XK_DEFINE_SPARSE_C\(c128, double\)$", src, flags=re.M)
    assert re.search(r"^XK_DEFINE_SPARSE_C\(c64, float\)$", src, flags=re.M)


def test_abi_version_is_unchanged():
    assert _capi.ABI_VERSION == 2
