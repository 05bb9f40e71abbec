"""CPU: the complex Hermitian Davidson entry points are declared in the header and typed in the ctypes binding, and the
binding asks for ABI version 2 (the version that added them)."""
import os
import re
from xitorch_amd import _capi

ENTRY_POINTS = ["xk_herm_eigh", "xk_herm_ritz", "xk_herm_cholqr"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Fn:
    restype = None
    argtypes = None


class _FakeLib:
    """stands in for the loaded library: every declared symbol exists, `_declare` types it"""

    def __init__(self, names):
        for n in names:
            setattr(self, n, _Fn())


def test_abi_version_is_2():
    assert _capi.ABI_VERSION == 2
    src = open(os.path.join(ROOT, "xitorch_amd", "csrc", "xk_api.hip")).read()
    assert re.search(r"xk_abi_version\(void\)\s*\{\s*return 2;\s*\}", src)


def test_header_declares_complex_entry_points():
    syms = set(_capi.header_symbols())
    for base in ENTRY_POINTS:
        for sfx in ("c128", "c64"):
            assert base + "_" + sfx in syms
    assert "xk_herm_eigh_workspace_elems" in syms and "xk_herm_eigh_lds_bytes" in syms


def test_binding_declares_argtypes_for_every_entry_point():
    names = _capi.header_symbols()
    L = _FakeLib(names)
    _capi._declare(L)
    for base in ENTRY_POINTS:
        for sfx in ("c128", "c64"):
            f = getattr(L, base + "_" + sfx)
            assert f.argtypes is not None and f.restype is not None, base + "_" + sfx
    # arity agrees with the header's prototype
    txt = open(_capi.HEADER_PATH).read()
    for base in ENTRY_POINTS:
        name = base + "_c128"
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
        assert len(getattr(L, name).argtypes) == len(proto.split(",")), name
