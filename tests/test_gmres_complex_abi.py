"""The ten entry points of the complex GMRES (xk_gmres_c.hip): declared in include/xitorch_amd.h, exported by the built
library, registered in _capi.py with argument types, and XK_OK on an empty problem (S == 0: nothing is launched, so no
device is needed).  The change is additive: the ABI version stays 2."""
import ctypes
import pytest
from xitorch_amd import _capi

NAMES = ["xk_%s_%s" % (k, s) for k in ("gmres_gram", "lincomb", "gmres_step", "gmres_finish", "gmres_solve")
         for s in ("c128", "c64")]


def test_ten_symbols():
    assert len(NAMES) == 10


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_registered(name):
    assert name in _capi.header_symbols()
    L = _capi.lib()
    assert hasattr(L, name)
    f = getattr(L, name)
    assert f.restype is ctypes.c_int and f.argtypes and f.argtypes[-1] is ctypes.c_void_p


@pytest.mark.parametrize("name", NAMES)
def test_empty_problem_is_ok(name):
    f = _capi.fn(name)
    zero = {ctypes.c_void_p: None, ctypes.c_int: 0, ctypes.c_long: 0, ctypes.c_double: 0.0}
    args = [zero[t] for t in f.argtypes]
    if "step" in name or "solve" in name:
        # cap > 0 is an argument error whatever S is: (k, cap) / (kd, cap)
        ints = [i for i, t in enumerate(f.argtypes) if t is ctypes.c_int]
        args[ints[1] if "step" in name else ints[2]] = 1
    assert f(*args) == 0


def test_abi_version_unchanged():
    assert _capi.ABI_VERSION == 2 and int(_capi.lib().xk_abi_version()) == 2
