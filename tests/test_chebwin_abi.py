"""CPU: the Clenshaw-step entry points are declared in the header, exported by the library and bound FROM the header
(argument types derived by the parser, nothing typed by hand); bad arguments are refused with XK_ERR_ARG before any
launch (no device is touched: every refusal below is decided on the host, the pointers are host memory that is never
dereferenced)."""
import ctypes
import inspect
import re
import pytest
from xitorch_amd import _capi, kernels

SFX = ("f64", "f32", "c128", "c64")
NAMES = ["xk_cheb_clenshaw_" + s for s in SFX]
XK_ERR_ARG = -1


def test_symbols_declared_and_exported():
    declared = _capi.header_symbols()
    L = _capi.lib()
    for n in NAMES:
        assert n in declared and hasattr(L, n), n


def test_bound_from_the_header():
    txt = re.sub(r"/\*.*?\*/", "", open(_capi.HEADER_PATH).read(), flags=re.S)
    L = _capi.lib()
    P, I, G = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    want = [P, G, G] * 5 + [P, I, I, I, P]               # five panels (pointer, pitch, stride), coef, Bt, p, N, stream
    for n in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % n, txt)
        assert len(m.group(1).split(",")) == 20
        res, args = _capi.signatures()[n]
        assert res is I and args == want, n
        assert getattr(L, n).argtypes == want and getattr(L, n).restype is I, n
    # no hand-written argtypes for them anywhere in the binding layer
    for mod in (_capi, kernels):
        assert not re.search(r"xk_cheb_clenshaw\w*\W+argtypes", inspect.getsource(mod))
    assert "call(\"xk_cheb_clenshaw\"" in inspect.getsource(kernels.cheb_clenshaw)


def test_cheb_step_prototype_is_unchanged():
    P, I, G = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    for s in SFX:
        assert _capi.signatures()["xk_cheb_step_" + s] == (I, [P, G, G] * 4 + [P, I, I, I, P])


@pytest.mark.parametrize("sfx", SFX)
def test_refusals(sfx):
    f = _capi.fn("xk_cheb_clenshaw_" + sfx)
    esz = {"f64": 8, "f32": 4, "c128": 16, "c64": 8}[sfx]
    bufs = [(ctypes.c_char * (esz * 1024))() for _ in range(5)]        # host memory: never dereferenced by a refusal
    pa, py, pp, px, po = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
    coef = ctypes.cast((ctypes.c_double * 8)(), ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    # Bt = 2, p = 3, N = 100 at pitch 104
    ok = dict(AY=pa, ldA=104, sA=312, Y=py, ldY=104, sY=312, Yp=pp, ldP=104, sP=312, X0=px, ldX=104, sX=312, out=po,
              ldO=104, sO=312, coef=coef, Bt=2, p=3, N=100)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["AY"], a["ldA"], a["sA"], a["Y"], a["ldY"], a["sY"], a["Yp"], a["ldP"], a["sP"], a["X0"], a["ldX"],
                 a["sX"], a["out"], a["ldO"], a["sO"], a["coef"], a["Bt"], a["p"], a["N"], null)

    for name in ("AY", "Y", "Yp", "X0", "out", "coef"):
        assert call(**{name: null}) == XK_ERR_ARG, name
    for name in ("Bt", "p", "N"):
        assert call(**{name: 0}) == XK_ERR_ARG and call(**{name: -2}) == XK_ERR_ARG, name
    for name in ("ldA", "ldY", "ldP", "ldX", "ldO"):
        assert call(**{name: 99}) == XK_ERR_ARG, name                  # a pitch below N
    for name in ("sA", "sY", "sP", "sX", "sO"):
        assert call(**{name: -1}) == XK_ERR_ARG, name
    assert call(sO=2 * 104 + 99) == XK_ERR_ARG                         # rows of out overlap: stride below (p-1) ld + N
    assert call(sO=0) == XK_ERR_ARG
    # out over AY, Y or X0 (whole, or shifted by a few elements): refused; over Yprev only when it IS Yprev
    for name in ("AY", "Y", "X0"):
        assert call(out=ok[name]) == XK_ERR_ARG, name
        assert call(out=ctypes.c_void_p(ok[name].value + 8 * esz)) == XK_ERR_ARG, name
    assert call(out=ctypes.c_void_p(pp.value + 8 * esz)) == XK_ERR_ARG
    assert call(out=pp, ldO=112, sO=336) == XK_ERR_ARG                 # same pointer, another pitch
    assert call(N=0x7fffffff, ldA=1, ldY=1, ldP=1, ldX=1, ldO=1) == XK_ERR_ARG
