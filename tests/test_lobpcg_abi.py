"""CPU: the LOBPCG rotation entry points are declared in the header, exported by the library and bound with the declared
argument counts; bad arguments are refused with XK_ERR_ARG before any launch (no device is touched: every refusal
below is decided on the host, the pointers are host memory that is never dereferenced)."""
import ctypes
import re
import pytest
from xitorch_amd import _capi

SFX = ("f64", "f32", "c128", "c64")
NAMES = ["xk_lobpcg_max_rows", "xk_lobpcg_blocks"] + ["xk_lobpcg_rotate_" + s for s in SFX]
XK_ERR_ARG = -1


def test_symbols_declared_and_exported():
    declared = _capi.header_symbols()
    L = _capi.lib()
    for n in NAMES:
        assert n in declared and hasattr(L, n), n


def test_argument_counts_match_the_header():
    txt = re.sub(r"/\*.*?\*/", "", open(_capi.HEADER_PATH).read(), flags=re.S)
    L = _capi.lib()
    for n in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % n, txt)
        args = m.group(1).strip()
        nargs = 0 if args == "void" else len(args.split(","))
        assert len(getattr(L, n).argtypes) == nargs, n
    assert len(_capi.fn("xk_lobpcg_rotate_f64").argtypes) == 23


def test_max_rows_and_blocks():
    assert _capi.fn("xk_lobpcg_max_rows")() >= 96
    blocks = _capi.fn("xk_lobpcg_blocks")
    # chunks of 256 vectors of 16 B: a function of N and the element size only
    for esize, per in ((4, 1024), (8, 512), (16, 256)):
        for N in (1, per - 1, per, per + 1, 4099, 10 * per):
            assert blocks(N, esize) == -(-N // per), (N, esize)
    assert blocks(0, 8) == 0 and blocks(-1, 8) == 0 and blocks(100, 3) == 0


@pytest.mark.parametrize("sfx", SFX)
def test_rotate_refusals(sfx):
    f = _capi.fn("xk_lobpcg_rotate_" + sfx)
    buf = (ctypes.c_double * 64)()                            # host memory: never dereferenced by a refused call
    p = ctypes.cast(buf, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    kmax = _capi.fn("xk_lobpcg_max_rows")()
    # N = 100 at pitch 104, (k, q, w) = (9, 6, 3): stacks of 9 rows
    ok = dict(S=p, ldS=104, sS=9 * 104, AS=p, ldA=104, sA=9 * 104, MS=p, ldM=104, sM=9 * 104, C=p, sC=54, sCa=6, sCc=1,
              lam=p, sLam=3, Pnorm=p, Pmax=p, Bt=2, N=100, k=9, q=6, w=3)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["S"], a["ldS"], a["sS"], a["AS"], a["ldA"], a["sA"], a["MS"], a["ldM"], a["sM"], a["C"], a["sC"],
                 a["sCa"], a["sCc"], a["lam"], a["sLam"], a["Pnorm"], a["Pmax"], a["Bt"], a["N"], a["k"], a["q"], a["w"],
                 null)

    for name in ("S", "AS", "C", "lam", "Pnorm", "Pmax"):
        assert call(**{name: null}) == XK_ERR_ARG, name
    for name in ("Bt", "N", "w"):
        assert call(**{name: 0}) == XK_ERR_ARG and call(**{name: -2}) == XK_ERR_ARG, name
    assert call(q=2) == XK_ERR_ARG                            # q < w
    assert call(q=10) == XK_ERR_ARG                           # q > k
    assert call(k=kmax + 1, q=6) == XK_ERR_ARG
    assert call(k=kmax + 1, q=kmax + 1, w=1) == XK_ERR_ARG
    for name in ("ldS", "ldA", "ldM"):
        assert call(**{name: 99}) == XK_ERR_ARG, name         # a pitch below N
    for name in ("sS", "sA", "sM"):
        assert call(**{name: 9 * 104 - 1}) == XK_ERR_ARG, name   # a stack stride below (q + w) * pitch
        assert call(**{name: 0}) == XK_ERR_ARG, name
    assert call(sS=9 * 104 - 1, Bt=1) == XK_ERR_ARG           # (also for a single member)
    # without an overlap stack its pitch and stride are not looked at — but everything else still is
    assert call(MS=null, ldM=0, sM=0, q=2) == XK_ERR_ARG
