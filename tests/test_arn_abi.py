"""CPU: the Krylov-Schur Arnoldi entry points are declared in the header, exported by the library and bound with the
declared argument counts; bad arguments are refused with XK_ERR_ARG before any launch (no device is touched: every
refusal below is decided on the host)."""
import ctypes
import re
from xitorch_amd import _capi
from xitorch_amd.linalg import host_eig

NAMES = ["xk_arn_max_rows", "xk_arn_status_words", "xk_arn_finish", "xk_arn_schur"]
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


def test_constants():
    rows = _capi.fn("xk_arn_max_rows")()
    assert rows >= 48 and rows == host_eig.ARN_MAX_NCV
    assert rows <= _capi.fn("xk_gkl_max_rows")()                       # the sweeps read every basis row of a cycle
    assert _capi.fn("xk_arn_status_words")() == 8


def test_finish_refusals():
    fin = _capi.fn("xk_arn_finish")
    buf = (ctypes.c_double * 8192)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    # part, Bt, nval, nchunk, coef, sC, nrm, rnrm, hcol, sHb, sHr, cplx, accumulate, dst, sdst, smax, u, brk, code, stream
    good = [p, 1, 3, 1, p, 0, p, p, p, 0, 4, 0, 0, null, 0, null, 0.0, null, 0, null]

    def call(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return fin(*a)

    assert call(_0=null) == XK_ERR_ARG and call(_1=0) == XK_ERR_ARG and call(_2=0) == XK_ERR_ARG
    assert call(_3=0) == XK_ERR_ARG and call(_2=200) == XK_ERR_ARG
    assert call(_6=null) == XK_ERR_ARG and call(_7=null) == XK_ERR_ARG
    assert call(_16=-1.0) == XK_ERR_ARG and call(_5=-1) == XK_ERR_ARG and call(_14=-1) == XK_ERR_ARG
    assert call(_11=2) == XK_ERR_ARG and call(_12=2) == XK_ERR_ARG     # cplx / accumulate are 0 or 1
    assert call(_11=1, _2=4) == XK_ERR_ARG                            # complex: re, im pairs and the sum of squares
    assert call(_10=0) == XK_ERR_ARG and call(_11=1, _10=1) == XK_ERR_ARG       # a row stride below one entry
    assert call(_1=2, _9=4, _5=2) == XK_ERR_ARG                       # members of the column overlap
    assert call(_1=2, _9=8, _5=1) == XK_ERR_ARG                       # members of coef overlap


def test_schur_refusals():
    schur = _capi.fn("xk_arn_schur")
    buf = (ctypes.c_double * 8192)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.c_void_p(p.value + 4096 * 8)
    null = ctypes.c_void_p(0)
    # H, Bt, m, neig, keep, keep_add, which, cplx, tol, u, brk, theta, Y, res, Q, Hnext, status, stream
    good = [p, 1, 8, 2, 5, null, 0, 0, 1e-6, 1e-16, null, q, q, q, q, q, q, null]

    def call(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return schur(*a)

    assert call(_1=0) == XK_ERR_ARG and call(_1=70000) == XK_ERR_ARG
    assert call(_2=1) == XK_ERR_ARG and call(_2=_capi.fn("xk_arn_max_rows")() + 1) == XK_ERR_ARG
    assert call(_3=0) == XK_ERR_ARG and call(_3=6) == XK_ERR_ARG       # neig outside [1, keep]
    assert call(_4=8) == XK_ERR_ARG                                    # keep beyond m - 1
    assert call(_6=-1) == XK_ERR_ARG and call(_6=5) == XK_ERR_ARG
    assert call(_6=3) == XK_ERR_ARG and call(_6=4) == XK_ERR_ARG       # LI / SI on a real matrix
    assert call(_7=2) == XK_ERR_ARG
    assert call(_8=-1.0) == XK_ERR_ARG and call(_9=-1.0) == XK_ERR_ARG
    for i in (0, 11, 12, 13, 14, 15, 16):
        assert call(**{"_%d" % i: null}) == XK_ERR_ARG, i
    assert call(_15=p) == XK_ERR_ARG                                   # Hnext must not be H
