"""CPU: the Golub-Kahan-Lanczos entry points are declared in the header, exported by the library and bound with the
declared argument counts; bad arguments are refused with XK_ERR_ARG before any launch (no device is touched: every
refusal below is decided on the host)."""
import ctypes
import re
import pytest
from xitorch_amd import _capi

NAMES = ["xk_gkl_max_rows", "xk_gkl_bsvd_max", "xk_gkl_chunk_elems", "xk_gkl_finish", "xk_gkl_bsvd"] + \
    ["xk_gkl_sweep_" + s for s in ("f64", "f32", "c128", "c64")]
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
    assert _capi.fn("xk_gkl_max_rows")() == 64 and _capi.fn("xk_gkl_bsvd_max")() == 64
    ce = _capi.fn("xk_gkl_chunk_elems")
    assert [ce(4), ce(8), ce(16)] == [256, 128, 64] and ce(2) == XK_ERR_ARG


@pytest.mark.parametrize("sfx", ["f64", "f32", "c128", "c64"])
def test_sweep_refusals(sfx):
    f = _capi.fn("xk_gkl_sweep_" + sfx)
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.c_void_p(p.value + 2048 * 8)
    part = (ctypes.c_double * 4096)()
    pp = ctypes.cast(part, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    ok = dict(Q=q, ldQ=64, sQ=0, w=p, sW=0, dst=p, sD=0, coef=null, sC=0, scale=null, part=pp, plen=4096, Bt=1, j=2, N=64)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["Q"], a["ldQ"], a["sQ"], a["w"], a["sW"], a["dst"], a["sD"], a["coef"], a["sC"], a["scale"],
                 a["part"], a["plen"], a["Bt"], a["j"], a["N"], null)

    assert call(N=0) == XK_ERR_ARG and call(Bt=0) == XK_ERR_ARG and call(j=-1) == XK_ERR_ARG
    assert call(j=65) == XK_ERR_ARG                                    # beyond the row cap
    assert call(w=null) == XK_ERR_ARG and call(dst=null) == XK_ERR_ARG and call(part=null) == XK_ERR_ARG
    assert call(Q=null) == XK_ERR_ARG and call(ldQ=63) == XK_ERR_ARG and call(sW=-1) == XK_ERR_ARG
    assert call(plen=2) == XK_ERR_ARG                                  # partials do not fit
    assert call(dst=q) == XK_ERR_ARG                                   # dst inside the rows of Q
    assert call(dst=ctypes.c_void_p(p.value + 16)) == XK_ERR_ARG       # dst overlaps w without being w
    assert call(Bt=2, sD=8, sW=8) == XK_ERR_ARG                        # members of dst overlap


def test_finish_and_bsvd_refusals():
    fin, bsvd = _capi.fn("xk_gkl_finish"), _capi.fn("xk_gkl_bsvd")
    buf = (ctypes.c_double * 8192)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    assert fin(null, 1, 3, 1, p, 0, p, p, null, 0, null, 0.0, null, 0, null) == XK_ERR_ARG
    assert fin(p, 0, 3, 1, p, 0, p, p, null, 0, null, 0.0, null, 0, null) == XK_ERR_ARG
    assert fin(p, 1, 0, 1, p, 0, p, p, null, 0, null, 0.0, null, 0, null) == XK_ERR_ARG
    assert fin(p, 1, 200, 1, p, 0, p, p, null, 0, null, 0.0, null, 0, null) == XK_ERR_ARG
    assert fin(p, 1, 3, 1, p, 0, null, p, null, 0, null, 0.0, null, 0, null) == XK_ERR_ARG
    assert fin(p, 1, 3, 1, p, 0, p, p, null, 0, null, -1.0, null, 0, null) == XK_ERR_ARG
    good = [p, null, null, null, 1, 8, 2, 4, 1, 1e-6, p, p, p, p, p, null, null]

    def call(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return bsvd(*a)

    assert call(_5=65) == XK_ERR_ARG and call(_5=0) == XK_ERR_ARG      # order beyond the LDS cap / empty
    assert call(_6=9) == XK_ERR_ARG and call(_7=9) == XK_ERR_ARG       # k, keep beyond the order
    assert call(_0=null) == XK_ERR_ARG and call(_14=null) == XK_ERR_ARG
    assert call(_15=p) == XK_ERR_ARG                                   # Bnext must not be Bm
    assert call(_9=-1.0) == XK_ERR_ARG
