"""CPU: the LSMR entry points are declared in the header, exported by the library and bound with the declared argument
counts; bad arguments are refused with XK_ERR_ARG / XK_ERR_UNSUPPORTED before any launch (no device is touched: every
refusal below is decided on the host)."""
import ctypes
import re
import pytest
from xitorch_amd import _capi

SFX = ("f64", "f32", "c128", "c64")
NAMES = ["xk_lsmr_state_len"] + ["xk_lsmr_%s_%s" % (k, s) for k in ("init", "bidiag", "update") for s in SFX]
XK_ERR_ARG, XK_ERR_UNSUPPORTED = -1, -2


def test_symbols_declared_and_exported():
    declared = _capi.header_symbols()
    L = _capi.lib()
    for n in NAMES:
        assert n in declared and hasattr(L, n), n
    assert [n for n in declared if n.startswith("xk_lsmr_")] == sorted(NAMES)


def test_argument_counts_match_the_header():
    txt = re.sub(r"/\*.*?\*/", "", open(_capi.HEADER_PATH).read(), flags=re.S)
    L = _capi.lib()
    for n in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % n, txt)
        args = m.group(1).strip()
        nargs = 0 if args == "void" else len(args.split(","))
        assert len(getattr(L, n).argtypes) == nargs, n


def test_state_len():
    from tests import lsmr_ref as lref
    assert _capi.fn("xk_lsmr_state_len")() == lref.NST


@pytest.mark.parametrize("sfx", SFX)
def test_refusals(sfx):
    init, bidiag, update = (_capi.fn("xk_lsmr_%s_%s" % (k, sfx)) for k in ("init", "bidiag", "update"))
    raw = (ctypes.c_double * 8192)()
    base = (ctypes.addressof(raw) + 63) // 64 * 64
    v = [ctypes.c_void_p(base + 4096 * i) for i in range(6)]          # 16 B aligned, disjoint
    P = [ctypes.c_void_p(base + 4096 * 6 + 1024 * i) for i in range(5)]
    st = ctypes.c_void_p(base + 4096 * 8)
    null = ctypes.c_void_p(0)
    off = lambda p: ctypes.c_void_p(p.value + 8)
    ok = dict(S=1, N=40, ld=40, nblk=1, k=0)

    def c_init(b=v[0], uh=v[1], **kw):
        a = dict(ok, **kw)
        return init(b, uh, P[0], st, P[1], a["S"], a["N"], a["ld"], a["nblk"], a["k"], null)

    def c_bidiag(Op=v[0], y=v[1], Pin=P[0], Pout=P[1], half=0, nblk_in=1, **kw):
        a = dict(ok, **kw)
        return bidiag(Op, y, Pin, Pout, st, half, a["S"], a["N"], a["ld"], a["nblk"], nblk_in, a["k"], null)

    def c_update(vh=v[0], h=v[1], hbar=v[2], x=v[3], Pxin=P[2], Pxout=P[3], nblk_u=1, damp=0.0, **kw):
        a = dict(ok, **kw)
        return update(vh, h, hbar, x, P[0], P[1], Pxin, Pxout, st, P[4], a["S"], a["N"], a["ld"], a["nblk"], nblk_u,
                      a["k"], damp, 1e-6, 1e-6, 1e8, null)

    for call in (c_init, c_bidiag, c_update):
        assert call(N=0) == XK_ERR_ARG and call(N=-3) == XK_ERR_ARG
        assert call(nblk=65) == XK_ERR_ARG and call(nblk=0) == XK_ERR_ARG
        assert call(ld=39) == XK_ERR_ARG                                # below N rounded up to the 16 B vector
        if sfx != "c128":                                               # (one complex128 element is a whole vector)
            assert call(N=39, ld=39) in (XK_ERR_ARG, XK_ERR_UNSUPPORTED)    # ld < npad = 40
        assert call(k=-1) == XK_ERR_ARG and call(S=-1) == XK_ERR_ARG
        assert call(S=0) == 0                                           # nothing to do, nothing launched
    assert c_init(b=off(v[0])) == XK_ERR_UNSUPPORTED and c_init(uh=off(v[1])) == XK_ERR_UNSUPPORTED
    assert c_bidiag(Op=off(v[0])) == XK_ERR_UNSUPPORTED and c_bidiag(y=off(v[1])) == XK_ERR_UNSUPPORTED
    assert c_update(x=off(v[3])) == XK_ERR_UNSUPPORTED and c_update(h=off(v[1])) == XK_ERR_UNSUPPORTED
    if sfx in ("f32",):
        assert c_init(N=40, ld=42) == XK_ERR_UNSUPPORTED                # a pitch that is not a multiple of 16 B
    assert c_init(b=null) == XK_ERR_ARG and c_bidiag(y=null) == XK_ERR_ARG and c_update(x=null) == XK_ERR_ARG
    assert c_bidiag(nblk_in=65) == XK_ERR_ARG and c_bidiag(half=2) == XK_ERR_ARG
    assert c_bidiag(Pout=P[0]) == XK_ERR_ARG and c_bidiag(y=v[0]) == XK_ERR_ARG
    assert c_update(nblk_u=0) == XK_ERR_ARG and c_update(damp=-1.0) == XK_ERR_ARG
    assert c_update(Pxout=P[2]) == XK_ERR_ARG and c_update(hbar=v[1]) == XK_ERR_ARG
