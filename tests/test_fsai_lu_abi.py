"""CPU: the unsymmetric-FSAI build entry points are declared in the header, exported by the library and bound with the
declared argument counts; bad arguments are refused with XK_ERR_ARG before any launch (no device is touched: every
refusal below is decided on the host)."""
import ctypes
import re
import pytest
from xitorch_amd import _capi

SFX = ("f64", "f32", "c128", "c64")
NAMES = ["xk_fsai_lu_max_row"] + ["xk_fsai_lu_build_" + s for s in SFX]
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
    assert len(_capi.lib().xk_fsai_lu_build_f64.argtypes) == 15


def test_max_row():
    assert _capi.fn("xk_fsai_lu_max_row")() == 32


@pytest.mark.parametrize("sfx", SFX)
def test_build_refusals(sfx):
    f = _capi.fn("xk_fsai_lu_build_" + sfx)
    esize = {"f64": 8, "f32": 4, "c128": 16, "c64": 8}[sfx]
    buf = (ctypes.c_double * 8192)()                          # host memory: never dereferenced by a refused call
    base = ctypes.cast(buf, ctypes.c_void_p).value
    at = lambda nbytes: ctypes.c_void_p(base + nbytes)
    null = ctypes.c_void_p(0)
    ints = (ctypes.c_int * 256)()
    ip = ctypes.cast(ints, ctypes.c_void_p)
    # A: 40 entries per member at the start of the buffer; G_L: 10 per member from byte 16384, W: 10 from byte 32768
    LOFF, WOFF = 16384, 32768
    ok = dict(a_ptr=ip, a_idx=ip, a_val=at(0), sV=40, a_nnz=40, g_ptr=ip, g_idx=ip, gl_val=at(LOFF), w_val=at(WOFF),
              sG=10, g_nnz=10, nfail=ip, N=10, B=2)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["a_ptr"], a["a_idx"], a["a_val"], a["sV"], a["a_nnz"], a["g_ptr"], a["g_idx"], a["gl_val"],
                 a["w_val"], a["sG"], a["g_nnz"], a["nfail"], a["N"], a["B"], null)

    for name in ("a_ptr", "a_idx", "a_val", "g_ptr", "g_idx", "gl_val", "w_val", "nfail"):
        assert call(**{name: null}) == XK_ERR_ARG, name
    assert call(N=0) == XK_ERR_ARG and call(N=-3) == XK_ERR_ARG
    assert call(B=0) == XK_ERR_ARG and call(B=-1) == XK_ERR_ARG
    assert call(sV=-1) == XK_ERR_ARG and call(sG=-1) == XK_ERR_ARG
    assert call(a_nnz=-1) == XK_ERR_ARG
    assert call(g_nnz=9) == XK_ERR_ARG                        # fewer entries than rows: a row without its diagonal
    assert call(sG=9) == XK_ERR_ARG and call(sG=0) == XK_ERR_ARG      # members of a factor overlap
    assert call(sV=39) == XK_ERR_ARG                          # members of A overlap (sV = 0, the broadcast, is legal)
    # either output overlapping a_val: the same array, starting inside A's last member, A starting inside the output
    for out, off in (("gl_val", LOFF), ("w_val", WOFF)):
        assert call(**{out: at(0)}) == XK_ERR_ARG, out
        assert call(**{out: at(esize * 79)}) == XK_ERR_ARG, out
        assert call(a_val=at(off + esize * 19)) == XK_ERR_ARG, out
        assert call(**{out: at(0)}, sV=0, B=1) == XK_ERR_ARG, out
    # the two outputs overlapping each other: the same array, W starting inside G_L's last member and the reverse
    assert call(w_val=at(LOFF)) == XK_ERR_ARG
    assert call(w_val=at(LOFF + esize * 19)) == XK_ERR_ARG
    assert call(gl_val=at(WOFF + esize * 19)) == XK_ERR_ARG
