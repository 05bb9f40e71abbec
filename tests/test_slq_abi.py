"""CPU: the Lanczos quadrature entry points are declared in the header, exported by the library and bound with the
declared argument counts; bad arguments are refused with XK_ERR_ARG / XK_ERR_UNSUPPORTED before any launch (no device
is touched: every refusal below is decided on the host)."""
import ctypes
import re
import pytest
from xitorch_amd import _capi

SFX = ("f64", "f32", "c128", "c64")
NAMES = ["xk_slq_state_len", "xk_slq_quad"] + ["xk_slq_%s_%s" % (k, s) for k in ("init", "step") for s in SFX]
XK_ERR_ARG, XK_ERR_UNSUPPORTED = -1, -2


def test_symbols_declared_and_exported():
    declared = _capi.header_symbols()
    L = _capi.lib()
    for n in NAMES:
        assert n in declared and hasattr(L, n), n
    assert [n for n in declared if n.startswith("xk_slq_")] == sorted(NAMES)


def test_argument_counts_match_the_header():
    txt = re.sub(r"/\*.*?\*/", "", open(_capi.HEADER_PATH).read(), flags=re.S)
    L = _capi.lib()
    for n in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % n, txt)
        args = m.group(1).strip()
        nargs = 0 if args == "void" else len(args.split(","))
        assert len(getattr(L, n).argtypes) == nargs, n


def test_state_len_and_constants():
    from tests import slq_ref as sref
    from xitorch_amd import kernels as K
    from xitorch_amd.linalg import host_slq
    assert _capi.fn("xk_slq_state_len")() == sref.NST
    assert K.SLQ_FN == sref.FN_CODES and tuple(K.SLQ_FN) == host_slq.FN_NAMES
    assert K.SLQ_MAX_STEPS == sref.MAX_STEPS == host_slq.MAX_STEPS
    assert host_slq.BREAK == sref.BREAK


def _buffers():
    raw = (ctypes.c_double * 8192)()
    base = (ctypes.addressof(raw) + 63) // 64 * 64
    v = [ctypes.c_void_p(base + 4096 * i) for i in range(6)]          # 16 B aligned, disjoint
    P = [ctypes.c_void_p(base + 4096 * 6 + 1024 * i) for i in range(8)]
    return raw, v, P


@pytest.mark.parametrize("sfx", SFX)
def test_refusals(sfx):
    init, step = (_capi.fn("xk_slq_%s_%s" % (k, sfx)) for k in ("init", "step"))
    raw, v, P = _buffers()
    st, Tal, Tbe = P[5], P[6], P[7]
    null = ctypes.c_void_p(0)
    off = lambda p: ctypes.c_void_p(p.value + 8)
    ok = dict(S=1, N=40, ld=40, nblk=1, k=0)

    def c_init(z=v[0], r2=v[1], Pb=P[0], state=st, **kw):
        a = dict(ok, **kw)
        return init(z, r2, Pb, state, a["S"], a["N"], a["ld"], a["nblk"], a["k"], null)

    def c_step(W=v[0], r2=v[1], r1=v[2], Pa=P[0], Pin=P[1], Pout=P[2], state=st, Tal=Tal, Tbe=Tbe, nsteps=8, **kw):
        a = dict(ok, **kw)
        return step(W, r2, r1, Pa, Pin, Pout, state, Tal, Tbe, a["S"], a["N"], a["ld"], a["nblk"], nsteps, a["k"], null)

    for call in (c_init, c_step):
        assert call(N=0) == XK_ERR_ARG and call(N=-3) == XK_ERR_ARG
        assert call(nblk=65) == XK_ERR_ARG and call(nblk=0) == XK_ERR_ARG
        assert call(ld=39) == XK_ERR_ARG                                # below N rounded up to the 16 B vector
        if sfx != "c128":                                               # (one complex128 element is a whole vector)
            assert call(N=39, ld=39) in (XK_ERR_ARG, XK_ERR_UNSUPPORTED)    # ld < npad = 40
        assert call(k=-1) == XK_ERR_ARG and call(S=-1) == XK_ERR_ARG
        assert call(S=0) == 0                                           # nothing to do, nothing launched
    assert c_init(z=off(v[0])) == XK_ERR_UNSUPPORTED and c_init(r2=off(v[1])) == XK_ERR_UNSUPPORTED
    assert c_step(W=off(v[0])) == XK_ERR_UNSUPPORTED and c_step(r2=off(v[1])) == XK_ERR_UNSUPPORTED
    assert c_step(r1=off(v[2])) == XK_ERR_UNSUPPORTED
    if sfx == "f32":
        assert c_init(N=40, ld=42) == XK_ERR_UNSUPPORTED                # a pitch that is not a multiple of 16 B
        assert c_step(N=40, ld=42) == XK_ERR_UNSUPPORTED
    assert c_init(z=null) == XK_ERR_ARG and c_init(Pb=null) == XK_ERR_ARG and c_init(state=null) == XK_ERR_ARG
    assert c_init(r2=v[0]) == XK_ERR_ARG                                # aliased
    for name in ("W", "r2", "r1", "Pa", "Pin", "Pout", "state", "Tal", "Tbe"):
        assert c_step(**{name: null}) == XK_ERR_ARG, name
    assert c_step(r1=v[1]) == XK_ERR_ARG and c_step(r1=v[0]) == XK_ERR_ARG and c_step(r2=v[0]) == XK_ERR_ARG
    assert c_step(Pout=P[1]) == XK_ERR_ARG and c_step(Pout=P[0]) == XK_ERR_ARG and c_step(Tbe=Tal) == XK_ERR_ARG
    assert c_step(nsteps=0) == XK_ERR_ARG and c_step(nsteps=129) == XK_ERR_ARG
    assert c_step(nsteps=128, S=0) == 0
    if sfx in ("c128", "c64"):                                          # 2 N real elements no longer fit the kernels' int
        big = 1 << 30
        assert c_init(N=big, ld=big) == XK_ERR_ARG and c_step(N=big, ld=big) == XK_ERR_ARG
    else:
        assert c_init(N=(1 << 31) - 1, ld=1 << 31) == XK_ERR_ARG       # rounds up to 2^31 elements


def test_quad_refusals():
    quad = _capi.fn("xk_slq_quad")
    raw, v, P = _buffers()
    null = ctypes.c_void_p(0)
    names = ("Tal", "Tbe", "state", "theta", "weight", "out", "flag")
    good = dict(zip(names, (v[0], v[1], v[2], v[3], v[4], P[0], P[1])))

    def c_quad(S=1, nsteps=8, k=0, fn=0, **kw):
        a = dict(good, **kw)
        return quad(*(a[n] for n in names), S, nsteps, k, fn, 1.0, null)

    assert c_quad(S=-1) == XK_ERR_ARG and c_quad(k=-1) == XK_ERR_ARG
    assert c_quad(nsteps=0) == XK_ERR_ARG and c_quad(nsteps=129) == XK_ERR_ARG
    assert c_quad(fn=-1) == XK_ERR_ARG and c_quad(fn=6) == XK_ERR_ARG
    for n in names:
        assert c_quad(**{n: null}) == XK_ERR_ARG, n
    assert c_quad(weight=v[3]) == XK_ERR_ARG and c_quad(theta=v[0]) == XK_ERR_ARG and c_quad(Tbe=v[0]) == XK_ERR_ARG
    assert c_quad(S=0) == 0 and c_quad(S=0, nsteps=128, fn=5) == 0
