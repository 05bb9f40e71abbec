"""CPU: the entry points of xk_fnm.hip are declared in the header, exported by the library and bound with the declared
argument counts; bad arguments are refused with XK_ERR_ARG / XK_ERR_UNSUPPORTED before any launch (no device is touched:
every refusal below is decided on the host)."""
import ctypes
import re
import pytest
from xitorch_amd import _capi

SFX = ("f64", "f32", "c128", "c64")
NAMES = ["xk_fnm_eig", "xk_fnm_coeff"] + ["xk_fnm_step_%s" % s for s in SFX]
XK_ERR_ARG, XK_ERR_UNSUPPORTED = -1, -2


def test_symbols_declared_and_exported():
    declared = _capi.header_symbols()
    L = _capi.lib()
    for n in NAMES:
        assert n in declared and hasattr(L, n), n
    assert [n for n in declared if n.startswith("xk_fnm_")] == sorted(NAMES)


def test_argument_counts_match_the_header():
    txt = re.sub(r"/\*.*?\*/", "", open(_capi.HEADER_PATH).read(), flags=re.S)
    L = _capi.lib()
    for n in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % n, txt)
        assert len(getattr(L, n).argtypes) == len(m.group(1).split(",")), n


def test_python_layer():
    from xitorch_amd import kernels as K
    from xitorch_amd import linalg
    from xitorch_amd.linalg import host_slq, native_fnm
    assert callable(K.fnm_eig) and callable(K.fnm_coeff) and callable(K.fnm_step) and callable(native_fnm.funm)
    assert "funm_multiply" in linalg.__all__ and "expm_multiply" in linalg.__all__
    assert host_slq.calls["funm"] >= 0


def test_constants_restated_from_xk_slq_agree():
    """xk_fnm.hip restates the state layout, the step and sweep caps, the function codes and the named functions of
    xk_slq.hip (which keeps them in its own file): if the two drift, the replay and the flags break silently, so the two
    sources are compared here, entry by entry"""
    import os
    csrc = os.path.join(os.path.dirname(os.path.abspath(_capi.__file__)), "csrc")
    slq = open(os.path.join(csrc, "xk_slq.hip")).read()
    fnm = open(os.path.join(csrc, "xk_fnm.hip")).read()

    def const(src, name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))

    for a, b in (("SQ_NST", "FN_NST"), ("SQ_MAX_STEPS", "FN_MAX_STEPS"), ("SQ_QL_SWEEPS", "FN_QL_SWEEPS")):
        assert const(slq, a) == const(fnm, b), (a, b)
    assert _capi.fn("xk_slq_state_len")() == const(fnm, "FN_NST")

    def enum(src, first):
        """{name: value} of the anonymous enum whose first entry is `first`"""
        body = re.search(r"enum \{ (%s\b[^}]*)\}" % first, src).group(1)
        out, v = {}, -1
        for item in body.split(","):
            name, _, val = (x.strip() for x in item.partition("="))
            v = int(val) if val else v + 1
            out[name] = v
        return out

    st_slq, st_fnm = enum(slq, "SQ_BETA"), enum(fnm, "FN_ST_FLAG")
    assert {"FN_ST_" + k[3:]: v for k, v in st_slq.items() if "FN_ST_" + k[3:] in st_fnm} == st_fnm
    fn_slq, fn_fnm = enum(slq, "SQ_FN_LOG"), enum(fnm, "FN_LOG")
    assert {"FN_" + k[6:]: v for k, v in fn_slq.items()} == fn_fnm
    # the named functions: the same switch, case for case
    body = lambda src, name: re.sub(r"\s+", " ", re.search(r"double %s\(int fn, double param, double x\) \{(.*?)\n\}"
                                                             % name, src, flags=re.S).group(1))
    assert body(slq, "sq_fn").replace("SQ_FN_", "FN_") == body(fnm, "fnm_fn")
    # and the two step kernels form y by the same expression
    y = "y[q] = (wv[q] * c0 - c2 * r2v[q]) - c1 * y[q];"
    y0 = "y[q] = wv[q] * c0 - c2 * r2v[q];"
    for src in (slq, fnm):
        assert y in src and y0 in src
        for c in ("const T c0 = wave_uniform((T)(1.0 / beta));", "const T c2 = wave_uniform((T)(alpha / beta));",
                  "const T c1 = wave_uniform((T)(beta / oldb));"):
            assert c in src, c


def _buffers():
    raw = (ctypes.c_double * 8192)()
    base = (ctypes.addressof(raw) + 63) // 64 * 64
    v = [ctypes.c_void_p(base + 4096 * i) for i in range(6)]          # 16 B aligned, disjoint
    P = [ctypes.c_void_p(base + 4096 * 6 + 1024 * i) for i in range(8)]
    return raw, v, P


@pytest.mark.parametrize("sfx", SFX)
def test_step_refusals(sfx):
    step = _capi.fn("xk_fnm_step_%s" % sfx)
    raw, v, P = _buffers()
    null = ctypes.c_void_p(0)
    off = lambda p: ctypes.c_void_p(p.value + 8)
    names = ("W", "r2", "r1", "X", "C", "Tal", "Tbe", "state")
    good = dict(zip(names, (v[0], v[1], v[2], v[3], P[0], P[1], P[2], P[3])))

    def call(S=1, N=40, ld=40, nblk=1, nsteps=8, k=0, kstate=0, last=0, **kw):
        a = dict(good, **kw)
        return step(*(a[n] for n in names), S, N, ld, nblk, nsteps, k, kstate, last, null)

    assert call(N=0) == XK_ERR_ARG and call(N=-3) == XK_ERR_ARG
    assert call(nblk=65) == XK_ERR_ARG and call(nblk=0) == XK_ERR_ARG
    assert call(ld=39) == XK_ERR_ARG                                    # below N rounded up to the 16 B vector
    if sfx != "c128":                                                   # (one complex128 element is a whole vector)
        assert call(N=39, ld=39) in (XK_ERR_ARG, XK_ERR_UNSUPPORTED)
    assert call(k=-1) == XK_ERR_ARG and call(S=-1) == XK_ERR_ARG and call(kstate=-1) == XK_ERR_ARG
    assert call(k=8) == XK_ERR_ARG                                      # k >= nsteps
    assert call(nsteps=0) == XK_ERR_ARG and call(nsteps=129, k=3) == XK_ERR_ARG
    assert call(S=0) == 0 and call(S=0, nsteps=128, k=127, last=1) == 0     # nothing to do, nothing launched
    for n in ("W", "r2", "r1", "X"):
        assert call(**{n: off(good[n])}) == XK_ERR_UNSUPPORTED, n
    if sfx == "f32":
        assert call(N=40, ld=42) == XK_ERR_UNSUPPORTED                  # a pitch that is not a multiple of 16 B
    for n in ("r2", "X", "C", "Tal", "Tbe", "state"):
        assert call(**{n: null}) == XK_ERR_ARG, n
    assert call(r1=null) == XK_ERR_ARG                                  # r1 is needed unless this is the last step
    assert call(W=null, r1=null, S=0) == 0 and call(r1=null, last=1, S=0) == 0
    assert call(r1=v[1]) == XK_ERR_ARG and call(r1=v[0]) == XK_ERR_ARG and call(r2=v[0]) == XK_ERR_ARG
    assert call(X=v[0]) == XK_ERR_ARG and call(X=v[1]) == XK_ERR_ARG and call(X=v[2]) == XK_ERR_ARG
    assert call(Tbe=P[1]) == XK_ERR_ARG
    if sfx in ("c128", "c64"):                                          # 2 N real elements no longer fit the kernels' int
        big = 1 << 30
        assert call(N=big, ld=big) == XK_ERR_ARG
    else:
        assert call(N=(1 << 31) - 1, ld=1 << 31) == XK_ERR_ARG


def test_eig_and_coeff_refusals():
    eig, coeff = _capi.fn("xk_fnm_eig"), _capi.fn("xk_fnm_coeff")
    raw, v, P = _buffers()
    null = ctypes.c_void_p(0)
    en = ("Tal", "Tbe", "state", "theta", "Qt", "flag")
    eg = dict(zip(en, (v[0], v[1], v[2], v[3], v[4], P[0])))

    def c_eig(S=1, nsteps=8, k=0, **kw):
        a = dict(eg, **kw)
        return eig(*(a[n] for n in en), S, nsteps, k, null)

    assert c_eig(S=-1) == XK_ERR_ARG and c_eig(k=-1) == XK_ERR_ARG
    assert c_eig(nsteps=0) == XK_ERR_ARG and c_eig(nsteps=129) == XK_ERR_ARG
    for n in en:
        assert c_eig(**{n: null}) == XK_ERR_ARG, n
    assert c_eig(Tbe=v[0]) == XK_ERR_ARG and c_eig(theta=v[0]) == XK_ERR_ARG and c_eig(Qt=v[3]) == XK_ERR_ARG
    assert c_eig(S=0) == 0 and c_eig(S=0, nsteps=128) == 0

    cn = ("Qt", "theta", "state", "fvals", "C", "tail", "flag")
    cg = dict(zip(cn, (v[0], v[1], v[2], v[3], v[4], P[0], P[1])))

    def c_coeff(S=1, nsteps=8, k=0, fn=0, cplx=0, **kw):
        a = dict(cg, **kw)
        return coeff(*(a[n] for n in cn), S, nsteps, k, fn, 1.0, cplx, null)

    assert c_coeff(S=-1) == XK_ERR_ARG and c_coeff(k=-1) == XK_ERR_ARG
    assert c_coeff(nsteps=0) == XK_ERR_ARG and c_coeff(nsteps=129) == XK_ERR_ARG
    assert c_coeff(fn=-2) == XK_ERR_ARG and c_coeff(fn=6) == XK_ERR_ARG
    for n in cn:
        if n != "fvals":
            assert c_coeff(**{n: null}) == XK_ERR_ARG, n
    assert c_coeff(fn=-1, fvals=null) == XK_ERR_ARG                     # the caller's values are the function
    assert c_coeff(fn=2, fvals=null, S=0) == 0                          # a named function needs none
    assert c_coeff(C=v[0]) == XK_ERR_ARG and c_coeff(C=v[1]) == XK_ERR_ARG and c_coeff(C=v[3], fn=-1) == XK_ERR_ARG
    assert c_coeff(S=0) == 0 and c_coeff(S=0, nsteps=128, fn=-1, cplx=1) == 0
