"""-m gpu: the block-Davidson basis and chain kernels of xk_basis.hip / xk_chain.hip (lincomb, ritz_residual,
diag_precond, panel_transform, davidson_extend_t, davidson_orth, davidson_ritz) in float64 and float32 against the
float64 reference of tests/davidson_ref.py with dtype-derived bounds.

The kernels are driven through the `kernels` wrappers on views laid out as the driver lays them out: basis rows of a
(B, cap, ld) buffer (batch pitch larger than rows x pitch), pitch pad_len(N) or pad_len(N) + 8, Y as a transposed
slice of a (B, pk, k) block, lam with a row stride > P, d / m broadcast or per member.  Every case also checks the
panel contract ([N, ld) zero in and out), that nothing outside the documented output region changes (NaN-poisoned
rows / guard regions compared bitwise), exact relations (rmax against the written residual, the status folds, info),
non-finite residuals and bit-determinism."""
import json
import math
import os
import zlib
import pytest
import torch
from tests import davidson_ref as dref
from xitorch_amd import kernels as K
from xitorch_amd.linalg._panel import pad_len

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
IDS = ["f64", "f32"]
DEV = torch.device("cuda:0")
IDTYPE = {torch.float64: torch.int64, torch.float32: torch.int32}


def _bits(t):
    return t.detach().contiguous().view(IDTYPE[t.dtype])


def _assert_only_changed(before, after, allowed, what):
    """bitwise: entries outside `allowed` (bool mask of the buffer's shape) are unchanged"""
    changed = (_bits(before).cpu() != _bits(after).cpu()).reshape(allowed.shape)
    bad = changed & ~allowed
    assert not bool(bad.any()), "%s: wrote outside its region at %s" % (what, bad.nonzero()[0].tolist())


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _r(t, dtype):
    return t.to(dtype).to(torch.float64)


class _Buf:
    """a (B, cap, ld) device buffer: rows [0, rows) hold `val` (float64 host values, (B, rows, N)) rounded to the dtype
    with [N, ld) zero, rows >= rows NaN-poisoned"""

    def __init__(self, val, dtype, cap, ld):
        B, rows, N = val.shape
        h = torch.full((B, cap, ld), math.nan, dtype=dtype)
        h[:, :rows] = 0
        h[:, :rows, :N] = val.to(dtype)
        self.N, self.rows, self.ld = N, rows, ld
        self.dev = h.to(DEV)
        self.before = self.dev.clone()

    def view(self, rows=None, n=None):
        return self.dev[:, :(self.rows if rows is None else rows), :(self.N if n is None else n)]

    def host(self, rows=None):
        return dref.hp(self.dev[:, :(self.rows if rows is None else rows), :self.N])

    def pad_zero(self, what, rows=None):
        r = self.rows if rows is None else rows
        pad = self.dev[:, :r, self.N:].cpu()
        assert bool((pad == 0).all()), "%s: [N, ld) not zero" % what

    def only_changed(self, rows, what, cols=None):
        allowed = torch.zeros(self.dev.shape, dtype=torch.bool)
        allowed[:, rows[0]:rows[1], :(self.ld if cols is None else cols)] = True
        _assert_only_changed(self.before, self.dev, allowed, what)


def _guarded(n, dtype, guard=64):
    """a scratch buffer of exactly n elements followed by a NaN-poisoned guard; returns (full, view of n)"""
    full = torch.full((n + guard,), math.nan, dtype=dtype, device=DEV)
    return full, full[:n]


def _guard_ok(full, n, what):
    assert bool(torch.isnan(full[n:].cpu()).all()), "%s: scratch guard region written" % what


def _sentinel_member(B):
    return B // 2


def _values(g, dtype, B, rows, N, sentinel=False, sentinel_rows=()):
    v = dref.rand(g, B, rows, N)
    if sentinel:
        s = _sentinel_member(B)
        sub = v[s:s + 1]
        dref.add_sentinels(sub, dtype, rows=sentinel_rows, cols=dref.sentinel_columns(N, dtype))
        v[s:s + 1] = sub
    return _r(v, dtype)


def _check(got, ref, dtype, what, kernel):
    return dref.check(got, ref, dtype, what=what, kernel=kernel)


# ------------------------------------------------------------------------------------------------ shapes
def _stream_cfgs(dtype):
    """(N, k, P, B, extra pitch)"""
    vn = dref.VEC_ELEMS[dtype]
    t = 256 * vn
    return [(1, 1, 1, 1, 0), (max(vn - 1, 1), 2, 3, 3, 8), (vn + 1, 3, 8, 3, 0), (t, 7, 9, 3, 8), (t + 1, 8, 16, 3, 0),
            (5 * t + 37, 9, 17, 3, 8), (5 * t + 37, 13, 3, 65, 0), (5 * t + 37, 64, 8, 3, 0),
            (16387, 129, 9, 3, 8), (100003, 13, 17, 1, 0), (2000, 1, 17, 65, 8), (2000, 2, 1, 1, 0),
            (2000, 3, 9, 3, 0)]


STREAM = [(d, i, c) for d in DTYPES for i, c in enumerate(_stream_cfgs(d))]
STREAM_IDS = ["%s-N%d-k%d-P%d-B%d-ld+%d" % ((IDS[DTYPES.index(d)],) + c) for d, i, c in STREAM]


# ------------------------------------------------------------------------------------------------ lincomb
@pytest.mark.parametrize("dtype,i,cfg", STREAM, ids=STREAM_IDS)
def test_lincomb(dtype, i, cfg):
    N, k, P, B, extra = cfg
    g = _gen("lincomb", str(dtype), cfg)
    ld = pad_len(N) + extra
    layout = ("ac", "ca")[i % 2]
    alpha, beta = -1.0, (0.5, 0.0, 1.0)[i % 3]
    Vb = _Buf(_values(g, dtype, B, k, N, sentinel=True), dtype, k + 3, ld)
    C = dref.rand(g, B, k, P)
    s = _sentinel_member(B)
    C[s, k - 1] *= 1e3
    C[s, :, P - 1] *= 1e3
    C = _r(C, dtype)
    Cd = (C if layout == "ac" else C.transpose(1, 2)).contiguous().to(dtype).to(DEV)
    Cbefore = Cd.clone()
    outv = _values(g, dtype, B, P, N)
    Ob = _Buf(outv, dtype, P + 2, ld)
    if beta == 0.0:
        Ob.dev[:, :P, :N] = math.nan          # BLAS semantics: beta == 0 never reads Out
        Ob.before = Ob.dev.clone()
    ref = dref.lincomb(Vb.host(), C, outv, alpha, beta, dtype)
    K.lincomb(Vb.view(), Cd, Ob.view(), k, P, coef_layout=layout, alpha=alpha, beta=beta)
    first = Ob.dev.clone()
    what = "lincomb %s N=%d k=%d P=%d B=%d ld=%d %s beta=%g" % (dtype, N, k, P, B, ld, layout, beta)
    _check({"Out": Ob.host()}, ref, dtype, what, "lincomb")
    Ob.pad_zero(what)
    Ob.only_changed((0, P), what)
    Vb.only_changed((0, 0), what + " (V)")
    assert torch.equal(_bits(Cd), _bits(Cbefore)), what + ": C written"
    # bit-determinism: the same call on the same input
    Ob.dev.copy_(Ob.before)
    K.lincomb(Vb.view(), Cd, Ob.view(), k, P, coef_layout=layout, alpha=alpha, beta=beta)
    assert torch.equal(_bits(first), _bits(Ob.dev)), what + ": not bit-reproducible"


# ------------------------------------------------------------------------------------------------ ritz_residual
def _ritz_inputs(g, dtype, N, k, P, B, extra, driver_y=True):
    ld = pad_len(N) + extra
    s = _sentinel_member(B)
    Vb = _Buf(_values(g, dtype, B, k, N, sentinel=True), dtype, k + 3, ld)
    AVb = _Buf(_values(g, dtype, B, k, N, sentinel=True), dtype, k + 5, ld)
    Y = dref.rand(g, B, k, P)
    Y[s, k - 1] *= 1e3
    Y[s, :, P - 1] *= 1e3
    Y = _r(Y, dtype)
    if driver_y:                               # as the driver passes it: a transposed slice of a (B, pk, k) block
        pk = P + 3
        Ybuf = torch.full((B, pk, k), math.nan, dtype=dtype)
        Ybuf[:, :P] = Y.transpose(1, 2).to(dtype)
        Yd = Ybuf.to(DEV)[:, :P].transpose(1, 2)
    else:
        Yd = Y.to(dtype).to(DEV)
    lam = _r(dref.rand(g, B, P) * 3, dtype)
    lbuf = torch.full((B, P + 5), math.nan, dtype=dtype)
    lbuf[:, :P] = lam.to(dtype)
    lamd = lbuf.to(DEV)[:, :P]                 # row stride > P
    Xb = _Buf(torch.zeros(B, P, N, dtype=torch.float64), dtype, P + 2, ld)
    Tb = _Buf(torch.zeros(B, P, N, dtype=torch.float64), dtype, P + 3, ld)
    for b in (Xb, Tb):                         # outputs: [0, N) poisoned before the call, [N, ld) zero (contract)
        b.dev[:, :P, :N] = math.nan
        b.before = b.dev.clone()
    return ld, Vb, AVb, Y, Yd, lam, lamd, Xb, Tb


@pytest.mark.parametrize("dtype,i,cfg", STREAM, ids=STREAM_IDS)
def test_ritz_residual_and_davidson_ritz(dtype, i, cfg):
    N, k, P, B, extra = cfg
    g = _gen("ritz", str(dtype), cfg)
    ld, Vb, AVb, Y, Yd, lam, lamd, Xb, Tb = _ritz_inputs(g, dtype, N, k, P, B, extra, driver_y=(i % 2 == 0))
    ref = dref.ritz_residual(Vb.host(), AVb.host(), Y, lam, dtype)
    what = "ritz_residual %s N=%d k=%d P=%d B=%d ld=%d" % (dtype, N, k, P, B, ld)
    rmax = torch.zeros(B, dtype=dtype, device=DEV)
    K.ritz_residual(Vb.view(), AVb.view(), Yd, lamd, Xb.view(), Tb.view(), rmax, k, P)
    _check({"X": Xb.host(), "Tn": Tb.host(), "rmax": rmax}, ref, dtype, what, "ritz_residual")
    for b in (Xb, Tb):
        b.pad_zero(what)
        b.only_changed((0, P), what)
    Vb.only_changed((0, 0), what + " (V)")
    AVb.only_changed((0, 0), what + " (AV)")
    # rmax is the max of the very residual the kernel wrote (Tn = -r): bit for bit
    tmax = Tb.dev[:, :P, :N].abs().flatten(1).max(1).values
    assert torch.equal(_bits(rmax), _bits(tmax)), what + ": rmax %s != max|Tn| %s" % (rmax.tolist(), tmax.tolist())
    X1, T1, r1 = Xb.dev.clone(), Tb.dev.clone(), rmax.clone()

    # the fused chain call on the same inputs: the same X / Tn bits, and the status folds
    Xb.dev.copy_(Xb.before)
    Tb.dev.copy_(Tb.before)
    rmax.zero_()
    info = torch.randint(0, 3, (B,), dtype=torch.int32, generator=g).to(DEV)
    flag = torch.randint(0, 2, (B,), dtype=torch.int32, generator=g).to(DEV)
    cond = (torch.rand(B, generator=g, dtype=torch.float64) * 100).to(dtype).to(DEV)
    orth = torch.zeros(B, dtype=dtype, device=DEV)
    status = torch.full((5,), math.nan, dtype=torch.float64, device=DEV)
    info_h, flag_h, cond_h = info.clone(), flag.clone(), cond.clone()
    gs_full = None
    if P > 8:                                  # the guard's Gram scratch at exactly B P P elements + a poisoned guard
        gs_full, gs = _guarded(B * P * P, dtype)
        key = (dtype, Vb.dev.device, torch.cuda.current_stream().cuda_stream)
        saved = K._gs_cache.get(key)
        K._gs_cache[key] = gs
    try:
        K.davidson_ritz(Vb.view(), AVb.view(), Yd, lamd, Xb.view(), Tb.view(), rmax, info, flag, status, k, P,
                        cond=cond, orth=orth)
        torch.cuda.synchronize()
    finally:
        if gs_full is not None:
            if saved is None:
                K._gs_cache.pop(key, None)
            else:
                K._gs_cache[key] = saved
    what = "davidson_ritz %s N=%d k=%d P=%d B=%d ld=%d" % (dtype, N, k, P, B, ld)
    if gs_full is not None:
        _guard_ok(gs_full, B * P * P, what)
    assert torch.equal(_bits(Xb.dev), _bits(X1)) and torch.equal(_bits(Tb.dev), _bits(T1)), \
        what + ": X / Tn differ from ritz_residual's"
    st = status.cpu().tolist()
    assert bool((rmax == 0).all()) and bool((cond == 0).all()) and bool((orth == 0).all()), \
        what + ": rmax / cond / orth not re-zeroed"
    want = dref.status_of(r1, info_h.cpu(), flag_h.cpu(), cond_h, torch.zeros(1))
    assert st[0] == want[0] and st[1] == want[1] and st[2] == want[2] and st[3] == want[3], (what, st, want)
    # status[4] is the guard of X: a standalone ritz_guard on the same X gives the same bits
    orth2 = torch.zeros(B, dtype=dtype, device=DEV)
    K.ritz_guard(Xb.view(), orth2, P, N)
    assert st[4] == float(orth2.double().max()), (what, st[4], orth2.tolist())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("P", [3, 8, 9, 17])
@pytest.mark.parametrize("where", ["AV", "Y"])
@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_nonfinite_residual_is_reported_as_inf(dtype, P, where, bad):
    """one NaN / +inf entry in AV (or Y) of member 1 of 3: rmax[1] must be +inf (the header's contract), the other
    members finite and right, and davidson_ritz's status[0] non-finite -- also when the entry lies in the second
    column chunk (P > 8, folded through the atomic max)"""
    N, k, B = 3001, 7, 3
    g = _gen("nonfinite", str(dtype), P, where, bad)
    ld, Vb, AVb, Y, Yd, lam, lamd, Xb, Tb = _ritz_inputs(g, dtype, N, k, P, B, 8)
    val = math.nan if bad == "nan" else math.inf
    AVh = AVb.host()
    if where == "AV":
        AVb.dev[1, k - 1, 1234] = val
        AVh[1, k - 1, 1234] = val
    else:
        Yd[1, k - 1, P - 1] = val
        Y[1, k - 1, P - 1] = val
    ref = dref.ritz_residual(Vb.host(), AVh, Y, lam, dtype)
    assert ref["rmax"][0][1].item() == math.inf
    what = "ritz_residual %s P=%d %s in %s" % (dtype, P, bad, where)
    for fused in (False, True):
        rmax = torch.zeros(B, dtype=dtype, device=DEV)
        if fused:
            status = torch.zeros(3, dtype=torch.float64, device=DEV)
            info = torch.zeros(B, dtype=torch.int32, device=DEV)
            K.davidson_ritz(Vb.view(), AVb.view(), Yd, lamd, Xb.view(), Tb.view(), rmax, info, None, status, k, P)
            s0 = status[0].item()
            assert not math.isfinite(s0), what + ": davidson_ritz status[0] = %r" % s0
        else:
            K.ritz_residual(Vb.view(), AVb.view(), Yd, lamd, Xb.view(), Tb.view(), rmax, k, P)
            r = rmax.cpu().double()
            assert r[1].item() == math.inf, what + ": rmax = %r" % r.tolist()
            ok = [0, 2]
            sub = {n: (v[ok], b_[ok]) for n, (v, b_) in ref.items()}
            _check({"X": Xb.host()[ok], "Tn": Tb.host()[ok], "rmax": r[ok]}, sub, dtype, what, "ritz_residual")


# ------------------------------------------------------------------------------------------------ diag_precond
@pytest.mark.parametrize("dtype,i,cfg", STREAM, ids=STREAM_IDS)
def test_diag_precond(dtype, i, cfg):
    N, k, P, B, extra = cfg
    g = _gen("precond", str(dtype), cfg)
    ld = pad_len(N) + extra
    floor = 1e-3
    fl = dref.cast(floor, dtype)
    s = _sentinel_member(B)
    tv = _values(g, dtype, B, P, N)
    Tb = _Buf(tv, dtype, P + 2, ld)
    lam = _r(dref.rand(g, B, P), dtype)
    lbuf = torch.full((B, P + 5), math.nan, dtype=dtype)
    lbuf[:, :P] = lam.to(dtype)
    lamd = lbuf.to(DEV)[:, :P]
    d_batch = (1, B)[i % 2]
    m_mode = (None, 1, B)[i % 3]
    dbuf = _r(dref.rand(g, B, N) * 4, dtype)
    m = None if m_mode is None else _r(1 + dref.rand(g, m_mode, N).abs(), dtype)
    # exact zero and tiny denominators of both signs for member s, column 0 (m = 1 there: d - lam exact by Sterbenz)
    l0 = lam[s, 0].item()
    drow = 0 if d_batch == 1 else s
    for j, dv in enumerate((l0, l0 * (1 + 1e-5), l0 * (1 - 1e-5), l0)):
        if j < N:
            dbuf[drow, j] = dv
            if m is not None:
                m[:, j] = 1
    dbuf = _r(dbuf, dtype)
    if N > 5:
        dbuf[drow, 5] = math.nan                 # NaN passes through
    d = dbuf[:1] if d_batch == 1 else dbuf
    dd = dbuf.to(dtype).to(DEV)[:d_batch]        # broadcast d: a one-row view of a buffer whose other rows differ
    md = None if m is None else m.to(dtype).to(DEV)
    ref = dref.diag_precond(tv, d, m, lam, fl, dtype)
    what = "diag_precond %s N=%d P=%d B=%d ld=%d d(%d) m(%s)" % (dtype, N, P, B, ld, d_batch, m_mode)
    K.diag_precond(Tb.view(), dd, lamd, P, m=md, floor=floor)
    first = Tb.dev.clone()
    _check({"Tn": Tb.host()}, ref, dtype, what, "diag_precond")
    Tb.pad_zero(what)
    Tb.only_changed((0, P), what, cols=N)
    Tb.dev.copy_(Tb.before)
    K.diag_precond(Tb.view(), dd, lamd, P, m=md, floor=floor)
    assert torch.equal(_bits(first), _bits(Tb.dev)), what + ": not bit-reproducible"


# ------------------------------------------------------------------------------------------------ panel_transform
@pytest.mark.parametrize("dtype,i,cfg", STREAM, ids=STREAM_IDS)
def test_panel_transform(dtype, i, cfg):
    N, k, P, B, extra = cfg
    g = _gen("transform", str(dtype), cfg)
    ld = pad_len(N) + extra
    tv = _values(g, dtype, B, P, N, sentinel=True)
    Tb = _Buf(tv, dtype, P + 2, ld)
    W = dref.rand(g, B, P, P)
    W[_sentinel_member(B), :, P - 1] *= 1e3
    W = _r(W, dtype)                            # the lower triangle holds different values: it must not be read
    Wd = W.to(dtype).to(DEV)
    ref = dref.panel_transform(tv, W, dtype)
    what = "panel_transform %s N=%d P=%d B=%d ld=%d" % (dtype, N, P, B, ld)
    K.panel_transform(Tb.view(), Wd, P)
    _check({"Tp": Tb.host()}, ref, dtype, what, "panel_transform")
    Tb.pad_zero(what)
    Tb.only_changed((0, P), what)


# ------------------------------------------------------------------------------------------------ extend_t
def _ext_cfgs(dtype):
    """(N, k0, q, B, extra pitch)"""
    vn = dref.VEC_ELEMS[dtype]
    t = 256 * vn
    c = [(1, 0, 1, 1, 0), (vn + 1, 1, 3, 3, 8), (t + 1, 7, 8, 3, 0), (5 * t + 37, 40, 9, 3, 8), (16387, 7, 17, 3, 0),
         (2000, 0, 16, 65, 8), (100003, 1, 3, 1, 0), (t, 40, 1, 3, 0)]
    if dtype == torch.float64:
        c.append((4099, 992, 8, 1, 0))           # a large basis (un-restarted runs reach 1500 vectors)
    return c


EXT = [(d, c) for d in DTYPES for c in _ext_cfgs(d)]
EXT_IDS = ["%s-N%d-k0%d-q%d-B%d-ld+%d" % ((IDS[DTYPES.index(d)],) + c) for d, c in EXT]


@pytest.mark.parametrize("dtype,cfg", EXT, ids=EXT_IDS)
def test_davidson_extend_t(dtype, cfg):
    N, k0, q, B, extra = cfg
    g = _gen("extend", str(dtype), cfg)
    kq = k0 + q
    ld = pad_len(N) + extra
    cap = kq + 3
    Vb = _Buf(_values(g, dtype, B, kq, N, sentinel=True), dtype, cap, ld)
    av = _values(g, dtype, B, kq, N, sentinel=True, sentinel_rows=[kq - 1])
    AVb = _Buf(av, dtype, cap, ld)
    AVb.dev[:, :k0] = math.nan                   # rows < k0 of AV are not read
    AVb.before = AVb.dev.clone()
    capT = kq + 2
    Tm = torch.full((B, capT, capT + 1), math.nan, dtype=dtype, device=DEV)
    Tm0 = Tm.clone()
    full, Tn = _guarded(B * q * kq, dtype)
    ref = dref.extend_t(Vb.host(), av, k0, q, dtype)
    what = "extend_t %s N=%d k0=%d q=%d B=%d ld=%d" % (dtype, N, k0, q, B, ld)
    K.davidson_extend_t(Vb.dev, AVb.dev, Tm, Tn, N, k0, q)
    Th = dref.hp(Tm)
    got = {"Tn": dref.hp(Tn).view(B, q, kq), "Trows": Th[:, k0:kq, :kq]}
    if k0:
        got["Tcols"] = Th[:, :k0, k0:kq]
    _check(got, ref, dtype, what, "extend_t")
    _guard_ok(full, B * q * kq, what)
    allowed = torch.zeros(Tm.shape, dtype=torch.bool)
    allowed[:, k0:kq, :kq] = True
    allowed[:, :k0, k0:kq] = True
    _assert_only_changed(Tm0, Tm, allowed, what)
    Vb.only_changed((0, 0), what + " (V)")
    AVb.only_changed((0, 0), what + " (AV)")
    T1 = Tm.clone()
    Tm.copy_(Tm0)
    K.davidson_extend_t(Vb.dev, AVb.dev, Tm, Tn, N, k0, q)
    assert torch.equal(_bits(T1), _bits(Tm)), what + ": not bit-reproducible"


# ------------------------------------------------------------------------------------------------ orth
def _orth_cfgs(dtype):
    """(N, k0, q, passes, B, extra pitch)"""
    vn = dref.VEC_ELEMS[dtype]
    t = 256 * vn
    c = [(1, 0, 1, 2, 1, 0), (vn + 1, 1, 2, 2, 3, 8), (t + 1, 7, 3, 1, 3, 0), (5 * t + 37, 40, 8, 2, 3, 8),
         (5 * t + 37, 7, 9, 2, 3, 0), (2000, 1, 16, 1, 65, 0), (2000, 40, 17, 2, 3, 8), (4099, 7, 32, 2, 3, 0),
         (4099, 0, 33, 2, 3, 8), (4099, 7, 40, 1, 3, 0), (4099, 1, 64, 2, 1, 0), (16387, 0, 8, 0, 3, 0),
         (16387, 9, 8, 3, 3, 0), (100003, 1, 3, 2, 1, 0)]
    if dtype == torch.float64:
        c.append((4099, 990, 10, 2, 1, 0))        # a large basis
    return c


ORTH = [(d, c) for d in DTYPES for c in _orth_cfgs(d)]
ORTH_IDS = ["%s-N%d-k0%d-q%d-passes%d-B%d-ld+%d" % ((IDS[DTYPES.index(d)],) + c) for d, c in ORTH]


def _orth_basis(g, dtype, B, k0, q, N):
    """rows [0, k0) orthonormal; rows [k0, k0+q) a panel diag(s) Q + M V (s in [0.5, 2]: kappa <= 4 after the
    projection, M: a sizeable component in span(V) for the projection to remove)"""
    Qf, _ = torch.linalg.qr(dref.rand(g, B, N, k0 + q))
    Qf = Qf.transpose(1, 2)
    s = 0.5 + 1.5 * torch.rand(B, q, 1, generator=g, dtype=torch.float64)
    pan = s * Qf[:, k0:]
    if k0:
        pan = pan + torch.einsum("bca,ban->bcn", 0.5 * dref.rand(g, B, q, k0), Qf[:, :k0])
    return _r(torch.cat([Qf[:, :k0], pan], 1), dtype)


@pytest.mark.parametrize("dtype,cfg", ORTH, ids=ORTH_IDS)
def test_davidson_orth(dtype, cfg):
    N, k0, q, passes, B, extra = cfg
    g = _gen("orth", str(dtype), cfg)
    ld = pad_len(N) + extra
    V0 = _orth_basis(g, dtype, B, k0, q, N)
    Vb = _Buf(V0, dtype, k0 + q + 2, ld)
    nC, nW = B * q * max(k0, q), B * q * q
    Cf, C = _guarded(nC, dtype)
    Wf, W = _guarded(nW, dtype)
    info = torch.zeros(B, dtype=torch.int32, device=DEV)
    cond = torch.zeros(B, dtype=dtype, device=DEV)
    ref = dref.orth(V0, k0, q, passes, dtype, cond=torch.zeros(B, dtype=torch.float64))
    assert bool((ref["_meta"]["kappa2"] <= dref.KAPPA2_MAX[dtype]).all()), ref["_meta"]["kappa2"]
    what = "davidson_orth %s N=%d k0=%d q=%d passes=%d B=%d ld=%d" % (dtype, N, k0, q, passes, B, ld)
    K.davidson_orth(Vb.dev, N, k0, q, C, W, info, passes=passes, cond=cond)
    Q = dref.hp(Vb.dev[:, k0:k0 + q, :N])
    _check({"Q": Q, "info": info, "cond": cond}, ref, dtype, what, "orth")
    Vb.pad_zero(what)
    Vb.only_changed((k0, k0 + q), what)
    _guard_ok(Cf, nC, what + " (C)")
    _guard_ok(Wf, nW, what + " (W)")
    if passes >= 2:
        po, pq = dref.orth_properties(V0, Q, k0, dtype)
        tol = dref.orth_tolerance(dtype, N, k0, q)
        assert bool((po <= tol).all()) and bool((pq <= tol).all()), (what, po.tolist(), pq.tolist(), tol)
    Q1 = Vb.dev.clone()
    Vb.dev.copy_(Vb.before)
    info.zero_()
    cond.zero_()
    K.davidson_orth(Vb.dev, N, k0, q, C, W, info, passes=passes, cond=cond)
    assert torch.equal(_bits(Q1), _bits(Vb.dev)), what + ": not bit-reproducible"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("q", [3, 8, 12, 32])
@pytest.mark.parametrize("passes", [0, 1])
def test_davidson_orth_info_flags_a_zero_row(dtype, q, passes):
    """row j = 2 of member 1's panel is zero: info = j + 1 on the fused (q <= 8) and the wide (9..32) path; member 0's
    preset info survives (sticky), member 2 stays 0 and is orthonormalised as if alone"""
    N, k0, B = 1500, 4, 3
    g = _gen("info", str(dtype), q, passes)
    V0 = _orth_basis(g, dtype, B, k0, q, N)
    V0[1, k0 + 2] = 0
    Vb = _Buf(V0, dtype, k0 + q + 1, pad_len(N))
    C = torch.empty(B * q * max(k0, q), dtype=dtype, device=DEV)
    W = torch.empty(B * q * q, dtype=dtype, device=DEV)
    info = torch.tensor([5, 0, 0], dtype=torch.int32, device=DEV)
    K.davidson_orth(Vb.dev, N, k0, q, C, W, info, passes=passes)
    assert info.tolist() == [5, 3, 0], (dtype, q, passes, info.tolist())
    ref = dref.orth(V0[2:], k0, q, passes, dtype)
    _check({"Q": dref.hp(Vb.dev[2:, k0:k0 + q, :N]), "info": torch.zeros(1)}, ref, dtype,
           "davidson_orth zero row q=%d passes=%d" % (q, passes), "orth")


def test_zz_worst_ratios():
    """the worst error / bound ratio per (dtype, kernel) of this run; written as JSON where XK_WORST_JSON points"""
    rep = {"%s/%s" % k: v for k, v in sorted(dref.WORST.items())}
    print("davidson kernels worst error/bound:", json.dumps(rep))
    path = os.environ.get("XK_WORST_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(rep, f, indent=1)
    assert all(v <= 1.0 for v in rep.values())
