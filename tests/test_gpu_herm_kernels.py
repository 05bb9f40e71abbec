"""-m gpu: the Hermitian Davidson kernels (xk_herm_ritz, xk_herm_cholqr, xk_herm_eigh, both complex types) and
kernels.dense_outer_complex against the complex128 restatement of tests/herm_ref.py: per entry, on strided views inside
sentinel-filled buffers, with the layouts the driver passes.  tests/test_herm_ref.py shows on the CPU that these checks
reject the faults of herm_ref.FAULTS at these shapes."""
import math
import pytest
import torch
from xitorch_amd import kernels as K
from xitorch_amd.linalg import native_eig_herm
from tests import herm_ref as hr

pytestmark = pytest.mark.gpu
c128, c64 = hr.c128, hr.c64
DTYPES = [c128, c64]
IDS = ["c128", "c64"]
NAN = complex(math.nan, math.nan)
SENT = complex(777.0, -333.0)


def _bits(t):
    """the storage of t as integers: equality of bit patterns, NaN included"""
    t = t.detach()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().view({8: torch.int64, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _panel(val, dtype, dev, cap, pad, extra, fill, row0=0):
    """val (B, R, N) placed in rows [row0, row0 + R) of a strided (B, cap, N) view (pitch N + pad, member stride
    cap * pitch + extra, offset 3) into a buffer filled with `fill`; returns (buffer, the (B, cap, N) view)"""
    B, R, N = val.shape
    ld = N + pad
    sB = cap * ld + extra
    buf = torch.full((B * sB + 8,), fill, dtype=dtype, device=dev)
    view = buf.as_strided((B, cap, N), (sB, ld, 1), 3)
    view[:, row0:row0 + R].copy_(val.to(dtype))
    return buf, view


def _outside_unchanged(buf, before, region):
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask.as_strided(region.shape, region.stride(), region.storage_offset()).fill_(False)
    return _same_bits(buf[mask], before[mask])


# ------------------------------------------------------------------------------------------------ Ritz
def _y_view(Y, layout, dtype, dev):
    B, k, p = Y.shape
    Yd = Y.to(dtype).to(dev)
    if layout == "contiguous":
        return Yd.contiguous()
    if layout == "transposed":                           # what the driver passes: herm_eigh's (B, p, k) output
        buf = torch.full((B, p + 1, k + 2), NAN, dtype=dtype, device=dev)
        buf[:, :p, :k] = Yd.transpose(1, 2)
        return buf[:, :p, :k].transpose(1, 2)
    buf = torch.full((B, 2 * k + 1, 3 * p + 2), NAN, dtype=dtype, device=dev)
    view = buf[:, 0:2 * k:2, 1:3 * p + 1:3]
    view.copy_(Yd)
    return view


def _run_ritz(dev, dtype, B, k, p, N, with_m, layout, plant=None):
    what = "herm_ritz %s %s" % (hr.DNAME[dtype], (B, k, p, N, with_m, layout, plant))
    c = hr.ritz_case(dtype, B, k, p, N, with_m)
    if plant is not None:
        c = hr.ritz_plant(c, plant)
    _, V = _panel(c["V"], dtype, dev, k + 3, 5, 11, NAN)
    _, AV = _panel(c["AV"], dtype, dev, k + 3, 5, 29, NAN)
    MV = _panel(c["MV"], dtype, dev, k + 3, 6, 7, NAN)[1] if with_m else None
    Y = _y_view(c["Y"], layout, dtype, dev)
    lbuf = torch.full((B, p + 4), math.nan, dtype=hr.REAL[dtype], device=dev)
    lbuf[:, 2:2 + p] = c["lam"].to(hr.REAL[dtype])
    lam = lbuf[:, 2:2 + p]
    zeros = torch.zeros(B, p, N, dtype=c128)
    xbuf, X = _panel(zeros, dtype, dev, p + 2, 3, 13, SENT)
    tbuf, Tn = _panel(zeros, dtype, dev, p + 2, 9, 5, SENT)
    X[:, :p].fill_(SENT)
    Tn[:, :p].fill_(SENT)
    x0, t0 = xbuf.clone(), tbuf.clone()
    status = torch.full((B + 2,), 7.0, dtype=torch.float64, device=dev)
    K.herm_ritz(V, AV, Y, lam, X, Tn, status, k, p, MV=MV)
    x1, t1, s1 = xbuf.clone(), tbuf.clone(), status.clone()
    ref = hr.ritz(c["V"], c["AV"], c["MV"], c["Y"], c["lam"], dtype)
    got = {"X": X[:, :p], "Tn": Tn[:, :p], "status": status[:B + 1]}
    hr.check(got, ref, dtype, what=what, kernel="herm_ritz")
    assert hr.status_consistent(status[:B + 1]), what
    assert status[B + 1].item() == 7.0, what + ": status written past B + 1"
    assert _outside_unchanged(xbuf, x0, X[:, :p]) and _outside_unchanged(tbuf, t0, Tn[:, :p]), what + ": stray write"
    K.herm_ritz(V, AV, Y, lam, X, Tn, status, k, p, MV=MV)
    assert _same_bits(xbuf, x1) and _same_bits(tbuf, t1) and _same_bits(status, s1), what + ": not reproducible"
    return status.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k", hr.RITZ_K)
def test_ritz_per_entry(dev, dtype, k):
    for cfg in hr.ritz_configs(k) + ([hr.RITZ_LONG] if k == hr.RITZ_LONG[1] else []):
        _run_ritz(dev, dtype, *cfg)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("value", [math.nan, math.inf])
def test_ritz_status_propagates_non_finite(dev, dtype, value):
    """a NaN / Inf in AV of the last member reaches status[1 + b] and status[0]; the other members stay finite"""
    B = 3
    same = torch.isnan if math.isnan(value) else torch.isinf
    for (k, p, N, with_m, layout) in ((5, 17, 257, True, "transposed"), (40, 6, 1037, False, "contiguous")):
        st = _run_ritz(dev, dtype, B, k, p, N, with_m, layout, plant=value)
        assert bool(same(st[0])) and bool(same(st[B])) and bool(torch.isfinite(st[1:B]).all()), st


# ------------------------------------------------------------------------------------------------ CholeskyQR
def _run_cholqr(dev, dtype, q, N, with_m, shifted, kind, per_entry):
    what = "herm_cholqr %s %s" % (hr.DNAME[dtype], (kind, q, N, with_m, shifted))
    B = hr.CHOL_B
    c = hr.cholqr_case(dtype, q, N, with_m, kind)
    sh = native_eig_herm._shift_rel(N, q, hr.REAL[dtype]) if shifted else 0.0
    assert sh == (hr.shift_rel(N, q, dtype) if shifted else 0.0)
    k0, cap = 3, q + 5                                   # the driver orthonormalises in place inside the basis
    wbuf, Wc = _panel(c["W"], dtype, dev, cap, 7, 9, SENT, row0=k0)
    W = Wc[:, k0:k0 + q]
    mbuf, MW = None, None
    if with_m:
        mbuf, Mc = _panel(c["MW"], dtype, dev, cap, 2, 21, SENT, row0=k0)
        MW = Mc[:, k0:k0 + q]
    w0, m0 = wbuf.clone(), (mbuf.clone() if with_m else None)
    info = torch.zeros(B, dtype=torch.int32, device=dev)
    Rinv = K.herm_cholqr(W, info, MW=MW, shift_rel=sh)
    fac = hr.cholqr_factor(c["W"], c["MW"], hr.cast(sh, dtype), dtype)
    meta = fac["_meta"]
    # info = 0 wherever Cholesky is bound to succeed; beyond that (complex64, nearly dependent, unshifted) a flagged
    # breakdown is legitimate, and only the structure of Rinv and the bookkeeping of the apply kernel are asserted
    must = hr.cholesky_must_succeed(meta["G"], N, dtype)
    done = info.cpu() == 0
    assert bool((done | ~must).all()), what + ": info %s" % info.cpu().tolist()
    assert not per_entry or bool(must.all()), what
    hr.cholqr_properties(Rinv, meta["G"], N, dtype, what=what, members=done)
    info.zero_()
    if per_entry:
        assert bool((meta["kappa2"] <= hr.KAPPA2_MAX[hr.REAL[dtype]]).all()), what
        hr.check({"Rinv": Rinv}, fac, dtype, what=what, kernel="herm_cholqr:Rinv")
    ap = hr.cholqr_apply(c["W"], c["MW"], hr.hp(Rinv), dtype)
    got = {"W": W, "MW": MW} if with_m else {"W": W}
    hr.check(got, ap, dtype, what=what, kernel="herm_cholqr:apply")
    assert _outside_unchanged(wbuf, w0, W), what + ": stray write"
    if with_m:
        assert _outside_unchanged(mbuf, m0, MW), what + ": stray write"
    w1, r1 = wbuf.clone(), Rinv.clone()
    wbuf.copy_(w0)
    if with_m:
        m1 = mbuf.clone()
        mbuf.copy_(m0)
    Rinv2 = K.herm_cholqr(W, info, MW=MW, shift_rel=sh)
    assert _same_bits(Rinv2, r1) and _same_bits(wbuf, w1) and (not with_m or _same_bits(mbuf, m1)), \
        what + ": not reproducible"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", hr.CHOL_N + (33,))
def test_cholqr_per_entry(dev, dtype, N):
    for (q, N, with_m, shifted) in hr.cholqr_entry_configs(N):
        _run_cholqr(dev, dtype, q, N, with_m, shifted, "gauss", True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cholqr_properties_of_ill_conditioned_blocks(dev, dtype):
    for (kind, q, N, with_m, shifted) in hr.CHOL_PROP_CONFIGS:
        _run_cholqr(dev, dtype, q, N, with_m, shifted, kind, False)


# ------------------------------------------------------------------------------------------------ eigh
def _eigh_call(dev, dtype, T, n, p, uppest):
    """T (B, n, n) complex128 as stored, inside a (B, n + 5, n + 3) buffer of NaN; workspace poisoned"""
    B = T.shape[0]
    buf = torch.full((B, n + 5, n + 3), NAN, dtype=dtype, device=dev)
    buf[:, :n, :n] = T.to(dtype)
    rdt = hr.REAL[dtype]
    K._workspace(max(5 * B * n * p, 1), rdt, dev).fill_(math.nan)
    lam, Y, flag = K.herm_eigh(buf, n, p, uppest=uppest)
    out = (lam.clone(), Y.clone(), flag.clone())
    K._workspace(max(5 * B * n * p, 1), rdt, dev).fill_(math.nan)
    lam2, Y2, flag2 = K.herm_eigh(buf, n, p, uppest=uppest)
    assert _same_bits(lam2, out[0]) and _same_bits(Y2, out[1]) and torch.equal(flag2, out[2]), "not reproducible"
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", hr.EIGH_N)
def test_eigh_contracted_matrix(dev, dtype, n):
    """lower triangle read, NaN above it and around the block never touched, imaginary diagonal ignored"""
    for kind in hr.EIGH_KINDS:
        T = hr.eigh_case(dtype, kind, n)
        if T is None:
            continue
        for p in hr.EIGH_P:
            if p > n:
                continue
            for uppest in (False, True):
                what = "herm_eigh %s %s" % (hr.DNAME[dtype], (kind, n, p, uppest))
                lam, Y, flag = _eigh_call(dev, dtype, T, n, p, uppest)
                assert flag.cpu().tolist() == [0] * hr.EIGH_B, what + ": flags %s" % flag.cpu().tolist()
                hr.eigh_check(T, lam, Y, p, uppest, dtype, what=what)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [2, 7, 64, 128])
def test_eigh_ignores_imaginary_diagonal(dev, dtype, n):
    """the contract stated literally: the same matrix with a zero and with a garbage imaginary diagonal gives the
    same bits.  (While the packed triangle was loaded with the diagonal's imaginary part, the two calls differed by
    |d lam| = 2.3 .. 5.9 and |d Y| = 0.4 .. 1.6 at n = 2 .. 128 in both dtypes: errors of the size of |T|.)"""
    p = min(6, n)
    T = hr.eigh_case(dtype, "generic", n)
    d = torch.diagonal(T, dim1=-2, dim2=-1)
    assert bool((d.imag.abs() > 0).all())
    T0 = T - torch.diag_embed(torch.complex(torch.zeros_like(d.imag), d.imag))
    for uppest in (False, True):
        lam, Y, flag = _eigh_call(dev, dtype, T, n, p, uppest)
        lam0, Y0, flag0 = _eigh_call(dev, dtype, T0, n, p, uppest)
        assert flag.cpu().tolist() == flag0.cpu().tolist() == [0] * hr.EIGH_B
        dl = (lam - lam0).abs().max().item()
        dy = (Y - Y0).abs().max().item()
        print("imaginary diagonal, %s n = %d uppest = %s: |d lam| %.3e |d Y| %.3e" % (hr.DNAME[dtype], n, uppest, dl, dy))
        assert torch.equal(lam, lam0) and torch.equal(Y, Y0), (dl, dy)


# ------------------------------------------------------------------------------------------------ dense_outer_complex
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dense_outer_complex_per_entry(dev, dtype):
    for B in hr.OUTER_B:
        for C in hr.OUTER_C:
            for (M, N) in hr.OUTER_MN:
                U, W = hr.outer_case(dtype, B, C, M, N)
                G = K.dense_outer_complex(U.to(dtype).to(dev), W.to(dtype).to(dev))
                assert G.shape == (B, M, N) and G.dtype == dtype
                got = torch.view_as_real(G).reshape(B, M, 2 * N)
                hr.check({"G": got}, hr.dense_outer_complex(U, W, dtype), dtype,
                         what="dense_outer_complex %s %s" % (hr.DNAME[dtype], (B, C, M, N)), kernel="dense_outer_complex")


def test_report_worst_ratios(dev):
    """the largest |kernel - reference| / bound (measured / tolerance for herm_eigh) per kernel and dtype seen by this
    module's checks (run last)"""
    for key in sorted(hr.WORST):
        print("WORST %s %s: %.3g" % (key[0], key[1], hr.WORST[key]))
    assert all(v <= 1.0 for v in hr.WORST.values())
