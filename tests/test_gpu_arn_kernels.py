"""-m gpu: the Krylov-Schur Arnoldi kernels (xk_arn.hip) against their restatement tests/arn_ref.py and numpy.linalg.eig.

xk_arn_finish: the same bits as xk_gkl_finish on the same partials; the stored / accumulated column of H per entry
against float64 sums.  xk_arn_schur: on the matrices of tests/arn_cases.py, orders 2 .. xk_arn_max_rows(), one and three
members per launch (three DIFFERENT matrices: members must not see each other), real and complex, every `which`.
Acceptance (the form of test_gpu_fnm_kernels.py): each of

    |B Q - Q Hnext|_F     (complex: Q = Z[:, :keep'], Hnext = T[:keep', :keep'], so this is |B Z - Z T|_F on the kept
                           columns; run with keep = m - 1 as well, where only the last Schur vector is missing)
    |Q^H Q - I|_F
    |B Y - Y diag(theta)|_F over the neig Ritz vectors
    the eigenvalue multiset distance to numpy.linalg.eig

is <= 4 x the restatement's own value on the same input + 16 m eps |B|_F (16 m eps for the dimensionless second one),
eps of double.  For the Jordan case only the residuals are compared.  The kernel has no output for the whole of Z and T.
"""
import functools
import numpy as np
import pytest
import torch
from tests import arn_ref, arn_cases as ac
from xitorch_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = np.finfo(np.float64).eps
WORST = {}


def _orders():
    return [2, 3, 5, 16, 17, 33, K.arn_max_rows()]


def _sizes(m):
    neig = max(1, min(3, m - 2))
    return neig, min(m - 1, neig + (m - neig) // 2)


def _dist(a, b):
    rem, d = list(b), 0.0
    for t in a:
        j = int(np.argmin(np.abs(np.array(rem) - t)))
        d = max(d, abs(rem.pop(j) - t))
    return d


def _figures(H, theta, Y, Q, Hn, kp, neig):
    m = H.shape[1]
    B = H[:m].astype(np.complex128)
    Qk, Hk = Q[:, :kp], Hn[:kp, :kp]
    return dict(inv=np.linalg.norm(B @ Qk - Qk @ Hk), orth=np.linalg.norm(Qk.conj().T @ Qk - np.eye(kp)),
                ritz=np.linalg.norm(B @ Y - Y * theta[:neig]), eig=_dist(theta, np.linalg.eigvals(B)))


@functools.lru_cache(maxsize=None)
def _reference(kind, m, cplx, which, neig, keep):
    H = _matrix(kind, m, cplx, keep)
    r = arn_ref.schur_restart(H, neig, keep, which, not cplx, tol=1e-6)
    return r, _figures(H, r["theta"], r["Y"], r["Q"], r["Hnext"], r["keep"], neig)


def _matrix(kind, m, cplx, keep):
    if kind == "rotation":
        return ac.rotation2().astype(np.complex128 if cplx else np.float64)
    if kind == "straddle":
        return ac.straddle(m, keep).astype(np.complex128 if cplx else np.float64)
    return ac.small_matrix(kind, m, cplx)


def _launch(Hs, neig, keep, which, **kw):
    H = torch.from_numpy(np.stack(Hs)).to(DEV)
    Hn = torch.full_like(H, -7.0)
    theta, Y, res, Q, status = K.arn_schur(H, neig, keep, which=which, tol=1e-6, u=EPS, Hnext=Hn, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (theta, Y, res, Q, Hn, status)]


def _accept(kind, m, cplx, which, neig, keep, H, out, b):
    theta, Y, res, Q, Hn, status = (t[b] for t in out)
    ref, fref = _reference(kind, m, cplx, which, neig, keep)
    assert status[2] & (K.ARN_FLAG_NONFINITE | K.ARN_FLAG_QR_LIMIT | K.ARN_FLAG_NOT_CLOSED) == 0, (kind, m, which, status)
    kp = int(status[3])
    tied = kind in ("companion", "identity", "zero")              # equal keys: the order among them is rounding's
    if not tied:
        assert kp == ref["keep"] and int(status[0]) == ref["nconv"], (kind, m, which, status, ref["keep"])
    assert 0 <= kp <= m - 1 and np.all(Q[:, kp:] == 0) and np.all(Hn[kp + 1:] == 0) and np.all(Hn[:, kp:] == 0)
    if not cplx:
        assert Q.dtype == np.float64
    nB = np.linalg.norm(H[:m])
    fdev = _figures(H, theta, Y, Q, Hn, kp, neig)
    for name in ("inv", "orth", "ritz", "eig"):
        if kind == "jordan" and name in ("eig", "ritz"):
            continue                                              # a defective pair: only the invariance is compared
        slack = 16 * m * EPS * (1.0 if name == "orth" else nB)
        bound = 4 * fref[name] + slack
        assert fdev[name] <= bound, (kind, m, cplx, which, name, fdev[name], fref[name], slack)
        if bound > 0:
            WORST[name] = max(WORST.get(name, 0.0), fdev[name] / bound)
    beta = H[m, m - 1]
    assert np.abs(Hn[kp, :kp] - beta * Q[m - 1, :kp]).max(initial=0.0) <= 4 * EPS * abs(beta)
    assert np.allclose(res, abs(beta) * np.abs(Y[m - 1]), rtol=1e-13, atol=0)
    assert np.allclose(np.linalg.norm(Y, axis=0), 1.0, rtol=0, atol=8 * EPS)


KINDS = list(ac.SMALL_KINDS)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("mi", range(7))
def test_schur_against_restatement(mi, cplx):
    m = _orders()[mi]
    neig, keep = _sizes(m)
    kinds = [k for k in KINDS if m >= 5 or k not in ("jordan", "hess_spike")]
    for which in (("LM", "LR", "SR", "LI", "SI") if cplx else ("LM", "LR", "SR")):
        # three different members per launch, then every matrix alone
        for i in range(0, len(kinds), 3):
            trio = (kinds + kinds)[i:i + 3]
            Hs = [_matrix(k, m, cplx, keep) for k in trio]
            out = _launch(Hs, neig, keep, which)
            for b, k in enumerate(trio):
                _accept(k, m, cplx, which, neig, keep, Hs[b], out, b)
        for k in kinds[:4]:
            H = _matrix(k, m, cplx, keep)
            _accept(k, m, cplx, which, neig, keep, H, _launch([H], neig, keep, which), 0)
    if m > 2:                                                     # all Schur vectors but the last one
        H = _matrix("random", m, cplx, m - 1)
        n1 = min(neig, m - 1)
        _accept("random", m, cplx, "LM", n1, m - 1, H, _launch([H], n1, m - 1, "LM"), 0)


@pytest.mark.parametrize("m,keep", [(5, 2), (6, 3), (16, 9), (17, 10), (33, 18), (48, 25), (48, 26)])
def test_a_pair_across_the_cut(m, keep):
    H = _matrix("straddle", m, False, keep)
    out = _launch([H, H, H], 2, keep, "LM")
    for b in range(3):
        _accept("straddle", m, False, "LM", 2, keep, H, out, b)
        st = out[5][b]
        assert st[3] == keep + 1 and st[2] & K.ARN_FLAG_KEEP_MOVED
        th = out[0][b]
        assert abs(th[keep - 1] - np.conj(th[keep])) <= 1e-12 and th[keep - 1].imag > 0
    # keep_add: one more vector for member 1 only; the next cut (keep + 1 | keep + 2) is between two pairs
    add = torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV)
    out = _launch([H, H, H], 2, keep, "LM", keep_add=add)
    assert [int(out[5][b][3]) for b in range(3)] == [keep + 1, keep + 1, keep + 1]
    # the same matrix as a complex operator: no pairing
    Hc = H.astype(np.complex128)
    assert int(_launch([Hc], 2, keep, "LM")[5][0][3]) == keep


def test_rotation():
    H = ac.rotation2()
    out = _launch([H], 1, 1, "LM")
    theta, st = out[0][0], out[5][0]
    assert st[3] == 0 and np.allclose(np.sort_complex(theta), [-1j, 1j], atol=4 * EPS) and theta[0].imag > 0
    _accept("rotation", 2, False, "LM", 1, 1, H, out, 0)


def test_nonfinite_sets_the_flag_and_writes_nothing_else():
    m = 12
    good = ac.small_matrix("random", m, False)
    bad = good.copy()
    bad[3, 4] = np.nan
    H = torch.from_numpy(np.stack([good, bad, good])).to(DEV)
    out = (torch.full((3, m), -7.0, dtype=torch.complex128, device=DEV),
           torch.full((3, m, 2), -7.0, dtype=torch.complex128, device=DEV),
           torch.full((3, 2), -7.0, dtype=torch.float64, device=DEV),
           torch.full((3, m, m), -7.0, dtype=torch.float64, device=DEV),
           torch.full((3, 8), -7, dtype=torch.int32, device=DEV))
    Hn = torch.full_like(H, -7.0)
    K.arn_schur(H, 2, 7, which="LM", tol=1e-6, u=EPS, Hnext=Hn, out=out)
    status = out[4].cpu().numpy()
    assert status[1, 2] == K.ARN_FLAG_NONFINITE and status[0, 2] == 0 and status[2, 2] == 0
    for t in out[:4] + (Hn,):
        assert bool((t[1] == -7.0).all()) and not bool((t[0] == -7.0).all())
    assert torch.equal(out[0][0], out[0][2]) and torch.equal(out[3][0], out[3][2])


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_repeat_launch_returns_the_same_bits(cplx):
    m = K.arn_max_rows()
    Hs = [ac.small_matrix(k, m, cplx) for k in ("random", "hess_spike", "companion")]
    a = _launch(Hs, 3, 25, "LM")
    b = _launch(Hs, 3, 25, "LM")
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("Bt", [1, 3])
@pytest.mark.parametrize("rows,nchunk", [(1, 1), (5, 64), (17, 130), (47, 3)])
def test_finish_equals_gkl_finish_and_accumulates(rows, nchunk, Bt, cplx):
    nval = (2 * rows if cplx else rows) + 1
    m = 48
    g = torch.Generator().manual_seed(rows * 7 + nchunk)
    parts = [torch.randn(Bt * nval * nchunk, dtype=torch.float64, generator=g) for _ in range(2)]
    for p in parts:                                               # the sum of squares is positive
        p.view(Bt, nval, nchunk)[:, nval - 1].abs_()
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=DEV)
    H = torch.zeros((Bt, m + 1, m), dtype=torch.complex128 if cplx else torch.float64, device=DEV)
    j = rows - 1
    hcol = H[:, :rows, j]
    Hr = torch.view_as_real(H) if cplx else H.unsqueeze(-1)
    outs = []
    for who in ("gkl", "arn"):
        coef, nrm, rnrm, smax, dst = f64(Bt, nval - 1), f64(Bt), f64(Bt), f64(Bt) + 0.5, f64(Bt, 3)
        brk = torch.full((Bt,), -1, dtype=torch.int32, device=DEV)
        for i, p in enumerate(parts):
            pd = p.to(DEV)
            if who == "gkl":
                K.gkl_finish(pd, Bt, nval, nchunk, coef, nrm, rnrm, dst=dst[:, 1], smax=smax, u=1e-16, brk=brk, code=4)
            else:
                K.arn_finish(pd, Bt, nval, nchunk, coef, nrm, rnrm, hcol=hcol, accumulate=i == 1, dst=Hr[:, j + 1, j, 0],
                             smax=smax, u=1e-16, brk=brk, code=4)
        torch.cuda.synchronize()
        outs.append((coef.cpu(), nrm.cpu(), rnrm.cpu(), smax.cpu(), brk.cpu(),
                     dst[:, 1].cpu() if who == "gkl" else Hr[:, j + 1, j, 0].cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # the column: c1 + c2 per entry against float64 sums; nothing else of H is touched
    P = [p.view(Bt, nval, nchunk).numpy() for p in parts]
    want = P[0][:, :nval - 1].sum(-1) + P[1][:, :nval - 1].sum(-1)
    mag = np.abs(P[0][:, :nval - 1]).sum(-1) + np.abs(P[1][:, :nval - 1]).sum(-1)
    got = torch.view_as_real(hcol).reshape(Bt, -1).cpu().numpy() if cplx else hcol.cpu().numpy()
    assert np.all(np.abs(got - want) <= (nchunk + 2) * EPS * mag)
    Hc = H.clone()
    Hc[:, :rows, j] = 0
    Hc[:, j + 1, j] = 0
    assert not bool(Hc.any())


def test_finish_flags_a_breakdown_like_gkl_finish():
    Bt, nval, nchunk = 2, 3, 2
    part = torch.tensor([[[1.0, 1.0], [2.0, 2.0], [1e-40, 0.0]], [[1.0, 0.0], [0.0, 1.0], [4.0, 5.0]]],
                        dtype=torch.float64, device=DEV).reshape(-1)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=DEV)
    coef, nrm, rnrm, smax, H = f64(Bt, 2), f64(Bt), f64(Bt), f64(Bt) + 1.0, f64(Bt, 4, 3)
    brk = torch.full((Bt,), -1, dtype=torch.int32, device=DEV)
    K.arn_finish(part, Bt, nval, nchunk, coef, nrm, rnrm, hcol=H[:, :2, 1], dst=H[:, 2, 1], smax=smax, u=1e-16, brk=brk,
                 code=9)
    torch.cuda.synchronize()
    assert brk.tolist() == [9, -1] and nrm.tolist() == [0.0, 3.0] and H[:, 2, 1].tolist() == [0.0, 3.0]
    assert H[:, :2, 1].tolist() == [[2.0, 4.0], [1.0, 1.0]] and smax.tolist() == [1.0, 3.0]


def test_worst_ratio_report():
    for name, w in sorted(WORST.items()):
        print("xk_arn_schur: worst %s / bound %.3f" % (name, w))
        assert w <= 1.0
