"""CPU: the numpy restatement of xk_arn_schur (tests/arn_ref.py) against numpy.linalg.eig, on the matrices of
tests/arn_cases.py.  Bounds: 16 m eps |B|_F, the constant of the fnm and slq tests (16 m eps for the dimensionless
|Z^H Z - I|_F)."""
import numpy as np
import pytest
from tests import arn_ref, arn_cases

EPS = np.finfo(np.float64).eps
ORDERS = [2, 3, 5, 16, 17, 33, 48]


def _sizes(m):
    neig = max(1, min(3, m - 2))
    return neig, min(m - 1, neig + (m - neig) // 2)


def _multiset_distance(a, b):
    rem, d = list(b), 0.0
    for t in a:
        j = int(np.argmin(np.abs(np.array(rem) - t)))
        d = max(d, abs(rem.pop(j) - t))
    return d


def _check(H, neig, keep, which, real_op, eigenvalues=True):
    m = H.shape[1]
    B = H[:m].astype(np.complex128)
    nB = np.linalg.norm(B)
    bound = 16 * m * EPS * nB
    r = arn_ref.schur_restart(H, neig, keep, which, real_op, tol=1e-6)
    assert r["flags"] & (arn_ref.FLAG_NONFINITE | arn_ref.FLAG_QR_LIMIT) == 0
    T, Z, kp = r["T"], r["Z"], r["keep"]
    assert np.all(np.tril(T, -1) == 0)
    assert np.linalg.norm(B @ Z - Z @ T) <= bound
    assert np.linalg.norm(Z.conj().T @ Z - np.eye(m)) <= 16 * m * EPS
    ev = np.linalg.eigvals(B)
    if eigenvalues:
        assert _multiset_distance(r["theta"], ev) <= 1e3 * bound + 1e-300       # (eig's own error: not a kernel bound)
        # the leading block holds the selected eigenvalues: its keys are the kp largest keys
        lead = np.sort(arn_ref.rank_key(np.diag(T)[:kp], which))[::-1]
        best = np.sort(arn_ref.rank_key(ev, which))[::-1][:kp]
        assert np.abs(lead - best).max(initial=0.0) <= 1e3 * bound + 1e-300
    Q, Hn = r["Q"], r["Hnext"]
    if real_op:
        assert Q.dtype == np.float64 and Hn.dtype == np.float64
        assert not r["flags"] & arn_ref.FLAG_NOT_CLOSED
    assert Q.shape == (m, kp)
    assert np.linalg.norm(Q.conj().T @ Q - np.eye(kp)) <= 16 * m * EPS
    assert np.linalg.norm(B @ Q - Q @ Hn[:kp, :kp]) <= bound
    assert np.abs(Hn[kp, :kp] - H[m, m - 1] * Q[m - 1]).max(initial=0.0) <= EPS * abs(H[m, m - 1])
    Y = r["Y"]
    for i in range(neig):
        assert abs(np.linalg.norm(Y[:, i]) - 1) <= 8 * EPS
        if eigenvalues:
            assert np.linalg.norm(B @ Y[:, i] - r["theta"][i] * Y[:, i]) <= 1e3 * bound + 1e-300
    assert np.allclose(r["res"], abs(H[m, m - 1]) * np.abs(Y[m - 1]), rtol=1e-14, atol=0)
    return r


CASES = [(kind, m) for kind in arn_cases.SMALL_KINDS for m in ORDERS
         if m >= 5 or kind not in ("jordan", "hess_spike")]       # (these two constructions need order >= 5)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("kind,m", CASES)
def test_schur_restart(kind, m, cplx):
    H = arn_cases.small_matrix(kind, m, cplx)
    neig, keep = _sizes(m)
    for which in (("LM", "LR", "SR", "LI", "SI") if cplx else ("LM", "LR", "SR")):
        _check(H, neig, keep, which, not cplx, eigenvalues=kind != "jordan")


def test_rotation_has_the_imaginary_pair():
    r = _check(arn_cases.rotation2(), 1, 1, "LM", True)
    assert np.allclose(np.sort_complex(r["theta"]), [-1j, 1j], atol=4 * EPS)
    assert r["theta"][0].imag > 0 and r["keep"] == 0              # the pair cannot be cut: nothing is kept


@pytest.mark.parametrize("m,keep", [(5, 2), (6, 3), (16, 9), (17, 10), (33, 18), (48, 25), (48, 26)])
def test_a_pair_across_the_cut_moves_it(m, keep):
    H = arn_cases.straddle(m, keep)
    r = _check(H, 2, keep, "LM", True)
    assert r["keep"] == keep + 1 and r["flags"] & arn_ref.FLAG_KEEP_MOVED
    th = r["theta"]
    assert abs(th[keep - 1] - np.conj(th[keep])) <= 1e-12 and th[keep - 1].imag > 0
    # complex operator: no pairing, the cut stays
    r = arn_ref.schur_restart(H.astype(np.complex128), 2, keep, "LM", False)
    assert r["keep"] == keep


def test_order_and_pairs():
    lam = np.array([0.5, 1 + 1j, 1 - 1j, -2.0, 0.1j, -0.1j, 1.5])
    order, partner = arn_ref.ranking(lam, "LM", True)
    assert order == [3, 6, 1, 2, 0, 4, 5] and partner[1] == 2 and partner[4] == 5
    order, _ = arn_ref.ranking(lam, "LR", True)
    assert order == [6, 1, 2, 0, 4, 5, 3]
    order, partner = arn_ref.ranking(lam, "SI", False)
    assert order[0] == 2 and partner == [-1] * 7


def test_nonfinite_sets_the_flag_only():
    H = arn_cases.small_matrix("random", 8, False)
    H[2, 3] = np.nan
    r = arn_ref.schur_restart(H, 2, 5, "LM", True)
    assert r["flags"] == arn_ref.FLAG_NONFINITE and "theta" not in r


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_cycle_finds_the_dominant_pairs(cplx):
    A, lam = arn_cases.normal_matrix(90, 4, cplx)
    v0 = np.random.default_rng(3).standard_normal(90) + (0j if cplx else 0.0)
    th, X, info = arn_ref.arnoldi(lambda v: A @ v, 90, 4, "LM", 20, v0, not cplx, min_eps=1e-10)
    assert info["converged"] and info["niter"] <= 25
    want = lam[np.argsort(-np.abs(lam))][:4]
    assert _multiset_distance(th, want) <= 1e-9
    assert info["resid"].max() <= 2e-10 * 2.0
