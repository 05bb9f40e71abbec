"""not-gpu: `solve(..., method="minres")` on operators in host memory (xitorch_amd/linalg/host_krylov.py::minres, the
torch restatement of the HIP driver): definite, indefinite, shifted (E, E and M), complex Hermitian, preconditioned,
non-converging, refused inputs, a consistent singular system, and the backward passes of solve / symeig through
`bck_options={"method": "minres"}`.  Criterion of the solves: the package's Krylov bar
|X - X_ref| <= 2 rtol kappa |X_ref| against a dense float64 / complex128 solve."""
import warnings
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd.linalg import host_krylov, solve, symeig, svd
from tests import minres_ref as mref
from tests.test_minres_ref import singular_case, singular_drift

F64 = torch.float64
RTOL = 1e-9


def _herm(seed, n, ev, dtype=F64):
    g = torch.Generator().manual_seed(seed)
    return mref.hermitian(g, dtype, n, ev)[0], g


def _randn(g, shape, dtype=F64):
    if dtype.is_complex:
        return torch.complex(torch.randn(shape, dtype=F64, generator=g), torch.randn(shape, dtype=F64, generator=g))
    return torch.randn(shape, dtype=F64, generator=g)


def _run(A, B, E=None, M=None, **kw):
    before = host_krylov.calls["minres"]
    tr = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        X = solve(xa.LinearOperator.m(A, is_hermitian=True), B, E=E,
                  M=None if M is None else xa.LinearOperator.m(M, is_hermitian=True), method="minres", rtol=RTOL,
                  trace=tr, **kw)
    assert host_krylov.calls["minres"] == before + 1
    assert tr["converged"] and tr["napply"] == tr["niter"] + 1 + tr["nrestart"]      # one apply per iteration
    h = tr["resid_history"]
    assert all(h[i + 1] <= h[i] * (1 + 1e-12) for i in range(len(h) - 1))
    return X, tr


def _close(X, Xref, kappa):
    assert float((X - Xref).norm()) <= 2 * RTOL * kappa * float(Xref.norm()), float((X - Xref).norm() / Xref.norm())


def test_definite():
    ev = torch.linspace(1.0, 40.0, 90, dtype=F64)
    A, g = _herm(1, 90, ev)
    B = _randn(g, (90, 3))
    X, _ = _run(A, B)
    _close(X, torch.linalg.solve(A, B), 40.0)


def test_indefinite_batched():
    ev = torch.linspace(0.1, 30.0, 120, dtype=F64) - 3.05
    kappa = float(ev.abs().max() / ev.abs().min())
    g = torch.Generator().manual_seed(2)
    A = torch.stack([mref.hermitian(g, F64, 120, ev)[0] for _ in range(2)])
    B = _randn(g, (2, 120, 2))
    X, tr = _run(A, B, max_niter=600)
    _close(X, torch.linalg.solve(A, B), kappa)
    assert tr["niter"] <= 120 + 2


def test_with_E_and_with_E_and_M():
    n = 70
    ev = torch.linspace(0.5, 20.0, n, dtype=F64)
    A, g = _herm(3, n, ev)
    B = _randn(g, (n, 2))
    E = torch.tensor([3.07, 11.13], dtype=F64)                     # both inside the spectrum
    X, _ = _run(A, B, E=E, max_niter=400)
    for c in range(2):
        As = A - E[c] * torch.eye(n, dtype=F64)
        k = float(torch.linalg.cond(As))
        _close(X[:, c], torch.linalg.solve(As, B[:, c]), k)
    M, _ = _herm(4, n, torch.linspace(1.0, 2.0, n, dtype=F64))
    X, _ = _run(A, B, E=E, M=M, max_niter=400)
    for c in range(2):
        As = A - E[c] * M
        _close(X[:, c], torch.linalg.solve(As, B[:, c]), float(torch.linalg.cond(As)))


def test_complex_hermitian():
    n = 80
    ev = torch.linspace(-4.0, 9.0, n, dtype=F64) + 0.07
    A, g = _herm(5, n, ev, torch.complex128)
    B = _randn(g, (n, 2), torch.complex128)
    X, _ = _run(A, B, max_niter=400)
    _close(X, torch.linalg.solve(A, B), float(ev.abs().max() / ev.abs().min()))
    # a complex-typed E with zero imaginary part is a real shift
    E = torch.tensor([0.4, -1.3], dtype=torch.complex128)
    X, _ = _run(A, B, E=E, max_niter=400)
    for c in range(2):
        As = A - E[c] * torch.eye(n, dtype=torch.complex128)
        _close(X[:, c], torch.linalg.solve(As, B[:, c]), float(torch.linalg.cond(As)))


def test_precond():
    n = 100
    g = torch.Generator().manual_seed(6)
    d = torch.logspace(0, 3, n, dtype=F64)
    d[::7] *= -1                                                  # indefinite, badly scaled
    R = 0.05 * torch.randn(n, n, dtype=F64, generator=g)
    A = torch.diag(d) + (R + R.T) / 2
    B = _randn(g, (n, 2))
    P = xa.LinearOperator.m(torch.diag(1.0 / d.abs()), is_hermitian=True)
    X0, tr0 = _run(A, B, max_niter=2000)
    X1, tr1 = _run(A, B, precond=P, max_niter=2000)
    kappa = float(torch.linalg.cond(A))
    _close(X0, torch.linalg.solve(A, B), kappa)
    _close(X1, torch.linalg.solve(A, B), kappa * 1e3)              # stops on the P-norm of the residual
    assert tr1["niter"] < tr0["niter"]
    with pytest.raises(RuntimeError, match="positive definite"):
        solve(xa.LinearOperator.m(A, is_hermitian=True), B, method="minres",
              precond=xa.LinearOperator.m(-torch.eye(n, dtype=F64), is_hermitian=True))


def test_nonconverging_warns_and_returns_a_confirmed_iterate():
    n = 150
    ev = torch.logspace(-3, 3, n, dtype=F64)
    ev[::2] *= -1
    A, g = _herm(7, n, ev)
    B = _randn(g, (n, 1))
    tr = {}
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        X = solve(xa.LinearOperator.m(A, is_hermitian=True), B, method="minres", rtol=1e-12, max_niter=15, trace=tr)
    msgs = [w for w in wl if issubclass(w.category, xa.ConvergenceWarning)]
    assert len(msgs) == 1 and not tr["converged"] and tr["niter"] == 15
    true = float((B - A @ X).norm())
    assert abs(true - tr["best_resid"]) <= 1e-10 * float(B.norm())   # the reported norm is the true one of X
    assert "%.3e" % tr["best_resid"] in str(msgs[0].message)
    assert true < float(B.norm())


def test_refused_inputs():
    n = 20
    g = torch.Generator().manual_seed(8)
    A = torch.randn(n, n, dtype=F64, generator=g)
    B = _randn(g, (n, 1))
    with pytest.raises(RuntimeError, match="bicgstab.*gmres"):
        solve(xa.LinearOperator.m(A, is_hermitian=False), B, method="minres")
    Ac, _ = _herm(9, n, torch.linspace(1, 2, n, dtype=F64), torch.complex128)
    with pytest.raises(RuntimeError, match="bicgstab.*gmres"):
        solve(xa.LinearOperator.m(Ac, is_hermitian=True), B.to(torch.complex128),
              E=torch.tensor([0.5 + 0.1j], dtype=torch.complex128), method="minres")
    # posdef is accepted and ignored
    Ah = (A + A.T) / 2 + 10 * torch.eye(n, dtype=F64)
    X = solve(xa.LinearOperator.m(Ah, is_hermitian=True), B, method="minres", posdef=False, rtol=RTOL)
    _close(X, torch.linalg.solve(Ah, B), float(torch.linalg.cond(Ah)))


def test_consistent_singular_system_stays_orthogonal_to_the_null_vector():
    A, lam, u, b = singular_case()
    n = A.shape[-1]
    tr = {}
    X = solve(xa.LinearOperator.m(A, is_hermitian=True), b.reshape(n, 1), E=lam.reshape(1), method="minres",
              rtol=1e-9, max_niter=3 * n, trace=tr)
    x = X[:, 0]
    assert tr["converged"]
    assert float(((A - lam * torch.eye(n, dtype=F64)) @ x - b).norm()) <= 1e-8 * float(b.norm())
    drift = float((u @ x).abs() / x.norm())
    assert drift <= 10 * max(singular_drift()["drift"], torch.finfo(F64).eps), drift


def test_gradcheck_solve_fwd_and_bck_minres():
    n = 12
    A0, g = _herm(10, n, torch.linspace(-2.0, 3.0, n, dtype=F64) + 0.3)
    A0 = A0.clone().requires_grad_()
    B0 = _randn(g, (n, 2)).requires_grad_()
    opts = {"method": "minres", "rtol": 1e-12, "atol": 1e-14, "max_niter": 200}

    def f(A, B):
        As = (A + A.T) / 2
        return solve(xa.LinearOperator.m(As, is_hermitian=True), B, bck_options=dict(opts), **opts)

    assert torch.autograd.gradcheck(f, (A0, B0), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_symeig_davidson_backward_through_minres_matches_exacteig():
    n, neig = 40, 3
    A0, g = _herm(11, n, torch.linspace(1.0, 25.0, n, dtype=F64) ** 1.3)
    wts = _randn(g, (neig,))
    wv = _randn(g, (n, neig))

    def loss(method, bck, **fwd):
        A = A0.clone().requires_grad_()
        As = (A + A.T) / 2
        ev, V = symeig(xa.LinearOperator.m(As, is_hermitian=True), neig=neig, mode="lowest", method=method,
                       bck_options=bck, **fwd)
        val = (ev * wts).sum() + ((V * wv).sum(0) ** 2).sum()          # sign-invariant in the eigenvectors
        val.backward()
        return A.grad

    g_ref = loss("exacteig", {})
    before = host_krylov.calls["minres"]
    g_min = loss("davidson", {"method": "minres", "rtol": 1e-11, "atol": 1e-13, "max_niter": 400}, min_eps=1e-10)
    assert host_krylov.calls["minres"] > before
    assert float((g_min - g_ref).norm()) <= 1e-6 * float(g_ref.norm()), float((g_min - g_ref).norm() / g_ref.norm())


def test_svd_backward_through_minres():
    g = torch.Generator().manual_seed(12)
    A0 = _randn(g, (14, 9))
    W1, W2 = _randn(g, (14, 2)), _randn(g, (2, 9))

    def grad(method, bck):
        A = A0.clone().requires_grad_()
        U, s, Vh = svd(xa.LinearOperator.m(A), k=2, mode="uppest", method=method, bck_options=bck)
        (s.sum() + (U ** 2 * W1).sum() + (Vh ** 2 * W2).sum()).backward()      # sign-invariant in the vectors
        return A.grad

    g_ref = grad("exacteig", {})
    before = host_krylov.calls["minres"]
    g_min = grad("davidson", {"method": "minres", "rtol": 1e-11, "atol": 1e-13, "max_niter": 300})
    assert host_krylov.calls["minres"] > before
    assert float((g_min - g_ref).norm()) <= 1e-6 * float(g_ref.norm())
