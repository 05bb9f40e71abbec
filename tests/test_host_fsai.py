"""CPU: solve() with the FSAI preconditioner on host-memory operators (linalg/host_krylov.py drivers).

The problem is the variable-coefficient 5-point grid operator at n = 24 (tests/fsai_cases.py; condition number ~6e3).
In float64 at the drivers' default tolerance plain CG needs about 250 iterations and CG with fsai(A) about 60, so the
cap of 150 iterations sits a factor of about two from either side."""
import warnings
import numpy as np
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd.linop import SparseLinearOperator
from xitorch_amd.linalg import solve, fsai
from tests import fsai_cases as fc

n = 24
N = n * n
CAP = 150


@pytest.fixture(scope="module")
def problem():
    A, dense = fc.grid_operator(n, batch=False)
    B = torch.as_tensor(np.random.default_rng(5).standard_normal((N, 2)))
    X = torch.as_tensor(np.linalg.solve(dense[0], B.numpy()))
    return A, dense, B, X


def _residual_ok(A, X, B, rtol=1e-6):
    # the drivers stop on |r| < rtol |b| per column; the recurrence residual may sit a little off the true one
    r = (A.mm(X) - B).norm(dim=-2)
    return bool((r <= 2 * rtol * B.norm(dim=-2)).all())


@pytest.mark.parametrize("how", ["operator", "string"])
def test_cg_converges_within_the_cap(problem, how):
    A, dense, B, Xref = problem
    tr = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        X = solve(A, B, method="cg", max_niter=CAP, trace=tr, precond=fsai(A) if how == "operator" else "fsai")
    assert tr["converged"] and tr["niter"] <= CAP
    assert _residual_ok(A, X, B)
    assert float((X - Xref).norm() / Xref.norm()) < 1e-3          # kappa 6e3 times the residual tolerance


def test_plain_cg_does_not_converge_within_the_cap(problem):
    A, dense, B, Xref = problem
    with pytest.warns(xa.ConvergenceWarning):
        solve(A, B, method="cg", max_niter=CAP)


def test_minres_indefinite_accepts_the_operator(problem):
    A, dense, B, Xref = problem
    ev = np.linalg.eigvalsh(dense[0])
    shift = 0.5 * (ev[40] + ev[41])                                # inside the spectrum, in a gap
    As, ds = fc.grid_operator(n, batch=False, shift=shift)
    P = fsai(A)                                                    # of the definite operator: positive definite
    tr = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        X = solve(As, B, method="minres", precond=P, max_niter=4000, rtol=1e-8, trace=tr)
    assert tr["converged"]
    r = (torch.as_tensor(ds[0]) @ X - B).norm(dim=0)
    assert bool((r <= 1e-6 * B.norm(dim=0)).all())
    # the string builds fsai of the indefinite operator itself: rows fall back (MathWarning), P stays positive
    # definite, the solve still confirms its residual
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        warnings.simplefilter("ignore", xa.MathWarning)
        X2 = solve(As, B, method="minres", precond="fsai", max_niter=6000, rtol=1e-8)
    r2 = (torch.as_tensor(ds[0]) @ X2 - B).norm(dim=0)
    assert bool((r2 <= 1e-6 * B.norm(dim=0)).all())


def test_gradcheck_equals_the_unpreconditioned_one():
    """gradcheck perturbs one number at a time; perturbing one stored entry of a Hermitian operator alone would make
    it non-Hermitian, which cg does not solve, so the check runs over one parameter per symmetric pair (A.values =
    w[pair]); the gradients w.r.t. A.values themselves are compared with the unpreconditioned solve's directly."""
    m = 6
    crow, col, vals = fc.grid_csr(m)
    rows = np.repeat(np.arange(m * m), np.diff(crow))
    key = np.maximum(rows, col) * m * m + np.minimum(rows, col)
    ukey, first, pair = np.unique(key, return_index=True, return_inverse=True)
    pair = torch.as_tensor(pair)
    w0 = torch.as_tensor(vals[0][first]).requires_grad_()
    Bm = torch.as_tensor(np.random.default_rng(2).standard_normal((m * m, 2))).requires_grad_()
    opts = dict(method="cg", rtol=1e-12, atol=1e-14)

    def f(v, b, **kw):
        A = SparseLinearOperator(torch.as_tensor(crow), torch.as_tensor(col), v, (m * m, m * m), is_hermitian=True)
        return solve(A, b, bck_options=dict(opts, **kw), **opts, **kw)

    assert torch.autograd.gradcheck(lambda w, b: f(w[pair], b, precond="fsai"), (w0, Bm), atol=1e-6, rtol=1e-5)
    v0 = torch.as_tensor(vals[0]).requires_grad_()
    g1 = torch.autograd.grad((f(v0, Bm, precond="fsai") ** 2).sum(), (v0, Bm))
    g0 = torch.autograd.grad((f(v0, Bm) ** 2).sum(), (v0, Bm))
    for a, b in zip(g1, g0):
        assert torch.allclose(a, b, rtol=1e-8, atol=1e-10)


def test_bck_options_string(problem):
    A, dense, B, Xref = problem
    v = A.values.clone().requires_grad_()
    A2 = SparseLinearOperator(A.crow, A.col, v, (N, N), is_hermitian=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        X = solve(A2, B, method="cg", max_niter=CAP, precond="fsai",
                  bck_options=dict(method="cg", max_niter=CAP, precond="fsai"))
        (gv,) = torch.autograd.grad(X.sum(), (v,))
    assert bool(torch.isfinite(gv).all()) and float(gv.abs().max()) > 0


def test_unknown_strings_and_dense_operators_raise(problem):
    A, dense, B, Xref = problem
    with pytest.raises(TypeError, match="unknown preconditioner name"):
        solve(A, B, method="cg", precond="ilu")
    with pytest.raises(TypeError, match="unknown preconditioner name"):
        solve(A, B, method="minres", precond="jacobi")
    D = xa.LinearOperator.m(torch.as_tensor(dense[0]), is_hermitian=True)
    with pytest.raises(TypeError, match="needs a SparseLinearOperator"):
        solve(D, B, method="cg", precond="fsai")
    with pytest.raises(TypeError):
        solve(A, B, method="bicgstab", precond_l="fsai")             # bicgstab takes the operator explicitly
    # (the left preconditioner of bicgstab enters its omega only and leaves the iteration count where it was; the
    # right one shortens the run below the cap)
    P = fsai(A)
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        X = solve(A, B, method="bicgstab", precond_l=P)
        Xr = solve(A, B, method="bicgstab", precond_r=P, max_niter=CAP)
    assert _residual_ok(A, X, B) and _residual_ok(A, Xr, B)
