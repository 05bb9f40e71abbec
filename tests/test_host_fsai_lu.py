"""CPU: gmres(precond_r=) and the named preconditioner "fsai_lu" on host-memory operators (linalg/host_krylov.py).

The problem is the convection-diffusion grid of tests/fsai_lu_cases.py at n = 24, pe = 0.5 (order 576, kappa_2 = 317,
|A - A^T| / |A| = 0.13) with the right-hand side default_rng(1).standard_normal(N).  A numpy prototype of un-restarted
GMRES to a relative true residual of 1e-8 needed 103 Arnoldi steps without a preconditioner, 43 with
fsai_lu(A, power=1) and 30 with power=2; the test asks for half the plain count and measures both counts itself."""
import warnings
import numpy as np
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd.linop import LinearOperator, SparseLinearOperator
from xitorch_amd.linalg import solve, fsai_lu, FSAILUOperator, host_krylov
from tests import fsai_lu_cases as lc

n = 24
N = n * n
F64 = torch.float64


@pytest.fixture(scope="module")
def problem():
    Ad = lc.convdiff(n, 0.5)
    A = lc.operator_of_dense(Ad)
    B = torch.as_tensor(lc.convdiff_rhs(N))
    return A, Ad, B


def _relres(Ad, X, B):
    Ad = torch.as_tensor(Ad)
    return float(((Ad @ X.to(Ad.dtype) - B).norm(dim=-2) / B.norm(dim=-2)).max())


def _steps(A, B, **kw):
    tr = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        X = host_krylov.gmres(A, B, rtol=1e-8, atol=0.0, posdef=True, trace=tr, **kw)
    assert tr["converged"]
    return X, tr["arnoldi_steps"]


def test_exact_inverse_converges_in_one_step(problem):
    A, Ad, B = problem
    P = LinearOperator.m(torch.as_tensor(np.linalg.inv(Ad)), is_hermitian=False)
    X, steps = _steps(A, B, precond_r=P)
    assert steps == 1 and _relres(Ad, X, B) <= 1e-8


def test_halves_the_arnoldi_steps(problem):
    A, Ad, B = problem
    X0, plain = _steps(A, B)
    P1, P2 = fsai_lu(A), fsai_lu(A, power=2)
    assert int(P1.nfallback) == 0 and int(P2.nfallback) == 0
    X1, s1 = _steps(A, B, precond_r=P1)
    X2, s2 = _steps(A, B, precond_r=P2)
    print("gmres Arnoldi steps to 1e-8: plain %d, fsai_lu(power=1) %d, fsai_lu(power=2) %d" % (plain, s1, s2))
    assert 2 * s1 <= plain and s2 <= s1
    for X in (X0, X1, X2):
        assert _relres(Ad, X, B) <= 1e-8
    # the quality of the factors themselves
    GL, GU = lc.factors_dense(P1)
    assert np.linalg.norm(np.eye(N) - GL[0] @ Ad @ GU[0]) / np.sqrt(N) < 0.4


def test_restarted(problem):
    """GMRES(20) with a budget of 100 steps: with the preconditioner the run converges (56 steps, 2 restarts when this
    was written); the plain restarted run needs 162 steps, so within the same budget it does not converge and warns"""
    A, Ad, B = problem
    tr = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        X = host_krylov.gmres(A, B, rtol=1e-8, atol=0.0, posdef=True, restart=20, max_niter=100, trace=tr,
                              precond_r=fsai_lu(A))
    assert tr["converged"] and tr["restarts"] >= 1 and _relres(Ad, X, B) <= 1e-8
    tr0 = {}
    with pytest.warns(xa.ConvergenceWarning):
        host_krylov.gmres(A, B, rtol=1e-8, atol=0.0, posdef=True, restart=20, max_niter=100, trace=tr0)
    assert not tr0["converged"]


def test_shift_columns_and_batch(problem):
    A, Ad, B = problem
    # an E shift and a two-column B: column c solves (A - E_c I) x = b_c; P is built for A, still a fair preconditioner
    B2 = torch.as_tensor(lc.convdiff_rhs(N, 2))
    E = torch.tensor([-0.3, 0.05], dtype=F64)
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        X = host_krylov.gmres(A, B2, E=E, rtol=1e-8, atol=0.0, posdef=True, precond_r=fsai_lu(A))
    for c in range(2):
        r = (torch.as_tensor(Ad) - E[c] * torch.eye(N, dtype=F64)) @ X[:, c] - B2[:, c]
        assert float(r.norm() / B2[:, c].norm()) <= 1e-8
    # a batch of two operators with different values (the second at twice the convection strength)
    Ab = np.stack([Ad, lc.convdiff(n, 1.0)])
    A2 = lc.operator_of_dense(Ab)
    P = fsai_lu(A2)
    assert P.GL.values.shape[0] == 2 and not torch.equal(P.GL.values[0], P.GL.values[1])
    tr = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        Xb = host_krylov.gmres(A2, B2, rtol=1e-8, atol=0.0, posdef=True, precond_r=P, trace=tr)
    assert Xb.shape == (2, N, 2) and tr["arnoldi_steps"] <= 60
    for b in range(2):
        assert _relres(Ab[b], Xb[b], B2) <= 1e-8


def test_bicgstab_with_the_name(problem):
    A, Ad, B = problem
    tr, tr0 = {}, {}
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        X = solve(A, B, method="bicgstab", precond_r="fsai_lu", rtol=1e-8, atol=0.0, posdef=True, trace=tr)
        Xl = solve(A, B, method="bicgstab", precond_l="fsai_lu", rtol=1e-8, atol=0.0, posdef=True)
        solve(A, B, method="bicgstab", rtol=1e-8, atol=0.0, posdef=True, trace=tr0)
    assert _relres(Ad, X, B) <= 2e-8 and _relres(Ad, Xl, B) <= 2e-8
    assert tr["niter"] < tr0["niter"]


def test_solve_forward_and_gradients_against_exactsolve():
    m = 8
    Ad = lc.convdiff(m, 0.5)
    crow, col, vals = lc.csr_of_dense(Ad)
    crow_t, col_t = torch.as_tensor(crow), torch.as_tensor(col)
    b0 = torch.as_tensor(lc.convdiff_rhs(m * m, 2))
    opts = dict(method="gmres", precond_r="fsai_lu", rtol=1e-13, atol=1e-15, posdef=True)
    outs = []
    for kw in (dict(bck_options=dict(opts), **opts), dict(method="exactsolve")):
        v = torch.as_tensor(vals).clone().requires_grad_()
        b = b0.clone().requires_grad_()
        A = SparseLinearOperator(crow_t, col_t, v, (m * m, m * m))
        x = solve(A, b, **kw)
        outs.append((x.detach(), *torch.autograd.grad((x ** 2).sum(), (v, b))))
    (x1, gv1, gb1), (x0, gv0, gb0) = outs
    assert torch.allclose(x1, x0, rtol=1e-9, atol=1e-11)
    assert torch.allclose(gv1, gv0, rtol=1e-8, atol=1e-10)
    assert torch.allclose(gb1, gb0, rtol=1e-8, atol=1e-10)


def test_backward_builds_the_adjoint_twin(problem, monkeypatch):
    """the backward solve arrives with A.H (an AdjointLinearOperator of the sparse A): its named preconditioner is
    fsai_lu(A).H, an FSAILUOperator with the adjoint flag set, not an AdjointLinearOperator"""
    from xitorch_amd.linalg import precond as pm
    A, Ad, B = problem
    P = pm.named_preconditioner("fsai_lu", A.H, "gmres")
    assert isinstance(P, FSAILUOperator) and P.adjoint
    Pf = pm.named_preconditioner("fsai_lu", A, "bicgstab")
    assert isinstance(Pf, FSAILUOperator) and not Pf.adjoint
    eye = torch.eye(N, dtype=F64)
    assert torch.equal(P.mm(eye), Pf.rmm(eye))


@pytest.mark.parametrize("cplx", [False, True])
def test_adjoint_operator(cplx):
    Ad = lc.convdiff_complex(8, 0.5) if cplx else lc.convdiff(8, 0.5)
    A = lc.operator_of_dense(Ad)
    P = fsai_lu(A, power=2)
    assert not P.is_hermitian and P._getparamnames() == [] and isinstance(P.H, FSAILUOperator)
    assert P.H.GL is P.GL and P.H.W is P.W and P.H.adjoint and not P.H.H.adjoint
    GL, GU = lc.factors_dense(P)
    Pd = GU[0] @ GL[0]
    X = torch.as_tensor(np.random.default_rng(2).standard_normal((64, 3)).astype(Ad.dtype))
    tol = 64 * torch.finfo(torch.float64).eps * np.abs(GU[0]).sum(1).max() * np.abs(GL[0]).sum(1).max() * 8
    assert np.abs(P.mm(X).numpy() - Pd @ X.numpy()).max() <= tol
    assert np.abs(P.H.mm(X).numpy() - np.conj(Pd.T) @ X.numpy()).max() <= tol
    assert np.abs(P.rmm(X).numpy() - np.conj(Pd.T) @ X.numpy()).max() <= tol
    assert np.abs(P.H.rmm(X).numpy() - Pd @ X.numpy()).max() <= tol
    assert np.abs(P.mv(X[:, 0]).numpy() - Pd @ X[:, 0].numpy()).max() <= tol


def test_refusals(problem):
    A, Ad, B = problem
    dense = LinearOperator.m(torch.as_tensor(Ad), is_hermitian=False)
    with pytest.raises(TypeError, match="SparseLinearOperator"):
        solve(dense, B, method="gmres", precond_r="fsai_lu")
    with pytest.raises(TypeError, match="SparseLinearOperator"):
        solve(dense, B, method="bicgstab", precond_l="fsai_lu")
    with pytest.raises(TypeError, match="unknown preconditioner name"):
        solve(A, B, method="gmres", precond_r="fsai")
    with pytest.raises(TypeError, match="unknown preconditioner name"):
        solve(A, B, method="cg", precond="fsai_lu")
    with pytest.raises(ValueError, match="normal equations"):
        host_krylov.gmres(A, B, posdef=False, precond_r=fsai_lu(A))
    with pytest.raises(TypeError, match="LinearOperator"):
        host_krylov.gmres(A, B, posdef=True, precond_r=torch.eye(N, dtype=F64))
    with pytest.raises(TypeError, match="SparseLinearOperator"):
        fsai_lu(dense)
    with pytest.raises(ValueError, match="max_row"):
        fsai_lu(A, max_row=33)
    with pytest.raises(ValueError, match="power"):
        fsai_lu(A, power=0)


def test_without_the_option_nothing_changes(problem, monkeypatch):
    """gmres(precond_r=None) returns the bits of the call without the option.  The host driver hands its small
    least-squares problem to torch.linalg.lstsq, and that library call does not return the same bits for the same input
    from one call to the next (31 x 30 doubles, one thread: seen here before this option existed), so two runs of the
    unchanged driver already differ in the last bits.  The test therefore answers a repeated least-squares input with
    the first answer it got: what is left to compare is the driver's own arithmetic, and that must not change."""
    A, Ad, B = problem
    real_lstsq, seen = torch.linalg.lstsq, {}

    def lstsq_once(H, g, *a, **k):
        key = (H.shape, H.numpy().tobytes(), g.numpy().tobytes())
        if key not in seen:
            seen[key] = real_lstsq(H, g, *a, **k)
        return seen[key]
    monkeypatch.setattr(torch.linalg, "lstsq", lstsq_once)
    kw = dict(rtol=1e-8, atol=0.0, posdef=True, restart=30, resid_calc_every=3)
    assert torch.equal(host_krylov.gmres(A, B, precond_r=None, **kw), host_krylov.gmres(A, B, **kw))
    hits = len(seen)
    assert torch.equal(solve(A, B, method="gmres", precond_r=None, **kw), solve(A, B, method="gmres", **kw))
    assert len(seen) == hits, "the same least-squares problems, bit for bit, in all four runs"
