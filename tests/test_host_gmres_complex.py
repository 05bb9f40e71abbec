"""solve(method="gmres") on COMPLEX operators in host memory (host_krylov.gmres): dense non-Hermitian, CSR and generic
`_mv` operators in complex128 and complex64, with E and M, batch dims with broadcasting, restart=, resid_calc_every=,
the zero right-hand side, a non-converging run, and the implicit backward through bck_options={"method": "gmres"}.

Two checks (tests/gmres_complex_cases.py): the method's own rule on the returned x, recomputed in complex128 with a
derived slack; and `trace["arnoldi_steps"]` EQUAL to a textbook complex128 MGS-GMRES on cases whose textbook residuals at
the crossing step and the step before are each a factor 2 away from the threshold."""
import warnings
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd.linalg import solve, host_krylov
from tests import gmres_complex_cases as C

DEV = "cpu"


def _solve(case, data, device=DEV, **kw):
    Aop, B, E, Mop = C.operators(case, data, device)
    tr = {}
    X = solve(Aop, B, E, Mop, method="gmres", posdef=True, trace=tr, **kw)
    return X, tr


@pytest.mark.parametrize("case", C.RULE_CASES, ids=[c["name"] for c in C.RULE_CASES])
def test_rule(case):
    data = C.make(case)
    rt, at = C.RTOL[case["dtype"]], C.ATOL[case["dtype"]]
    before = host_krylov.calls["gmres"]
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        X, tr = _solve(case, data, rtol=rt, atol=at)
    assert host_krylov.calls["gmres"] == before + 1
    assert X.dtype == case["dtype"] and tr["converged"]
    bshape = torch.broadcast_shapes(data["A"].shape[:-2], data["B"].shape[:-2],
                                    () if data["E"] is None else data["E"].shape[:-1])
    assert tuple(X.shape) == (*bshape, case["n"], data["B"].shape[-1])
    r, lim = C.residual_rule(case, data, X, rt, at)
    print("%s: max |r| / limit %.3f, steps %d" % (case["name"], float((r / lim).max()), tr["arnoldi_steps"]))
    assert bool((r <= lim).all())


@pytest.mark.parametrize("case", C.STEP_CASES, ids=[c["name"] for c in C.STEP_CASES])
def test_step_cases_meet_the_factor_2(case):
    steps, ok = C.textbook_steps(case, C.make(case), case["rtol"], C.STEP_ATOL)
    assert ok and steps == case["steps"]


def test_enough_step_cases():
    assert len(C.STEP_CASES) >= 8


@pytest.mark.parametrize("case", C.STEP_CASES, ids=[c["name"] for c in C.STEP_CASES])
def test_arnoldi_steps_equal_the_textbook(case):
    data = C.make(case)
    steps, ok = C.textbook_steps(case, data, case["rtol"], C.STEP_ATOL)
    assert ok
    X, tr = _solve(case, data, rtol=case["rtol"], atol=C.STEP_ATOL)
    assert tr["converged"] and tr["arnoldi_steps"] == steps
    r, lim = C.residual_rule(case, data, X, case["rtol"], C.STEP_ATOL)
    assert bool((r <= lim).all())


@pytest.mark.parametrize("name", ["dense_c128", "csr_c64", "dense_EM_c128"])
def test_restart(name):
    case = next(c for c in C.RULE_CASES if c["name"] == name)
    data = C.make(case)
    rt, at = C.RTOL[case["dtype"]], C.ATOL[case["dtype"]]
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        X, tr = _solve(case, data, rtol=rt, atol=at, restart=7, max_niter=400)
    assert tr["converged"] and tr["restarts"] >= 1
    r, lim = C.residual_rule(case, data, X, rt, at)
    assert bool((r <= lim).all())


@pytest.mark.parametrize("name", ["dense_c128", "mv_c64", "csr_E_c128"])
def test_resid_calc_every(name):
    case = next(c for c in C.RULE_CASES if c["name"] == name)
    data = C.make(case)
    rt, at = C.RTOL[case["dtype"]], C.ATOL[case["dtype"]]
    X1, tr1 = _solve(case, data, rtol=rt, atol=at)
    X5, tr5 = _solve(case, data, rtol=rt, atol=at, resid_calc_every=5)
    assert tr5["converged"] and tr5["napply"] < tr1["napply"]
    r, lim = C.residual_rule(case, data, X5, rt, at)
    assert bool((r <= lim).all())


@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64])
def test_zero_rhs(dtype):
    case = dict(kind="dense", dtype=dtype, n=20, seed=50, ncols=2)
    data = C.make(case)
    data["B"] = torch.zeros_like(data["B"])
    X, tr = _solve(case, data)
    assert X.dtype == dtype and tuple(X.shape) == (20, 2) and bool((X == 0).all()) and tr == {}


def test_not_converged_returns_the_best_iterate_with_a_warning():
    case = dict(kind="dense", dtype=torch.complex128, n=48, seed=1)
    data = C.make(case)
    with pytest.warns(xa.ConvergenceWarning):
        X, tr = _solve(case, data, rtol=1e-12, atol=1e-30, max_niter=6)
    assert not tr["converged"] and tr["arnoldi_steps"] == 5
    # the best iterate: its residual is the recorded best, and it beats x0 = 0
    r, _ = C.residual_rule(case, data, X, 0.0, 0.0)
    bn = torch.linalg.vector_norm(data["B"], dim=-2)
    assert abs(float(r.max()) - tr["best_resid"]) <= 1e-12 * float(bn.max()) and bool((r < bn).all())


def test_backward_gradcheck_through_gmres():
    g = torch.Generator().manual_seed(60)
    n = 6
    A0 = (0.3 * C._crand(g, n, n) + torch.eye(n, dtype=torch.complex128) * (2.0 + 0.5j)).requires_grad_()
    B0 = C._crand(g, n, 2).requires_grad_()
    E0 = (0.1 * C._crand(g, 2)).requires_grad_()
    # (un-restarted, at most n - 1 Krylov vectors contribute, like the reference's loop: GMRES(n) lifts that cap)
    opts = dict(method="gmres", posdef=True, rtol=1e-13, atol=1e-30, restart=n, max_niter=60)

    def f(A, B, E):
        return solve(xa.LinearOperator.m(A, is_hermitian=False), B, E, bck_options=dict(opts), **opts)
    before = host_krylov.calls["gmres"]
    # (nondet_tol: the adjoint solve is iterative and stops at rtol = 1e-13 — two backward runs agree to the solver's
    # tolerance times the conditioning, not bit for bit)
    assert torch.autograd.gradcheck(f, (A0, B0, E0), eps=1e-6, atol=1e-6, rtol=1e-5, nondet_tol=1e-10)
    assert host_krylov.calls["gmres"] > before + 1          # forward and adjoint solves both ran GMRES
