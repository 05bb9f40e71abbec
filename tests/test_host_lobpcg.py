"""CPU: the host twin of LOBPCG (`host_eig.lobpcg`, reached through `symeig(method="lobpcg")` on operators in host
memory) against torch.linalg.eigh — every pair's residual, M-orthonormality and eigenvalue, none left out.  The cap
is 300 iterations: a prototype of the algorithm needed 0 .. 79 for these cases, so one that needs more is a bug."""
import warnings
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd.linalg import symeig, svd, fsai
from xitorch_amd.linalg import host_eig
from xitorch_amd.linalg.native_eig import GUARD_BAD
from tests import chebfsi_cases as cc
from tests import lobpcg_cases as lc

CPU = torch.device("cpu")
f64 = torch.float64


def run(op, neig, mode, dtype, M=None, **kw):
    tr = {}
    n0 = host_eig.calls["lobpcg"]
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        ev, X = symeig(op, neig, mode, M=M, method="lobpcg", min_eps=lc.min_eps(dtype), max_niter=lc.MAX_NITER,
                       trace=tr, **kw)
    assert host_eig.calls["lobpcg"] == n0 + 1
    assert tr["niter"] <= lc.MAX_NITER and tr["best_resid"] < lc.min_eps(dtype)
    print("niter %d napply %d best %.2e restarts %d redraws %d" % (tr["niter"], tr["napply"], tr["best_resid"],
                                                                  tr["restarts"], tr["redraws"]))
    return ev, X, tr


@pytest.mark.parametrize("dtype", lc.DTYPES, ids=lc.IDS)
@pytest.mark.parametrize("mode", ["lowest", "uppest"])
@pytest.mark.parametrize("neig", [1, 4, 6])
def test_dense(dtype, mode, neig):
    A, lam = cc.dense_case(dtype, (), lc.N)
    ev, X, tr = run(xa.LinearOperator.m(A, True), neig, mode, dtype)
    lc.assert_pairs(A, None, ev, X, neig, mode, dtype)
    assert tr["w"] == neig + max(2, -(-neig // 4)) and tr["napply"] == tr["niter"] + 1 + tr["restarts"]


@pytest.mark.parametrize("batch", [(3,), (2, 2)], ids=["b3", "b2x2"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.complex64], ids=["f64", "c64"])
def test_batch_with_three_spectra(batch, dtype):
    A, lam = cc.dense_case(dtype, batch, lc.N, spectrum=lc.batch_spectra(batch))
    ev, X, _ = run(xa.LinearOperator.m(A, True), 4, "lowest", dtype)
    assert ev.shape == (*batch, 4)
    lc.assert_pairs(A, None, ev, X, 4, "lowest", dtype)


@pytest.mark.parametrize("dtype", lc.DTYPES, ids=lc.IDS)
@pytest.mark.parametrize("mode", ["lowest", "uppest"])
def test_generalised(dtype, mode):
    A, _ = cc.dense_case(dtype, (), 196)
    M = lc.overlap_matrix(14, dtype)
    ev, X, _ = run(xa.LinearOperator.m(A, True), 4, mode, dtype, M=xa.LinearOperator.m(M, True))
    lc.assert_pairs(A, M, ev, X, 4, mode, dtype)


@pytest.mark.parametrize("dtype", lc.DTYPES, ids=lc.IDS)
@pytest.mark.parametrize("precond", ["none", "diag", "tensor"])
def test_diagonally_dominant(dtype, precond):
    A = lc.dominant_matrix(dtype)
    pc = {"none": None, "diag": "diag", "tensor": torch.diagonal(A).real.clone()}[precond]
    ev, X, tr = run(xa.LinearOperator.m(A, True), 4, "lowest", dtype, precond=pc)
    lc.assert_pairs(A, None, ev, X, 4, "lowest", dtype)
    if precond != "none" and lc.REAL_OF[dtype] == f64:
        assert tr["niter"] < 40           # the diagonal is nearly the operator: far fewer steps than without


def test_generalised_with_diagonal_preconditioner():
    A = lc.dominant_matrix(f64, n=196)
    M = lc.overlap_matrix(14, f64)
    ev, X, _ = run(xa.LinearOperator.m(A, True), 4, "lowest", f64, M=xa.LinearOperator.m(M, True), precond="diag")
    lc.assert_pairs(A, M, ev, X, 4, "lowest", f64)


@pytest.mark.parametrize("kind,precond", [("sparse", False), ("sparse", True), ("banded", False), ("mv", False)],
                         ids=["csr", "csr-fsai", "banded", "mv"])
def test_grid_with_double_eigenvalues(kind, precond):
    """the 5-point matrix on 16 x 16: eigenvalues and residuals, never vectors"""
    A = lc.grid_matrix(16)
    op = lc.operator_of(kind, A, CPU)
    ev, X, tr = run(op, 6, "lowest", f64, precond=fsai(op) if precond else None)
    lc.assert_pairs(A, None, ev, X, 6, "lowest", f64)
    lam, _ = lc.reference_spectrum(A)
    assert abs(float(lam[1] - lam[2])) < 1e-12 and abs(float(ev[1] - ev[2])) < 1e-6     # the double pair, found twice


def test_v0_with_three_exact_eigenvectors_of_four():
    A, lam, Q = cc.dense_case(f64, (), lc.N, with_vectors=True)
    ev, X, tr = run(xa.LinearOperator.m(A, True), 4, "lowest", f64, V0=Q[:, :3])
    lc.assert_pairs(A, None, ev, X, 4, "lowest", f64)
    assert tr["w"] == 6


def test_exact_v0_converges_in_zero_iterations():
    A, lam, Q = cc.dense_case(f64, (), lc.N, with_vectors=True)
    ev, X, tr = run(xa.LinearOperator.m(A, True), 4, "lowest", f64, V0=Q[:, :6])
    assert tr["niter"] == 0 and tr["napply"] == 1 and len(tr["resid_history"]) == 1
    lc.assert_pairs(A, None, ev, X, 4, "lowest", f64)


def test_diagonal_operator():
    A = torch.diag(torch.arange(1, lc.N + 1, dtype=f64))
    for pc in (None, "diag"):
        ev, X, _ = run(xa.LinearOperator.m(A, True), 4, "lowest", f64, precond=pc)
        lc.assert_pairs(A, None, ev, X, 4, "lowest", f64)


def test_clustered_spectrum():
    A, lam = cc.dense_case(f64, (), lc.N, spectrum=lc.cluster_spectrum())
    ev, X, _ = run(xa.LinearOperator.m(A, True), 6, "lowest", f64)
    lc.assert_pairs(A, None, ev, X, 6, "lowest", f64)


def test_two_iterations_warn_and_return_the_best_block():
    A, lam = cc.dense_case(f64, (), lc.N)
    tr = {}
    with pytest.warns(xa.ConvergenceWarning):
        ev, X = symeig(xa.LinearOperator.m(A, True), 4, "lowest", method="lobpcg", min_eps=1e-10, max_niter=2, trace=tr)
    assert tr["niter"] == 2 and tr["best_resid"] >= 1e-10 and len(tr["resid_history"]) == 3
    assert bool(torch.isfinite(ev).all()) and bool(torch.isfinite(X).all())
    R = A @ X - X * ev.unsqueeze(-2)
    assert abs(float(R.abs().max()) - tr["best_resid"]) <= 1e-12 and tr["best_resid"] == min(tr["resid_history"])
    assert float((X.T @ X - torch.eye(4, dtype=f64)).abs().max()) <= GUARD_BAD[f64]


def test_refusals_and_hand_over():
    A, lam = cc.dense_case(f64, (), lc.N)
    op = xa.LinearOperator.m(A, True)
    with pytest.raises(NotImplementedError):
        symeig(op, 4, "lowest", method="lobpcg", process_group=object())
    with pytest.raises(NotImplementedError, match="chebfsi"):
        symeig(op, 30, "lowest", method="lobpcg")                       # w = 38: 3 w beyond the rotation kernel's rows
    with pytest.raises(RuntimeError, match="Unknown lobpcg preconditioner"):
        symeig(op, 4, "lowest", method="lobpcg", precond="davidson")    # davidson's shifted form: not reinterpreted
    small, lam_s = cc.dense_case(f64, (), 24)
    tr = {}
    ev, X = symeig(xa.LinearOperator.m(small, True), 4, "lowest", method="lobpcg", trace=tr)   # N <= 5 w
    assert tr["handed_to"] == "exacteig" and float((ev - lam_s[:4]).abs().max()) < 1e-10


def test_dependent_start_vectors_are_redrawn():
    A, lam, Q = cc.dense_case(f64, (), lc.N, with_vectors=True)
    V0 = torch.randn(lc.N, 6, dtype=f64, generator=torch.Generator().manual_seed(2))
    V0[:, 3] = V0[:, 1]                                                   # two identical columns
    ev, X, tr = run(xa.LinearOperator.m(A, True), 4, "lowest", f64, V0=V0)
    assert tr["redraws"] + tr["restarts"] > 0
    lc.assert_pairs(A, None, ev, X, 4, "lowest", f64)


def test_cholesky_flag_of_the_new_directions_redraws_them_once(monkeypatch):
    """a Cholesky flag while W is orthonormalised (forced: the third factorisation of the run, the first of W): W is
    redrawn and orthonormalised with three passes, the run goes on; a second failure in the same step raises"""
    A, lam = cc.dense_case(f64, (), lc.N)
    real, ncall = torch.linalg.cholesky_ex, [0]

    def failing(fail_on):
        def chol(G, **kw):
            L, info = real(G, **kw)
            ncall[0] += 1
            return (L, torch.ones_like(info)) if ncall[0] in fail_on else (L, info)
        return chol
    monkeypatch.setattr(torch.linalg, "cholesky_ex", failing({3}))
    ev, X, tr = run(xa.LinearOperator.m(A, True), 4, "lowest", f64)
    assert tr["redraws"] == tr["w"] and tr["restarts"] == 0
    lc.assert_pairs(A, None, ev, X, 4, "lowest", f64)
    ncall[0] = 0
    monkeypatch.setattr(torch.linalg, "cholesky_ex", failing({3, 5}))
    with pytest.raises(RuntimeError, match="could not be orthonormalised"):
        symeig(xa.LinearOperator.m(A, True), 4, "lowest", method="lobpcg", min_eps=1e-8, max_niter=lc.MAX_NITER)


def test_backward_matches_exacteig():
    """N = 40, neig = 3 (w = 5), float64, 1e-6 relative, as the symeig gradient tests"""
    g = torch.Generator().manual_seed(7)
    A0, _ = cc.dense_case(f64, (), 40)
    W = torch.randn(40, 3, dtype=f64, generator=g)
    grads = {}
    for meth, kw in (("lobpcg", dict(min_eps=1e-10, max_niter=lc.MAX_NITER)), ("exacteig", {})):
        Ap = A0.clone().requires_grad_()
        tr = {}
        ev, X = symeig(xa.LinearOperator.m(Ap, True), 3, "lowest", method=meth, **(dict(kw, trace=tr) if kw else {}))
        assert meth == "exacteig" or "handed_to" not in tr
        # (a loss that does not depend on the sign of the eigenvectors)
        loss = (ev * torch.arange(1, 4, dtype=f64)).sum() + ((X * W).sum(0) ** 2).sum()
        grads[meth], = torch.autograd.grad(loss, Ap)
    ga, gb = grads["lobpcg"], grads["exacteig"]
    ga, gb = (ga + ga.T) * 0.5, (gb + gb.T) * 0.5
    assert float((ga - gb).abs().max()) <= 1e-6 * float(gb.abs().max())


def test_svd_through_lobpcg():
    A = torch.randn(60, 40, dtype=f64, generator=torch.Generator().manual_seed(11))
    u, s, vh = svd(xa.LinearOperator.m(A), 3, method="lobpcg", min_eps=1e-10, max_niter=lc.MAX_NITER)
    want = torch.linalg.svdvals(A)[:3]
    assert float((s.sort(descending=True)[0] - want).abs().max()) <= 1e-8 * float(want[0])


def test_symeig_reaches_the_same_function_as_the_direct_call():
    import sys
    from xitorch_amd.linalg import native_lobpcg
    assert sys.modules["xitorch_amd.linalg.symeig"]._SYMEIG_METHODS["lobpcg"] is native_lobpcg.lobpcg
    A, lam = cc.dense_case(f64, (), lc.N)
    op = xa.LinearOperator.m(A, True)
    ev1, X1 = symeig(op, 4, "lowest", method="lobpcg", min_eps=1e-8, max_niter=lc.MAX_NITER)
    ev2, X2 = native_lobpcg.lobpcg(op, 4, "lowest", min_eps=1e-8, max_niter=lc.MAX_NITER)
    assert torch.equal(ev1, ev2) and torch.equal(X1, X2)
