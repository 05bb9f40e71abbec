"""CPU: `host_eig.chebfsi`, the torch-op statement of the Chebyshev-filtered subspace iteration, through
`symeig(method="chebfsi")` on operators in host memory.  (The method does not exist on the parent commit.)

Operators are Q diag(lam) Q^H with a known spectrum whose gaps are >= 1 at the wanted end, so pairs match by order.
Asserted for ALL pairs: max|A x - lam x| < min_eps recomputed in float64 / complex128, max|X^H X - I| <= GUARD_BAD,
|lam_hat - lam| <= sqrt(N) min_eps + 64 eps |A|_2 (Bauer-Fike for Hermitian operators, the residual's 2-norm bounded
by sqrt(N) times its largest entry).

min_eps: 1e-8 for the 64-bit dtypes; for the 32-bit ones 4x the largest max|resid| the host twin was measured to reach on
these cases (4.2e-5, the figures are beside MEASURED32 in tests/chebfsi_cases.py): 1.68e-4.  The margin covers the
different summation order of the device kernels.
"""
import warnings
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd.linalg import symeig
from xitorch_amd.linalg import host_eig
from xitorch_amd.linalg.native_eig import GUARD_BAD
from tests import chebfsi_cases as cc

DTYPES = cc.DTYPES
IDS = cc.IDS


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("neig", [1, 6, 24])
@pytest.mark.parametrize("mode", ["lowest", "uppest"])
def test_known_spectrum_dense(dtype, neig, mode):
    A, lam = cc.dense_case(dtype, (), cc.N)
    tr = {}
    ev, X = symeig(xa.LinearOperator.m(A, True), neig, mode, method="chebfsi", min_eps=cc.min_eps(dtype), trace=tr)
    cc.assert_pairs(A, lam, ev, X, neig, mode, dtype)
    assert tr["w"] == neig + max(8, -(-neig // 4)) and tr["niter"] >= 1 and tr["napply"] > tr["niter"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_batch_2x3_with_a_broadcast_dimension(dtype):
    A, lam = cc.dense_case(dtype, (2, 1), cc.N)
    Ab = A.expand(2, 3, cc.N, cc.N)
    ev, X = symeig(xa.LinearOperator.m(Ab, True), 6, "lowest", method="chebfsi", min_eps=cc.min_eps(dtype))
    assert ev.shape == (2, 3, 6) and X.shape == (2, 3, cc.N, 6)
    cc.assert_pairs(Ab, lam.expand(2, 3, cc.N), ev, X, 6, "lowest", dtype)


KIND_CASES = [(k, d) for k in ("banded", "sparse", "mv") for d in DTYPES]


@pytest.mark.parametrize("kind,dtype", KIND_CASES, ids=["%s-%s" % (k, IDS[DTYPES.index(d)]) for k, d in KIND_CASES])
def test_operator_kinds(kind, dtype):
    op, A, lam = cc.operator_case(kind, dtype, torch.device("cpu"))
    ev, X = symeig(op, 6, "lowest", method="chebfsi", min_eps=cc.min_eps(dtype))
    cc.assert_pairs(A, lam, ev, X, 6, "lowest", dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128], ids=["f64", "c128"])
def test_clustered_pair_inside_the_block(dtype):
    """two wanted eigenvalues 1e-3 apart: residual and orthonormality only (the vectors of a cluster are not unique)"""
    spec = torch.arange(cc.N, dtype=torch.float64)
    spec[3] = spec[2] + 1e-3
    A, lam = cc.dense_case(dtype, (), cc.N, spectrum=spec)
    ev, X = symeig(xa.LinearOperator.m(A, True), 6, "lowest", method="chebfsi", min_eps=1e-8)
    cc.assert_residual_and_orthonormality(A, ev, X, 1e-8, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_zero_operator(dtype):
    A = torch.zeros(cc.N, cc.N, dtype=dtype)
    ev, X = symeig(xa.LinearOperator.m(A, True), 4, "lowest", method="chebfsi", min_eps=cc.min_eps(dtype))
    assert float(ev.abs().max()) <= cc.eigenvalue_bound(cc.N, cc.min_eps(dtype), dtype, 0.0)
    cc.assert_residual_and_orthonormality(A, ev, X, cc.min_eps(dtype), dtype)


def test_block_as_wide_as_the_space_is_handed_to_exacteig():
    A, lam = cc.dense_case(torch.float64, (), 40)
    tr = {}
    ev, X = symeig(xa.LinearOperator.m(A, True), 32, "lowest", method="chebfsi", trace=tr)       # w = 32 + 8 = N
    assert tr["handed_to"] == "exacteig" and tr["w"] == 40 and tr["napply"] == 0
    ev2, X2 = symeig(xa.LinearOperator.m(A, True), 32, "lowest", method="exacteig")
    assert torch.equal(ev, ev2) and torch.equal(X, X2)


def test_overlap_operator_and_process_group_raise():
    A, _ = cc.dense_case(torch.float64, (), cc.N)
    op = xa.LinearOperator.m(A, True)
    Mop = xa.LinearOperator.m(torch.eye(cc.N, dtype=torch.float64), True)
    with pytest.raises(NotImplementedError, match="davidson"):
        symeig(op, 3, "lowest", M=Mop, method="chebfsi")
    with pytest.raises(NotImplementedError, match="davidson"):
        symeig(op, 3, "lowest", method="chebfsi", process_group=object())


def test_start_block_is_honoured():
    """the exact invariant subspace as V0: converged at the first Rayleigh-Ritz"""
    A, lam, Q = cc.dense_case(torch.float64, (), cc.N, with_vectors=True)
    tr = {}
    ev, X = symeig(xa.LinearOperator.m(A, True), 6, "lowest", method="chebfsi", min_eps=1e-8, V0=Q[:, :14], trace=tr)
    assert tr["niter"] == 1 and tr["w"] == 14
    cc.assert_pairs(A, lam, ev, X, 6, "lowest", torch.float64)
    # a narrower V0 is completed by random columns, a wider one widens the block
    tr = {}
    symeig(xa.LinearOperator.m(A, True), 6, "lowest", method="chebfsi", min_eps=1e-8, V0=Q[:, :3], trace=tr)
    assert tr["w"] == 14
    tr = {}
    symeig(xa.LinearOperator.m(A, True), 6, "lowest", method="chebfsi", min_eps=1e-8, V0=Q[:, :20], trace=tr)
    assert tr["w"] == 20 and tr["niter"] == 1


def test_one_iteration_on_a_hard_spectrum_warns_and_returns_the_best_block():
    spec = 1.0 + torch.arange(cc.N, dtype=torch.float64) * 1e-3          # relative gaps of 1e-3
    A, lam = cc.dense_case(torch.float64, (), cc.N, spectrum=spec)
    tr = {}
    with pytest.warns(xa.ConvergenceWarning):
        ev, X = symeig(xa.LinearOperator.m(A, True), 6, "lowest", method="chebfsi", min_eps=1e-10, max_niter=1, trace=tr)
    assert tr["niter"] == 1 and tr["best_resid"] >= 1e-10
    Ad = A.to(torch.float64)
    R = Ad @ X - X * ev.unsqueeze(-2)
    assert abs(float(R.abs().max()) - tr["best_resid"]) <= 1e-12
    assert float((X.T @ X - torch.eye(6, dtype=torch.float64)).abs().max()) <= GUARD_BAD[torch.float64]


def test_backward_matches_exacteig():
    """N = 40, neig = 3 (nguard = 8: w = 11), float64, 1e-6 relative, as the symeig gradient tests"""
    g = torch.Generator().manual_seed(7)
    A0, _ = cc.dense_case(torch.float64, (), 40)
    W = torch.randn(40, 3, dtype=torch.float64, generator=g)
    grads = {}
    for meth, kw in (("chebfsi", dict(min_eps=1e-10)), ("exacteig", {})):
        Ap = A0.clone().requires_grad_()
        ev, X = symeig(xa.LinearOperator.m(Ap, True), 3, "lowest", method=meth, **kw)
        # (a loss that does not depend on the sign of the eigenvectors)
        loss = (ev * torch.arange(1, 4, dtype=torch.float64)).sum() + ((X * W).sum(0) ** 2).sum()
        grads[meth], = torch.autograd.grad(loss, Ap)
    ga, gb = grads["chebfsi"], grads["exacteig"]
    ga, gb = (ga + ga.T) * 0.5, (gb + gb.T) * 0.5
    assert float((ga - gb).abs().max()) <= 1e-6 * float(gb.abs().max())


def test_symeig_reaches_the_same_function_as_the_direct_call(monkeypatch):
    import sys
    from xitorch_amd.linalg import native_chebfsi
    symeig_mod = sys.modules["xitorch_amd.linalg.symeig"]
    assert symeig_mod._SYMEIG_METHODS["chebfsi"] is native_chebfsi.chebfsi
    A, lam = cc.dense_case(torch.float64, (), cc.N)
    op = xa.LinearOperator.m(A, True)
    n0 = host_eig.calls["chebfsi"]
    ev1, X1 = symeig(op, 6, "lowest", method="chebfsi", min_eps=1e-8)
    ev2, X2 = native_chebfsi.chebfsi(op, 6, "lowest", min_eps=1e-8)
    assert host_eig.calls["chebfsi"] == n0 + 2
    assert torch.equal(ev1, ev2) and torch.equal(X1, X2)
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        xa.linalg.lsymeig(op, 6, method="chebfsi", min_eps=1e-8)
