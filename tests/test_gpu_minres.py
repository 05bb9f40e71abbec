"""-m gpu: the native MINRES driver (native_krylov.minres on the xk_minres_* kernels) through `solve(method="minres")`
on MatrixLinearOperator, BandedLinearOperator and SparseLinearOperator (real and complex values), with and without
E, M and precond.

Criterion (the package's Krylov bar): |X - X_ref| <= 2 rtol kappa |X_ref| against a float64 / complex128 dense solve
of the operator's own full matrix.  For f64 / c128 the iteration count is within +-1 of the restated iteration
(tests/minres_ref.py::iterate) on the same input; `resid_history` never grows; two runs are bit-identical; no host
driver runs; on real indefinite input the answer agrees with native gmres.  fp32: kappa <= 100, rtol = 1e-4.
tests/test_minres_ref.py::test_solver_inputs_meet_the_criterion_on_the_restated_iteration shows on the CPU that the
inputs below are solvable to that criterion by the restated iteration alone."""
import warnings
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd.linalg import host_krylov, solve, symeig
from tests import minres_ref as mref
from tests.test_minres_ref import singular_case, singular_drift

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F64 = torch.float64
HP = {torch.float64: torch.float64, torch.float32: torch.float64,
      torch.complex128: torch.complex128, torch.complex64: torch.complex128}
RTOL = {torch.float64: 1e-9, torch.complex128: 1e-9, torch.float32: 1e-4, torch.complex64: 1e-4}


def _randn(g, shape, dtype):
    if dtype.is_complex:
        return torch.complex(torch.randn(shape, dtype=F64, generator=g), torch.randn(shape, dtype=F64, generator=g))
    return torch.randn(shape, dtype=F64, generator=g)


# ------------------------------------------------------------------------------------------------ inputs (host, hp)
def dense_input(dtype, seed=1, B=2, n=300):
    """batch of dense Hermitian operators shifted into the spectrum: eigenvalues in +-[1, 5] (kappa = 5), a
    quarter of them negative.  kappa is kept small against the order on purpose: the iteration count is compared
    with the restated iteration to +-1, which only means something while convergence is governed by the residual
    polynomial (about kappa ln(2 / rtol) steps, well below n) and not by the exhaustion of the Krylov space near
    step n, where the loss of orthogonality of the Lanczos vectors -- rounding noise, different for every summation
    order -- decides the step (tests/test_minres_ref.py asserts niter < n / 2 for all inputs of this file)."""
    g = torch.Generator().manual_seed(seed)
    ev = torch.linspace(1.0, 5.0, n, dtype=F64)
    ev[::4] *= -1
    A = torch.stack([mref.hermitian(g, dtype, n, ev)[0] for _ in range(B)])
    return A, _randn(g, (B, n, 2), dtype), 5.0


def banded_input(dtype, seed=2, B=2, n=1501, hb=3):
    """DIA band (B, 2 hb + 1, n) of a symmetric indefinite matrix: diagonal of alternating sign and modulus in
    [1, 3], off-diagonals 0.05 randn (Gershgorin keeps |lambda| in about [0.5, 3.5])"""
    g = torch.Generator().manual_seed(seed)
    band = torch.zeros(B, 2 * hb + 1, n, dtype=F64)
    d = 1.0 + 2.0 * torch.rand(B, n, dtype=F64, generator=g)
    d[:, ::3] *= -1
    band[:, hb] = d
    for j in range(1, hb + 1):
        o = 0.05 * torch.randn(B, n - j, dtype=F64, generator=g)
        band[:, hb + j, :n - j] = o                     # A[i, i + j]
        band[:, hb - j, j:] = o                         # A[i + j, i]
    return band, _randn(g, (B, n, 2), dtype)


def banded_full(band):
    """dense (B, n, n) matrix of a DIA band: band[b, d, i] = A_b[i, i + d - hb]"""
    B, nd, n = band.shape
    hb = nd // 2
    A = torch.zeros(B, n, n, dtype=band.dtype)
    for d in range(nd):
        off = d - hb
        i = torch.arange(max(0, -off), min(n, n - off))
        A[:, i, i + off] = band[:, d, i]
    return A


def laplacian_input(dtype, m=8, seed=3):
    """7-point Laplacian of an m^3 grid (complex: with a Peierls phase on the x hops, Hermitian), and a shift in the
    middle of the widest gap between two neighbouring eigenvalues among the lowest 40"""
    n = m ** 3
    hp = HP[dtype]
    A = torch.zeros(n, n, dtype=hp)
    idx = lambda i, j, k: (i * m + j) * m + k
    ph = torch.polar(torch.tensor(1.0, dtype=F64), torch.tensor(0.37, dtype=F64)) if dtype.is_complex else 1.0
    for i in range(m):
        for j in range(m):
            for k in range(m):
                a = idx(i, j, k)
                A[a, a] = 6.0
                if i + 1 < m:
                    A[a, idx(i + 1, j, k)] = -ph
                    A[idx(i + 1, j, k), a] = -(ph.conj() if dtype.is_complex else ph)
                if j + 1 < m:
                    A[a, idx(i, j + 1, k)] = A[idx(i, j + 1, k), a] = -1.0
                if k + 1 < m:
                    A[a, idx(i, j, k + 1)] = A[idx(i, j, k + 1), a] = -1.0
    lam = torch.linalg.eigvalsh(A)
    gaps = lam[1:41] - lam[:40]
    i = int(gaps.argmax())
    sigma = float((lam[i] + lam[i + 1]) / 2)
    kappa = float((lam - sigma).abs().max() / (lam - sigma).abs().min())
    g = torch.Generator().manual_seed(seed)
    return A, sigma, kappa, _randn(g, (n, 2), dtype)


# ------------------------------------------------------------------------------------------------ helpers
def _reference(Afull, B, E=None, Mfull=None):
    """dense solve in float64 / complex128, column by column when shifted; also the largest condition number"""
    Afull, B = Afull.cpu().to(HP[Afull.dtype]), B.cpu().to(HP[B.dtype])
    if E is None:
        return torch.linalg.solve(Afull, B), float(torch.linalg.cond(Afull).max())
    X = torch.zeros_like(B.expand(*Afull.shape[:-2], *B.shape[-2:]).contiguous())
    kap = 0.0
    Mf = torch.eye(Afull.shape[-1], dtype=Afull.dtype) if Mfull is None else Mfull.cpu().to(Afull.dtype)
    for c in range(B.shape[-1]):
        As = Afull - float(E[c]) * Mf
        X[..., c] = torch.linalg.solve(As, B[..., c].unsqueeze(-1)).squeeze(-1)
        kap = max(kap, float(torch.linalg.cond(As).max()))
    return X, kap


def _solve(Aop, B, dtype, E=None, M=None, **kw):
    before = dict(host_krylov.calls)
    out = []
    for _ in range(2):
        tr = {}
        with warnings.catch_warnings():
            warnings.simplefilter("error", xa.ConvergenceWarning)
            X = solve(Aop, B, E=E, M=M, method="minres", rtol=RTOL[dtype], trace=tr, **kw)
        out.append((X, tr))
    assert host_krylov.calls == before, "a device run reached a host driver"
    (X, tr), (X2, tr2) = out
    assert torch.equal(X, X2) and tr["niter"] == tr2["niter"], "two runs differ"
    assert tr["converged"]
    h = tr["resid_history"]
    assert all(h[i + 1] <= h[i] for i in range(len(h) - 1)), "resid_history grows"
    if kw.get("precond") is None:
        assert tr["napply"] == tr["niter"] + 1 + tr["nrestart"], "one apply per iteration (+ confirmations)"
    return X, tr


def _close(X, Xref, dtype, kappa):
    X = X.cpu().to(Xref.dtype)
    err, nrm = float((X - Xref).norm()), float(Xref.norm())
    print("minres %s: |X - Xref| / |Xref| = %.3e, bar %.3e" % (dtype, err / nrm, 2 * RTOL[dtype] * kappa))
    assert err <= 2 * RTOL[dtype] * kappa * nrm, (err / nrm, kappa)


def _restated_niter(Afull, B, dtype, E=None):
    """iteration count of tests/minres_ref.py::iterate on the same systems (one system per batch member x column)"""
    Afull, B = Afull.cpu().to(HP[dtype]), B.cpu().to(HP[dtype])
    Bt = B.expand(*Afull.shape[:-2], *B.shape[-2:]).reshape(-1, *B.shape[-2:])
    Af = Afull.reshape(-1, *Afull.shape[-2:])
    nb, n, nc = Bt.shape
    rhs = Bt.transpose(-2, -1).reshape(nb * nc, n)
    eye = torch.eye(n, dtype=Af.dtype)

    def apply(V):
        V = V.reshape(nb, nc, n)
        out = torch.einsum("bij,bcj->bci", Af, V)
        if E is not None:
            out = out - V * E.cpu().to(F64).reshape(1, nc, 1)
        return out.reshape(nb * nc, n)

    stop = torch.clamp(RTOL[dtype] * rhs.norm(dim=-1), min=1e-8)
    return mref.iterate(apply, rhs, stop, 4 * n)["niter"]


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("dtype", mref.DTYPES, ids=mref.IDS)
@pytest.mark.parametrize("variant", ["plain", "E", "EM", "precond"])
def test_dense(dtype, variant):
    A, B, kappa = dense_input(dtype)
    Ad, Bd = A.to(dtype).to(DEV), B.to(dtype).to(DEV)
    Aop = xa.LinearOperator.m(Ad, is_hermitian=True)
    n = A.shape[-1]
    E = M = Mfull = P = None
    g = torch.Generator().manual_seed(17)
    if variant in ("E", "EM"):
        E = torch.tensor([0.2, -0.2], dtype=F64)                   # inside the spectrum: between -1 and +1
    if variant == "EM":
        Mfull = mref.hermitian(g, dtype, n, torch.linspace(1.0, 1.5, n, dtype=F64))[0]
        M = xa.LinearOperator.m(Mfull.to(dtype).to(DEV), is_hermitian=True)
    if variant == "precond":
        P = xa.LinearOperator.m(torch.diag_embed(1.0 + torch.rand(n, dtype=F64, generator=g)).to(dtype).to(DEV),
                                is_hermitian=True)
    rd = torch.float32 if dtype in (torch.float32, torch.complex64) else F64
    X, tr = _solve(Aop, Bd, dtype, E=None if E is None else E.to(rd).to(DEV), M=M, precond=P, max_niter=4 * n)
    Xref, kap = _reference(Ad, Bd, E, None if Mfull is None else Mfull.to(dtype))
    if dtype in (torch.float32, torch.complex64) and kap > 100:
        pytest.fail("test input: fp32 cases must keep kappa <= 100, got %.1f" % kap)
    _close(X, Xref, dtype, kap * (2.0 if variant == "precond" else 1.0))      # P-norm stop: spectrum of P in [1, 2]
    if dtype in (F64, torch.complex128) and variant in ("plain", "E"):
        want = _restated_niter(Ad, Bd, dtype, E)
        print("minres %s %s: %d iterations, restated iteration %d" % (dtype, variant, tr["niter"], want))
        assert tr["nrestart"] == 0 and abs(tr["niter"] - want) <= 1, (tr["niter"], want)


@pytest.mark.parametrize("dtype", [F64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("withE", [False, True], ids=["plain", "E"])
def test_banded(dtype, withE):
    band, B = banded_input(dtype)
    Aop = xa.BandedLinearOperator(band.to(dtype).to(DEV), is_hermitian=True)
    Bd = B.to(dtype).to(DEV)
    E = torch.tensor([0.1, -0.2], dtype=F64) if withE else None
    X, tr = _solve(Aop, Bd, dtype, E=None if E is None else E.to(dtype).to(DEV))
    Xref, kap = _reference(Aop.fullmatrix(), Bd, E)
    assert kap <= 100
    _close(X, Xref, dtype, kap)
    if dtype == F64:
        want = _restated_niter(Aop.fullmatrix(), Bd, dtype, E)
        assert abs(tr["niter"] - want) <= 1, (tr["niter"], want)


@pytest.mark.parametrize("dtype", mref.DTYPES, ids=mref.IDS)
def test_sparse_shifted_laplacian(dtype):
    A, sigma, kappa, B = laplacian_input(dtype)
    if dtype in (torch.float32, torch.complex64) and kappa > 100:
        pytest.fail("test input: fp32 cases must keep kappa <= 100, got %.1f" % kappa)
    t = A.to(dtype).to_sparse_csr()
    Aop = xa.SparseLinearOperator(t.crow_indices().to(DEV), t.col_indices().to(DEV), t.values().to(DEV),
                                  tuple(A.shape), is_hermitian=True)
    Bd = B.to(dtype).to(DEV)
    rd = torch.float32 if dtype in (torch.float32, torch.complex64) else F64
    E = torch.full((2,), sigma, dtype=F64)
    X, tr = _solve(Aop, Bd, dtype, E=E.to(rd).to(DEV), max_niter=4 * A.shape[-1])
    Xref, kap = _reference(A.to(dtype), Bd, E)
    _close(X, Xref, dtype, kap)
    if dtype in (F64, torch.complex128):
        want = _restated_niter(A.to(dtype), Bd, dtype, E)
        assert abs(tr["niter"] - want) <= 1, (tr["niter"], want)


def test_agrees_with_native_gmres_on_real_indefinite_input():
    A, B, kappa = dense_input(F64, seed=5, B=1, n=200)
    Aop = xa.LinearOperator.m(A.to(DEV), is_hermitian=True)
    Bd = B.to(DEV)
    X, _ = _solve(Aop, Bd, F64)
    Xg = solve(Aop, Bd, method="gmres", rtol=RTOL[F64])
    _close(X, Xg.cpu(), F64, kappa)


def test_preconditioner_flag_raises():
    A, B, _ = dense_input(F64, seed=6, B=1, n=64)
    Aop = xa.LinearOperator.m(A.to(DEV), is_hermitian=True)
    P = xa.LinearOperator.m(-torch.eye(64, dtype=F64, device=DEV), is_hermitian=True)
    with pytest.raises(RuntimeError, match="positive definite"):
        solve(Aop, B.to(DEV), method="minres", precond=P)
    with pytest.raises(RuntimeError, match="bicgstab.*gmres"):
        solve(xa.LinearOperator.m(torch.randn(8, 8, dtype=F64, device=DEV), is_hermitian=False),
              torch.randn(8, 1, dtype=F64, device=DEV), method="minres")


def test_singular_system_stays_in_the_complement_of_the_null_vector():
    A, lam, u, b = singular_case()
    n = A.shape[-1]
    Aop = xa.LinearOperator.m(A.to(DEV), is_hermitian=True)
    tr = {}
    X = solve(Aop, b.reshape(n, 1).to(DEV), E=lam.reshape(1).to(DEV), method="minres", rtol=1e-9, max_niter=3 * n,
              trace=tr)
    x = X[:, 0].cpu()
    assert tr["converged"]
    drift = float((u @ x).abs() / x.norm())
    allowed = 10 * singular_drift()["drift"]          # 10 x the float64 restated iteration
    print("minres singular: drift %.3e, allowed %.3e, %d iterations" % (drift, allowed, tr["niter"]))
    assert drift <= allowed


def test_symeig_davidson_backward_through_minres_vs_finite_differences():
    g = torch.Generator().manual_seed(9)
    n, neig = 96, 2
    A0 = mref.hermitian(g, F64, n, torch.linspace(1.0, 30.0, n, dtype=F64) ** 1.2)[0].to(DEV)
    D = torch.randn(n, n, dtype=F64, generator=g)
    D = ((D + D.T) / 2).to(DEV)
    wv = torch.randn(n, neig, dtype=F64, generator=g).to(DEV)

    def loss(A):
        ev, V = symeig(xa.LinearOperator.m((A + A.T) / 2, is_hermitian=True), neig=neig, mode="lowest",
                       method="davidson", min_eps=1e-11,
                       bck_options={"method": "minres", "rtol": 1e-11, "atol": 1e-13, "max_niter": 600})
        return ev.sum() + ((V * wv).sum(0) ** 2).sum()

    before = dict(host_krylov.calls)
    A = A0.clone().requires_grad_()
    loss(A).backward()
    assert host_krylov.calls == before
    ana = float((A.grad * D).sum())
    h = 1e-5
    with torch.no_grad():
        num = float((loss(A0 + h * D) - loss(A0 - h * D)) / (2 * h))
    print("minres symeig backward: analytic %.10e, finite differences %.10e" % (ana, num))
    assert abs(ana - num) <= 1e-6 * max(abs(num), 1.0)
