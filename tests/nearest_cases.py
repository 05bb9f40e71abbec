"""Operators and assertions shared by tests/test_host_symeig_nearest.py and tests/test_gpu_symeig_nearest.py: the same
matrices on the host and on the device, for symeig(mode="nearest", sigma=).

Every case computes the float64 spectrum of the matrix AS STORED in the case's dtype (`reference`), and asserts its
own precondition first: the neig-th and (neig+1)-th distances |lambda - sigma| differ by at least 1e-3 of the spectral
range, so the wanted set is well defined.  A case that violates it is a bug of the test (move sigma).

Checks (`check`), with eps the unit in the last place of the dtype and |A| = max |lambda|:
  eigenvalues  |lam_hat - lam_ref| <= sqrt(N) min_eps + N eps |A|    (Hermitian residual bound |lam_hat - lam| <=
               |r|_2 <= sqrt(N) max|r|, plus the rounding of the operator's arithmetic)
  residual     max|A x - lam x| recomputed in float64 < min_eps + N eps |A|
  orthonormal  max|X^H X - I| <= GUARD_BAD of the dtype
  projector    (only where asked: a wanted set that holds whole multiplets)  |X X^H - P_ref|_2 <= sqrt(N) min_eps / sep,
               sep = the distance from the wanted eigenvalues to the rest (Davis-Kahan)
min_eps: 1e-9 for float64 / complex128, 5e-5 for float32 / complex64 (a float64 prototype's fp32 runs stopped at
max|r| <= 8.4e-6).  max_niter = 30 at the defaults; no ConvergenceWarning is tolerated.
"""
import math
import warnings
import torch
import xitorch_amd as xa
from xitorch_amd.linalg.native_eig import GUARD_BAD
from tests.chebfsi_cases import _UserOp

DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
IDS = ["f64", "f32", "c128", "c64"]
REAL_OF = {torch.float64: torch.float64, torch.float32: torch.float32,
           torch.complex128: torch.float64, torch.complex64: torch.float32}
MAX_NITER = 30


def min_eps(dtype):
    return 1e-9 if REAL_OF[dtype] == torch.float64 else 5e-5


def _wide(dtype):
    return torch.complex128 if dtype.is_complex else torch.float64


def dense_matrix(dtype, n, seed=0):
    """Q diag(linspace(-1, 2, n)) Q^H, exactly Hermitian storage, built in 64-bit"""
    g = torch.Generator().manual_seed(300 + seed + n)
    Z = torch.randn((n, n), dtype=torch.float64, generator=g)
    if dtype.is_complex:
        Z = torch.complex(Z, torch.randn((n, n), dtype=torch.float64, generator=g))
    Q, _ = torch.linalg.qr(Z.to(_wide(dtype)))
    lam = torch.linspace(-1.0, 2.0, n, dtype=torch.float64)
    A = torch.matmul(Q * lam.to(Q.dtype), Q.transpose(-2, -1).conj())
    A = ((A + A.transpose(-2, -1).conj()) * 0.5).to(dtype)
    return (A + A.transpose(-2, -1).conj()) * 0.5


def _phases(A, dtype):
    """D A D^H with a diagonal unitary D: the same spectrum, genuinely complex entries"""
    if not dtype.is_complex:
        return A.to(dtype)
    n = A.shape[-1]
    al = 0.7 * torch.arange(n, dtype=torch.float64) ** 1.5
    d = torch.complex(torch.cos(al), torch.sin(al))
    return (d.unsqueeze(-1) * A.to(torch.complex128) * d.conj().unsqueeze(-2)).to(dtype)


def laplacian_matrix(dtype, nx, ny):
    """the 5-point Laplacian on an nx x ny grid (Dirichlet): eigenvalues 4 - 2 cos(i pi / (nx+1)) - 2 cos(j pi / (ny+1))"""
    def lap1(n):
        return 2.0 * torch.eye(n, dtype=torch.float64) - torch.diag(torch.ones(n - 1, dtype=torch.float64), 1) \
            - torch.diag(torch.ones(n - 1, dtype=torch.float64), -1)
    A = torch.kron(lap1(nx), torch.eye(ny, dtype=torch.float64)) + torch.kron(torch.eye(nx, dtype=torch.float64), lap1(ny))
    return _phases(A, dtype)


def tridiagonal_matrix(dtype, n):
    A = 2.0 * torch.eye(n, dtype=torch.float64) - torch.diag(torch.ones(n - 1, dtype=torch.float64), 1) \
        - torch.diag(torch.ones(n - 1, dtype=torch.float64), -1)
    return _phases(A, dtype)


def make_operator(kind, A, device):
    """the matrix A (host, its own dtype) as an operator of `kind` on `device`"""
    n = A.shape[-1]
    if kind == "dense":
        return xa.LinearOperator.m(A.to(device), True)
    if kind == "mv":
        return _UserOp(A.to(device))
    if kind == "sparse":
        idx = torch.nonzero(A)                                               # row-major: already CSR order
        crow = torch.zeros(n + 1, dtype=torch.int64)
        crow[1:] = torch.cumsum(torch.bincount(idx[:, 0], minlength=n), 0)
        return xa.SparseLinearOperator(crow.to(device), idx[:, 1].contiguous().to(device),
                                       A[idx[:, 0], idx[:, 1]].to(device), (n, n), is_hermitian=True)
    if kind == "banded":                                                     # tridiagonal: band[d, i] = A[i, i + d - 1]
        band = torch.zeros(3, n, dtype=A.dtype)
        band[1] = torch.diagonal(A)
        band[2, :n - 1] = torch.diagonal(A, 1)
        band[0, 1:] = torch.diagonal(A, -1)
        return xa.BandedLinearOperator(band.to(device), is_hermitian=True)
    raise ValueError(kind)


# name -> (matrix builder, operator kind, sigma, neig, projector check)
CASES = {
    "dense257": (lambda dt: dense_matrix(dt, 257), "dense", 0.62, 4, False),
    "dense200": (lambda dt: dense_matrix(dt, 200), "dense", 0.62, 4, False),
    "dense257_below": (lambda dt: dense_matrix(dt, 257), "dense", -5.0, 4, False),
    "dense257_above": (lambda dt: dense_matrix(dt, 257), "dense", 7.0, 4, False),
    "lap16x17_csr": (lambda dt: laplacian_matrix(dt, 16, 17), "sparse", 3.3, 6, False),
    "lap16x16_5": (lambda dt: laplacian_matrix(dt, 16, 16), "sparse", 2.9, 5, False),
    "lap16x16_7": (lambda dt: laplacian_matrix(dt, 16, 16), "sparse", 2.9, 7, True),
    "tridiag300": (lambda dt: tridiagonal_matrix(dt, 300), "banded", 1.37, 5, False),
    "tridiag300_mv": (lambda dt: tridiagonal_matrix(dt, 300), "mv", 1.37, 5, False),
}


def reference(A, sigma, neig):
    """float64 spectrum of the stored matrix; (lam_all, indices of the neig nearest sigma ascending, sep, vectors);
    asserts the precondition of the case"""
    lam, U = torch.linalg.eigh(A.to(_wide(A.dtype)))
    d = (lam - sigma).abs()
    order = torch.argsort(d, stable=True)
    ds = d[order]
    rng = float(lam[-1] - lam[0])
    assert float(ds[neig] - ds[neig - 1]) >= 1e-3 * rng, \
        "test bug: distances %d and %d from sigma = %g differ by %.3e < 1e-3 of the range %.3e: move sigma" \
        % (neig, neig + 1, sigma, float(ds[neig] - ds[neig - 1]), rng)
    sel = torch.sort(order[:neig])[0]
    rest = torch.ones_like(lam, dtype=torch.bool)
    rest[sel] = False
    sep = float((lam[rest].unsqueeze(0) - lam[sel].unsqueeze(1)).abs().min())
    return lam, sel, sep, U


def check(A, sigma, neig, ev, X, dtype, eps_=None, projector=False, what=""):
    """all the assertions of one member; returns the figures"""
    eps_ = min_eps(dtype) if eps_ is None else eps_
    n = A.shape[-1]
    lam, sel, sep, U = reference(A, sigma, neig)
    norm = float(lam.abs().max())
    ulp = torch.finfo(REAL_OF[dtype]).eps
    assert ev.shape == (neig,) and X.shape == (n, neig), (ev.shape, X.shape)
    evw = ev.detach().cpu().to(torch.float64)
    Xw = X.detach().cpu().to(_wide(dtype))
    assert bool((evw[1:] >= evw[:-1]).all()), "eigenvalues not ascending %s" % what
    err = float((evw - lam[sel]).abs().max())
    bound = math.sqrt(n) * eps_ + n * ulp * norm
    R = torch.matmul(A.to(_wide(dtype)), Xw) - Xw * evw.to(Xw.dtype)
    res = float(R.abs().max())
    G = float((torch.matmul(Xw.transpose(-2, -1).conj(), Xw) - torch.eye(neig, dtype=Xw.dtype)).abs().max())
    print("%s: |d lam| %.3e (bound %.3e)  max|r| %.3e (bound %.3e)  |X^H X - I| %.3e" % (
        what, err, bound, res, eps_ + n * ulp * norm, G))
    assert err <= bound, "%s eigenvalue error %.3e > %.3e" % (what, err, bound)
    assert res < eps_ + n * ulp * norm, "%s max|A x - lam x| = %.3e" % (what, res)
    assert G <= GUARD_BAD[REAL_OF[dtype]], "%s max|X^H X - I| = %.3e" % (what, G)
    if projector:
        P = torch.matmul(U[:, sel], U[:, sel].transpose(-2, -1).conj())
        dp = float(torch.linalg.matrix_norm(torch.matmul(Xw, Xw.transpose(-2, -1).conj()) - P, ord=2))
        print("%s: |X X^H - P|_2 %.3e (bound %.3e, sep %.3e)" % (what, dp, math.sqrt(n) * eps_ / sep, sep))
        assert dp <= math.sqrt(n) * eps_ / sep, "%s projector error %.3e > %.3e" % (what, dp, math.sqrt(n) * eps_ / sep)
    return err, res


def solve(op, neig, sigma, dtype, method="chebfsi", trace=None, **kw):
    """symeig(mode="nearest") at the defaults with the case's min_eps; a ConvergenceWarning is an error"""
    from xitorch_amd.linalg import symeig
    kw.setdefault("min_eps", min_eps(dtype))
    kw.setdefault("max_niter", MAX_NITER)
    if method == "exacteig":
        kw = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error", xa.ConvergenceWarning)
        with torch.no_grad():
            return symeig(op, neig, "nearest", method=method, sigma=sigma, trace=trace, **kw) if method != "exacteig" \
                else symeig(op, neig, "nearest", method=method, sigma=sigma)
