"""Problems with a known spectrum and the per-pair assertions shared by tests/test_host_lobpcg.py and
tests/test_gpu_lobpcg.py (the same matrices on the host and on the device).  The reference spectrum is
torch.linalg.eigh in float64 of the matrix the operator stores; for the generalised problem, of L^-1 A L^-H with
M = L L^H."""
import math
import numpy as np
import torch
import xitorch_amd as xa
from xitorch_amd.linalg.native_eig import GUARD_BAD
from tests import chebfsi_cases as cc

N = cc.N
DTYPES, IDS, REAL_OF = cc.DTYPES, cc.IDS, cc.REAL_OF
MAX_NITER = 300
# best max|resid| the HOST twin reaches on the dense N = 200, lam_i = i cases when asked for min_eps = 1e-30
# (max_niter = 300; neig 1 / 4 / 6), measured on the CPU:
#   float32    lowest 8.1e-7 / 7.8e-6 / 1.2e-5   uppest 1.9e-5 / 1.0e-4 / 1.5e-4
#   complex64  lowest 9.2e-7 / 7.9e-6 / 1.1e-5   uppest 2.4e-5 / 2.4e-4 / 1.4e-4
# min_eps of the 32-bit cases = 4 x the largest of them
MEASURED32 = 2.4e-4
MIN_EPS32 = 4 * MEASURED32


def min_eps(dtype):
    return 1e-8 if REAL_OF[dtype] == torch.float64 else MIN_EPS32


def wide(t):
    return t.detach().cpu().to(torch.complex128 if t.is_complex() else torch.float64)


def grid_matrix(n, dtype=torch.float64, phase=False):
    """the 5-point matrix of an n x n grid (4 on the diagonal, -1 to the four neighbours; exact double eigenvalues);
    phase: every off-diagonal pair times a unit-modulus phase and its conjugate (Hermitian, still diagonally dominant)"""
    Nn = n * n
    A = torch.zeros((Nn, Nn), dtype=torch.complex128 if phase else torch.float64)
    idx = np.arange(Nn).reshape(n, n)
    rng = np.random.default_rng(5)
    for i in range(n):
        for j in range(n):
            k = idx[i, j]
            A[k, k] = 4.0
            for (a, b) in ((i, j + 1), (i + 1, j)):
                if a < n and b < n:
                    v = -1.0 * (np.exp(2j * np.pi * rng.random()) if phase else 1.0)
                    A[k, idx[a, b]] = v
                    A[idx[a, b], k] = np.conj(v)
    return A.to(dtype)


def overlap_matrix(n, dtype):
    """M = I + 0.3 (5-point grid matrix) / 4 of order n^2: eigenvalues in (1, 1.6)"""
    G = grid_matrix(n, torch.complex128 if dtype.is_complex else torch.float64, phase=dtype.is_complex)
    M = torch.eye(n * n, dtype=G.dtype) + 0.3 * G / 4.0
    return ((M + M.transpose(-2, -1).conj()) * 0.5).to(dtype)


def dominant_matrix(dtype, n=N, seed=3):
    """diag(1 .. n) + 0.05 sym(randn)"""
    g = torch.Generator().manual_seed(seed)
    Z = torch.randn((n, n), dtype=torch.float64, generator=g)
    if dtype.is_complex:
        Z = torch.complex(Z, torch.randn((n, n), dtype=torch.float64, generator=g))
    A = torch.diag(torch.arange(1, n + 1, dtype=torch.float64)).to(Z.dtype) + 0.05 * (Z + Z.transpose(-2, -1).conj()) / 2
    return ((A + A.transpose(-2, -1).conj()) * 0.5).to(dtype)


def csr_of(A, device):
    idx = torch.nonzero(A)                                               # row-major: already CSR order
    n = A.shape[-1]
    crow = torch.zeros(n + 1, dtype=torch.int64)
    crow[1:] = torch.cumsum(torch.bincount(idx[:, 0], minlength=n), 0)
    return xa.SparseLinearOperator(crow.to(device), idx[:, 1].contiguous().to(device),
                                   A[idx[:, 0], idx[:, 1]].to(device), (n, n), is_hermitian=True)


def banded_of(A, hb, device):
    n = A.shape[-1]
    band = torch.zeros(2 * hb + 1, n, dtype=A.dtype)
    for d in range(-hb, hb + 1):                                         # band[d + hb, i] = A[i, i + d]
        diag = torch.diagonal(A, d)
        if d >= 0:
            band[d + hb, :n - d] = diag
        else:
            band[d + hb, -d:] = diag
    return xa.BandedLinearOperator(band.to(device), is_hermitian=True)


def operator_of(kind, A, device):
    if kind == "dense":
        return xa.LinearOperator.m(A.to(device), True)
    if kind == "sparse":
        return csr_of(A, device)
    if kind == "banded":
        hb = int((torch.nonzero(A)[:, 0] - torch.nonzero(A)[:, 1]).abs().max())
        return banded_of(A, hb, device)
    if kind == "mv":
        return cc._UserOp(A.to(device))
    raise ValueError(kind)


def reference_spectrum(A, M=None):
    """ascending eigenvalues (.., n) in float64 of A x = lam M x, and lam_min(M) (1 without M)"""
    Aw = wide(A)
    if M is None:
        return torch.linalg.eigvalsh(Aw), 1.0
    Mw = wide(M)
    L = torch.linalg.cholesky(Mw)
    Li = torch.linalg.inv(L)
    T = Li @ Aw @ Li.transpose(-2, -1).conj()
    return torch.linalg.eigvalsh((T + T.transpose(-2, -1).conj()) * 0.5), float(torch.linalg.eigvalsh(Mw).min())


def eigenvalue_bound(n, eps_, dtype, norm2, lmin_m=1.0):
    """cc.eigenvalue_bound with the residual term divided by sqrt(lam_min(M)) (the M^-1 norm of the residual)"""
    return math.sqrt(n) * eps_ / math.sqrt(lmin_m) + 64 * torch.finfo(REAL_OF[dtype]).eps * norm2


def assert_pairs(A, M, ev, X, neig, mode, dtype, eps_=None, spectrum=None):
    """all pairs, none left out: residual entries, M-orthonormality, eigenvalues by order (ascending in both modes).
    Vectors are never compared (the spectra may be degenerate).  Returns the largest residual entry."""
    eps_ = min_eps(dtype) if eps_ is None else eps_
    n = A.shape[-1]
    assert ev.shape[-1] == neig and X.shape[-2:] == (n, neig), (ev.shape, X.shape)
    Aw, Xw, evw = wide(A), wide(X), ev.detach().cpu().to(torch.float64)
    MX = Xw if M is None else wide(M) @ Xw
    R = Aw @ Xw - MX * evw.unsqueeze(-2).to(Xw.dtype)
    res = R.abs().amax(dim=-2)
    assert bool((res < eps_).all()), "max|A x - lam M x| per pair: worst %.3e >= %.3e" % (float(res.max()), eps_)
    G = Xw.transpose(-2, -1).conj() @ MX - torch.eye(neig, dtype=Xw.dtype)
    assert float(G.abs().max()) <= GUARD_BAD[REAL_OF[dtype]], "max|X^H M X - I| = %.3e" % float(G.abs().max())
    lam, lmin = reference_spectrum(A, M) if spectrum is None else spectrum
    want = lam[..., :neig] if mode == "lowest" else lam[..., n - neig:]
    err = (evw - want).abs()
    bound = eigenvalue_bound(n, eps_, dtype, float(lam.abs().max()), lmin)
    assert bool((err <= bound).all()), "eigenvalue error %.3e > %.3e" % (float(err.max()), bound)
    return float(res.max())


def cluster_spectrum(n=N):
    """{1, 1 + 1e-6, 1 + 2e-6, 2, 2, 2, 3, 4, ...}"""
    s = torch.arange(n, dtype=torch.float64) - 3.0
    s[:6] = torch.tensor([1.0, 1.0 + 1e-6, 1.0 + 2e-6, 2.0, 2.0, 2.0], dtype=torch.float64)
    return s


def batch_spectra(batch, n=N):
    """three different spectra dealt out over the members"""
    i = torch.arange(n, dtype=torch.float64)
    three = [i, 0.5 * i + 0.01 * i * i, 10.0 + 2.0 * i]
    nb = math.prod(batch)
    return torch.stack([three[b % 3] for b in range(nb)]).reshape(*batch, n)
