"""Matrices and the a-posteriori checks shared by tests/test_host_gkl.py (CPU) and tests/test_gpu_gkl.py (-m gpu).

Every matrix is built once in float64 / complex128 from chosen singular values and random orthonormal factors; the
operator under test is that matrix rounded to the test's dtype, and the TRUE singular values are those of the rounded
matrix (numpy, float64).  The checks need no tolerance fitted to the solver:

  r     = max_i max(|A v_i - s_i u_i|, |A^H u_i - s_i v_i|), recomputed in float64 from what the solver returned
  Weyl  : the augmented operator [[0, A], [A^H, 0]] has an eigenvalue within sqrt(2) r of every s_i (unit u_i, v_i)
  stop  : the solver stops on |beta P[last, i]| <= min_eps sigma_max, an estimate of that residual; r <= 2 min_eps
          sigma_max allows the estimate to be off by its own size (the roundings of one cycle, ncv u sigma_max, are far
          below min_eps = 100 u for ncv <= 64 only in sum with it: the factor 2)
  orth  : max|U^H U - I|, max|V^H V - I| <= ORTH_C u ncv  (gkl_ref: CGS2 and the restart rotations)
"""
import functools
import numpy as np
import torch
from tests import gkl_ref as gref


def _orth(rng, n, r, cplx):
    x = rng.standard_normal((n, r))
    if cplx:
        x = x + 1j * rng.standard_normal((n, r))
    return np.linalg.qr(x)[0]


def with_spectrum(m, n, sigma, seed=0, cplx=False):
    rng = np.random.default_rng(seed + 31 * m + n)
    r = min(m, n)
    s = np.asarray(sigma, dtype=np.float64)
    assert s.shape == (r,)
    U, V = _orth(rng, m, r, cplx), _orth(rng, n, r, cplx)
    return torch.from_numpy((U * s) @ V.conj().T)


@functools.lru_cache(maxsize=None)
def graded(m, n, cplx=False):
    """sigma = 1, 1e-1, ..., 1e-11 and a tail at 1e-12"""
    r = min(m, n)
    s = np.full(r, 1e-12)
    s[:12] = 10.0 ** -np.arange(12.0)
    return with_spectrum(m, n, s, cplx=cplx)


@functools.lru_cache(maxsize=None)
def slow(m, n, cplx=False):
    """sigma_i = (1 + i)^(-1/2): no gap to speak of, restarts are needed"""
    return with_spectrum(m, n, (1.0 + np.arange(min(m, n))) ** -0.5, seed=1, cplx=cplx)


@functools.lru_cache(maxsize=None)
def lowest(m, n, cplx=False):
    """three separated small values 1e-3, 2e-3, 4e-3 under a bulk in [0.5, 1]"""
    r = min(m, n)
    s = np.linspace(1.0, 0.5, r)
    s[-3:] = [4e-3, 2e-3, 1e-3]
    return with_spectrum(m, n, s, seed=2, cplx=cplx)


@functools.lru_cache(maxsize=None)
def rank_deficient(m, n, rank, cplx=False):
    s = np.zeros(min(m, n))
    s[:rank] = np.linspace(1.0, 0.3, rank)
    return with_spectrum(m, n, s, seed=3, cplx=cplx)


@functools.lru_cache(maxsize=None)
def uneven_batch(cplx=False):
    """three members (200, 150): four values over a flat tail at 1e-6 (converged within the first cycle), the slowly
    decaying spectrum and the graded one.  With k = 4 and min_eps = 100 u the slow member needs a restart at ncv = 12 in
    every dtype (at ncv = 16 it is done in one cycle in single precision, where 100 u is 1.2e-5)"""
    s_fast = np.full(150, 1e-6)
    s_fast[:4] = [1.0, 0.5, 0.25, 0.125]
    return torch.stack([with_spectrum(200, 150, s_fast, seed=7, cplx=cplx), slow(200, 150, cplx), graded(200, 150, cplx)])


def check_uneven(trace, k):
    """member 0 of `uneven_batch` has its k triplets converged in a cycle in which another member has not (the
    per-cycle converged counts of every member, trace["converged_history"]), and the run went on for that member"""
    hist = trace["converged_history"]
    print("converged per cycle and member:", hist)
    assert all(len(h) == 3 for h in hist) and len(hist) == trace["niter"]
    early = [c for c, h in enumerate(hist) if h[0] >= k and min(h[1:]) < k]
    assert early and early[0] + 1 < trace["niter"], hist
    assert min(hist[-1]) >= k


def true_values(A, k, mode):
    """the k wanted singular values of the (already rounded) matrix A, ascending, float64 (numpy)"""
    s = np.linalg.svd(A.detach().cpu().to(torch.complex128 if A.is_complex() else torch.float64).numpy(),
                      compute_uv=False)
    s = s[..., ::-1]                                                          # ascending
    return s[..., :k] if mode == "lowest" else s[..., s.shape[-1] - k:]


def unit_roundoff(dtype):
    return torch.finfo(dtype).eps


def residual(A, u, s, vh):
    """largest true residual norm over the returned triplets, float64"""
    wide = torch.complex128 if A.is_complex() else torch.float64
    A, u, vh, s = A.detach().cpu().to(wide), u.detach().cpu().to(wide), vh.detach().cpu().to(wide), \
        s.detach().cpu().to(torch.float64)
    v = vh.transpose(-2, -1).conj()
    r1 = torch.linalg.vector_norm(A @ v - u * s.unsqueeze(-2), dim=-2)
    r2 = torch.linalg.vector_norm(A.transpose(-2, -1).conj() @ u - v * s.unsqueeze(-2), dim=-2)
    return float(torch.maximum(r1, r2).max())


def check(A, u, s, vh, k, mode, min_eps, ncv, label=""):
    """the bounds of the module docstring; returns (max |s - sigma|, r) for the tests that print or compare them"""
    ur = unit_roundoff(A.dtype)
    sig = true_values(A, k, mode)
    smax = float(np.linalg.svd(A.detach().cpu().numpy().astype(np.complex128 if A.is_complex() else np.float64),
                               compute_uv=False).max())
    r = residual(A, u, s, vh)
    err = float(np.abs(s.detach().cpu().double().numpy() - sig).max())
    print("%s: max|s - sigma| = %.3e, r = %.3e, min_eps sigma_max = %.3e" % (label, err, r, min_eps * smax))
    assert err <= 2.0 ** 0.5 * r, (label, err, r)
    assert r <= 2.0 * min_eps * smax, (label, r, min_eps * smax)
    eye = torch.eye(k, dtype=torch.float64)
    wide = torch.complex128 if A.is_complex() else torch.float64
    uw, vw = u.detach().cpu().to(wide), vh.detach().cpu().to(wide).transpose(-2, -1).conj()
    for name, X in (("U", uw), ("V", vw)):
        dev = float((X.transpose(-2, -1).conj() @ X - eye).abs().max())
        assert dev <= gref.ORTH_C * ur * ncv, (label, name, dev, gref.ORTH_C * ur * ncv)
    return err, r
