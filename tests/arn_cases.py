"""Inputs of the Krylov-Schur Arnoldi tests: the projected matrices H (m + 1, m) of the kernel tests and the operators of
the solver tests, as numpy arrays (the tests move them to torch / the device)."""
import numpy as np

SMALL_KINDS = ("random", "triu", "hessenberg", "hess_spike", "companion", "jordan", "zero", "identity", "tiny", "huge")


def _rand(rng, shape, cplx):
    a = rng.standard_normal(shape)
    return a + 1j * rng.standard_normal(shape) if cplx else a


def small_matrix(kind, m, cplx, seed=0):
    """H (m + 1, m): the Rayleigh quotient in rows [0, m), beta in H[m, m - 1]"""
    rng = np.random.default_rng(1000 * seed + 17 * m + (1 if cplx else 0))
    H = np.zeros((m + 1, m), np.complex128 if cplx else np.float64)
    B = _rand(rng, (m, m), cplx)
    if kind == "random":
        H[:m] = B
    elif kind == "triu":
        H[:m] = np.triu(B)
    elif kind == "hessenberg":
        H[:m] = np.triu(B, -1)
    elif kind == "hess_spike":                      # the shape after a restart: a full block, the spike row, Hessenberg
        k = max(1, m // 2)
        H[:m] = np.triu(B, -1)
        H[:k, :k] = B[:k, :k]
        H[k, :k] = B[k, :k]
        H[k + 1:m, :k] = 0
    elif kind == "companion":                       # z^m - 1: all |lambda| equal
        H[np.arange(1, m), np.arange(m - 1)] = 1.0
        H[0, m - 1] = 1.0
    elif kind == "jordan":                          # [[1, 1], [0, 1]] embedded in a larger matrix
        H[:m] = 0.1 * B
        H[:2, :] = 0
        H[:, :2] = 0
        H[0, 0] = H[1, 1] = H[0, 1] = 1.0
    elif kind == "zero":
        pass
    elif kind == "identity":
        H[:m] = np.eye(m)
    elif kind == "tiny":
        H[:m] = B * 1e-150
    elif kind == "huge":
        H[:m] = B * 1e150
    else:
        raise KeyError(kind)
    scale = {"tiny": 1e-150, "huge": 1e150}.get(kind, 1.0)
    H[m, m - 1] = 0.3 * scale
    return H


def rotation2():
    """2 x 2 rotation: the purely imaginary pair +-i"""
    return np.array([[0.0, -1.0], [1.0, 0.0], [0.0, 0.25]])


def straddle(m, keep, seed=0):
    """real H (m + 1, m), orthogonally similar to a block diagonal of known 2 x 2 blocks, such that the eigenvalues
    ranked keep - 1 and keep by modulus are ONE conjugate pair: pairs of moduli 2, 1.95, ... behind one real eigenvalue
    2.5 when keep is even"""
    rng = np.random.default_rng(seed)
    B = np.zeros((m, m))
    i, r = (keep - 1) % 2, 2.0
    if i:
        B[0, 0] = 2.5
    while i + 1 < m:
        a, b = r * np.cos(0.3 + 0.1 * i), r * np.sin(0.3 + 0.1 * i)
        B[i:i + 2, i:i + 2] = [[a, b], [-b, a]]
        i, r = i + 2, r - 0.05
    if i < m:
        B[i, i] = 0.01
    U, _ = np.linalg.qr(rng.standard_normal((m, m)))
    H = np.zeros((m + 1, m))
    H[:m] = U @ B @ U.T
    H[m, m - 1] = 0.2
    return H


# ---------------------------------------------------------------------------------------------------------------------
def normal_spectrum(n, nwanted, cplx, seed=0):
    """eigenvalues of a normal test operator: nwanted on 1.5 <= |lambda| <= 2, at least 0.05 apart, the rest inside
    |lambda| <= 1.  Real operators get conjugate pairs (nwanted even)."""
    rng = np.random.default_rng(seed)
    npair = nwanted if cplx else nwanted // 2
    # moduli 2.0, 1.9, ... (0.1 apart) and arguments spread over the upper half plane: any two differ by >= 0.1
    mod = 2.0 - 0.1 * np.arange(npair)
    arg = 0.4 + 2.2 * np.arange(npair) / max(npair, 1)
    big = mod * np.exp(1j * arg)
    nrest = n - (nwanted if cplx else 2 * npair)
    if cplx:
        rest = np.sqrt(rng.uniform(0, 1, nrest)) * np.exp(2j * np.pi * rng.uniform(0, 1, nrest))
        return np.concatenate([big, rest])
    nrp = nrest // 2
    rest = np.sqrt(rng.uniform(0, 1, nrp)) * np.exp(1j * np.pi * rng.uniform(0.05, 0.95, nrp))
    lam = np.concatenate([big, np.conj(big), rest, np.conj(rest)])
    if nrest % 2:
        lam = np.concatenate([lam, [0.3]])
    return lam


def normal_matrix(n, nwanted, cplx, seed=0, extra_real=()):
    """(A, lam): A = U blockdiag([[a, b], [-b, a]]) U^T with U orthogonal (real) or U diag(lam) U^H (complex);
    extra_real: real eigenvalues that replace as many of the bulk (they shift the parity of the ranking by modulus)"""
    rng = np.random.default_rng(seed + 1)
    lam = np.concatenate([normal_spectrum(n - len(extra_real), nwanted, cplx, seed), np.asarray(extra_real, complex)])
    if cplx:
        U, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
        return (U * lam) @ U.conj().T, lam
    D = np.zeros((n, n))
    up = [z for z in lam if z.imag > 0]
    i = 0
    for z in up:
        D[i:i + 2, i:i + 2] = [[z.real, z.imag], [-z.imag, z.real]]
        i += 2
    for z in lam:
        if z.imag == 0:
            D[i, i] = z.real
            i += 1
    U, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return U @ D @ U.T, lam


def toeplitz_eigs(n, a, b, c):
    """eigenvalues a + 2 sqrt(bc) cos(j pi / (n + 1)) of tridiag(b, a, c) (b below, c above the diagonal)"""
    j = np.arange(1, n + 1)
    return a + 2.0 * np.sqrt(complex(b * c)) * np.cos(j * np.pi / (n + 1))


def toeplitz_dense(n, a, b, c):
    return a * np.eye(n) + b * np.eye(n, k=-1) + c * np.eye(n, k=1)


def toeplitz_operator(kind, n, a, b, c, dtype, device):
    """tridiag(b, a, c) as a BandedLinearOperator ("banded") or a SparseLinearOperator ("csr") on `device`"""
    import torch
    from xitorch_amd.linop import SparseLinearOperator, BandedLinearOperator
    if kind == "banded":
        band = torch.zeros(3, n, dtype=dtype)
        band[0], band[1], band[2] = b, a, c          # band[d, i] = A[i, i + d - 1]
        return BandedLinearOperator(band.to(device))
    T = torch.from_numpy(toeplitz_dense(n, a, b, c)).to(dtype)
    rows, cols = torch.nonzero(T, as_tuple=True)                   # row-major order: sorted by row
    crow = torch.zeros(n + 1, dtype=torch.int64)
    crow[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    return SparseLinearOperator(crow.to(device), cols.to(device), T[rows, cols].to(device), (n, n))


def toeplitz_cond(n, b, c):
    """condition number of the closed-form eigenvector matrix D S, D = diag((b / c)^(i / 2)), S orthogonal (sines)"""
    r = np.sqrt(abs(b / c))
    return max(r, 1.0 / r) ** (n - 1)


def stochastic(n, seed=0):
    """column-stochastic matrix with positive entries: Perron eigenvalue 1, positive eigenvector"""
    rng = np.random.default_rng(seed)
    P = rng.uniform(0.0, 1.0, (n, n)) ** 4 + 0.01
    return P / P.sum(axis=0, keepdims=True)


def block_diagonal(n, nb, seed=0):
    """blockdiag(A1 (nb x nb), A2): a start vector inside the first block spans an invariant subspace of dimension nb.
    A1 has its eigenvalues on |lambda| in [1.5, 2] (normal, real 2 x 2 blocks), A2 inside |lambda| <= 1."""
    A1, lam1 = normal_matrix(nb, nb - nb % 2, False, seed)
    lam1 = lam1.copy()
    A2, lam2 = normal_matrix(n - nb, 0, False, seed + 5)
    A = np.zeros((n, n))
    A[:nb, :nb] = A1
    A[nb:, nb:] = A2
    return A, np.concatenate([lam1, lam2])
