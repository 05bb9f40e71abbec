"""Shared by the FSAI tests: the variable-coefficient grid problem and a dense numpy restatement of FSAI.

The grid problem is the 5-point diffusion operator on an n x n grid with Dirichlet boundaries and edge conductances
exp(1.5 g), g ~ N(0, 1) from numpy.random.default_rng(seed): symmetric positive definite, condition number in the
thousands at n = 24.  `fsai_dense` is written from the formulas alone (per row: gather A[S, S], solve A_JJ y = e_m,
g = conj(y) / sqrt(Re y_m)) and shares no code with the package.
"""
import numpy as np
import torch


def grid_edges(n, seed=0, nmembers=1):
    """conductances of the horizontal (n, n+1) and vertical (n+1, n) edges, one set per member"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nmembers):
        cx = np.exp(1.5 * rng.standard_normal((n, n + 1)))
        cy = np.exp(1.5 * rng.standard_normal((n + 1, n)))
        out.append((cx, cy))
    return out


def grid_csr(n, seed=0, nmembers=1, phase=False):
    """-> crow (N+1,), col (nnz,) int64 numpy and values (nmembers, nnz) float64.  phase: complex128, every off-diagonal
    pair multiplied by a unit-modulus phase and its conjugate; the matrix stays Hermitian and irreducibly diagonally
    dominant with a positive diagonal, hence positive definite.  Full storage (both triangles), columns ascending."""
    N = n * n
    idx = np.arange(N).reshape(n, n)
    rows, cols, slots = [], [], []                    # slot: which conductance feeds the entry
    # entry list built once; values per member from the conductances
    def add(r, c, kind, a, b):
        rows.append(r), cols.append(c), slots.append((kind, a, b))
    for i in range(n):
        for j in range(n):
            k = idx[i, j]
            add(k, k, "d", i, j)
            if j > 0:
                add(k, idx[i, j - 1], "x", i, j)
            if j < n - 1:
                add(k, idx[i, j + 1], "x", i, j + 1)
            if i > 0:
                add(k, idx[i - 1, j], "y", i, j)
            if i < n - 1:
                add(k, idx[i + 1, j], "y", i + 1, j)
    rows, cols = np.array(rows), np.array(cols)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    slots = [slots[o] for o in order]
    crow = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=N), out=crow[1:])
    vals = np.zeros((nmembers, len(rows)), dtype=np.complex128 if phase else np.float64)
    prng = np.random.default_rng(seed + 1000)
    ph = np.exp(2j * np.pi * prng.random((N, N))) if phase else None
    for b, (cx, cy) in enumerate(grid_edges(n, seed, nmembers)):
        for k, (kind, a, c) in enumerate(slots):
            if kind == "d":
                vals[b, k] = cx[a, c] + cx[a, c + 1] + cy[a, c] + cy[a + 1, c]
            else:
                v = -(cx[a, c] if kind == "x" else cy[a, c])
                if phase:
                    r_, c_ = rows[k], cols[k]
                    v = v * (ph[r_, c_] if r_ > c_ else np.conj(ph[c_, r_]))
                vals[b, k] = v
    return crow, cols, vals


def grid_operator(n, seed=0, nmembers=1, dtype=torch.float64, device="cpu", phase=False, shift=0.0, batch=True):
    """SparseLinearOperator of the grid problem (minus shift * I), Hermitian; also returns the dense matrices
    (nmembers, N, N) as float64 / complex128 numpy."""
    from xitorch_amd.linop import SparseLinearOperator
    crow, col, vals = grid_csr(n, seed, nmembers, phase)
    N = n * n
    rows = np.repeat(np.arange(N), np.diff(crow))
    vals = vals.copy()
    vals[:, rows == col] -= shift
    dense = np.zeros((nmembers, N, N), dtype=vals.dtype)
    for b in range(nmembers):
        dense[b, rows, col] = vals[b]
    v = torch.as_tensor(vals).to(dtype).to(device)
    if not batch:
        v = v[0]
    shape = (nmembers, N, N) if batch else (N, N)
    A = SparseLinearOperator(torch.as_tensor(crow).to(device), torch.as_tensor(col).to(device), v, shape,
                             is_hermitian=True)
    return A, dense


def dense_of(crow, col, vals, N):
    """dense (nb, N, N) numpy matrix of a CSR operator, duplicates added"""
    crow, col = np.asarray(crow), np.asarray(col)
    vals = np.asarray(vals)
    vals = vals.reshape(-1, vals.shape[-1])
    rows = np.repeat(np.arange(N), np.diff(crow))
    out = np.zeros((vals.shape[0], N, N), dtype=vals.dtype)
    for b in range(vals.shape[0]):
        np.add.at(out[b], (rows, col), vals[b])
    return out


def hermitian_from_lower(Ad):
    """the Hermitian matrix FSAI sees: the lower triangle mirrored, the diagonal's real part"""
    low = np.tril(Ad, -1)
    return low + np.conj(low.T) + np.diag(np.real(np.diag(Ad)))


def pattern_dense(Ad, power, max_row):
    """rows of sorted column lists of G from the dense structure (Ad: lower triangle significant)"""
    N = Ad.shape[0]
    S = (np.tril(Ad) != 0)
    S = S | S.T | np.eye(N, dtype=bool)
    P = S.copy()
    for _ in range(power - 1):
        P = (P.astype(np.int64) @ S.astype(np.int64)) > 0
    out = []
    for i in range(N):
        cols = [j for j in range(i + 1) if P[i, j]]
        out.append(cols[-max_row:])
    return out


def fsai_dense(Ad, pattern):
    """G (N, N) dense from the formulas: per row solve A_JJ y = e_m, g = conj(y) / sqrt(Re y_m).  Ad: one dense
    matrix whose lower triangle is read.  A block that is not positive definite (checked by numpy's Cholesky) or not
    finite gives the Jacobi row.  -> (G, number of fallback rows, kappa_2 of every block)"""
    H = hermitian_from_lower(np.asarray(Ad))
    N = H.shape[0]
    G = np.zeros((N, N), dtype=H.dtype)
    nfall, kappa = 0, []
    for i, S in enumerate(pattern):
        S = list(S)
        m = len(S)
        blk = H[np.ix_(S, S)]
        ok = bool(np.all(np.isfinite(blk)))
        if ok:
            try:
                np.linalg.cholesky(blk)
            except np.linalg.LinAlgError:
                ok = False
        if ok:
            e = np.zeros(m, dtype=H.dtype)
            e[-1] = 1
            y = np.linalg.solve(blk, e)
            G[i, S] = np.conj(y) / np.sqrt(y[-1].real)
            kappa.append(np.linalg.cond(blk))
        else:
            a = abs(H[i, i].real)
            G[i, i] = 1 / np.sqrt(a) if (a > 0 and np.isfinite(a)) else 1.0
            nfall += 1
            kappa.append(np.inf)
    return G, nfall, np.array(kappa)


def g_dense(P):
    """dense (nb, N, N) numpy G of an FSAIOperator"""
    G = P.G
    N = G.shape[-1]
    return dense_of(G.crow.cpu().numpy(), G.col.cpu().numpy(), G.values.detach().cpu().numpy(), N)


def random_hpd(dtype, nb=2, seed=0, density=0.12, n=61, full=True):
    """random sparse Hermitian with the constant diagonal 2 max_i sum_j |a_ij| + 1: by Gershgorin the spectrum of every
    principal block lies in [d - s, d + s] with d = 2 s + 1, so kappa_2 < 3.  CSR host arrays with unsorted columns;
    full: both triangles stored"""
    rng = np.random.default_rng(seed)
    cplx = dtype.is_complex
    mask = np.tril(rng.random((n, n)) < density, -1)
    low = np.zeros((nb, n, n), dtype=np.complex128 if cplx else np.float64)
    for b in range(nb):
        v = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if cplx else 0)
        low[b] = np.where(mask, v, 0)
    H = low + np.conj(np.swapaxes(low, 1, 2))
    off = np.abs(H).sum(-1)
    for b in range(nb):
        H[b] += (2 * off[b].max() + 1) * np.eye(n)
    S = mask | mask.T | np.eye(n, dtype=bool) if full else mask | np.eye(n, dtype=bool)
    rows, cols = np.nonzero(S)
    perm = np.lexsort((rng.random(rows.size), rows))                 # unsorted columns inside each row
    rows, cols = rows[perm], cols[perm]
    crow = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=crow[1:])
    vals = H[:, rows, cols]
    return crow, cols, vals, H


def check_rows(Gd, Ad, pattern, dtype, c=16):
    """per entry against the dense restatement, and the three exact properties in double"""
    eps = torch.finfo(dtype).eps
    Gr, nfall, kap = fsai_dense(Ad, pattern)
    assert nfall == 0
    for i, S in enumerate(pattern):
        assert set(np.nonzero(Gd[i])[0]) <= set(S)
        err = np.abs(Gd[i] - Gr[i]).max()
        bound = c * len(S) * eps * kap[i] * np.abs(Gr[i]).max()
        assert err <= bound, (i, err, bound)
    H = hermitian_from_lower(Ad)
    G = Gd.astype(np.complex128 if np.iscomplexobj(Gd) else np.float64)
    GA = G @ H
    assert np.abs(np.diag(GA @ np.conj(G.T)) - 1).max() <= 64 * len(max(pattern, key=len)) * eps
    for i, S in enumerate(pattern):
        for j in S[:-1]:
            assert abs(GA[i, j]) <= 64 * len(S) * eps * np.abs(G[i]).max() * np.abs(H[S, j]).sum(), (i, j)
    d = np.diag(Gd)
    assert np.all(d.real > 0) and np.all(d.imag == 0)
