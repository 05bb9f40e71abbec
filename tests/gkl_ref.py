"""float64 / complex128 restatement of the Golub-Kahan-Lanczos kernels (xk_gkl.hip) and the error bounds the tests use.

`sweep` restates xk_gkl_sweep_* (update, rounding to the storage type, partial sums per chunk), `finish` restates
xk_gkl_finish, `jacobi_values` is a model of the one-sided (Hestenes) Jacobi of xk_gkl_bsvd that reports the singular
values only (compared with numpy.linalg.svd).  Nothing here imports the package.

Bounds (u = unit roundoff of the storage type, u64 = 2^-53, L = chunk length, j = basis rows):
  dst      the kernel evaluates s * (w - sum_i c_i q_i) in double — j products and j + 1 additions and one product, each
           within (1 + u64) — and rounds once:   |dst - exact| <= u |exact| + (j + 3) u64 |s| (|w| + sum_i |c_i| |q_i|)
  partial  a dot over a chunk of the values AS STORED: sum_n |q_n| * (bound of dst_n)   (a stored value may differ
           from the restated one by that much) + (L + 2) u64 sum_n |q_n| |dst_n|          (the summation itself)
  CGS2     two passes of classical Gram-Schmidt against j orthonormal vectors leave |Q^H q| <= ORTH_C u sqrt(j) per
           vector when the first pass does not cancel more than half the digits (Giraud, Langou, Rozloznik, van den
           Eshof, Numer. Math. 101 (2005) 87, Theorem 2): the basis of ncv vectors has max|Q^H Q - I| <= ORTH_C u ncv
           with ORTH_C below.  ORTH_C = 8 covers the rounding of the update (3 operations per row and element), of the
           normalisation (2) and of the norm (1), and a factor for the restart rotations, which multiply an orthonormal
           basis by an orthogonal matrix known to 6 u64 n sweeps (see `jacobi_bound`).
"""
from fractions import Fraction
import numpy as np

U64 = 2.0 ** -53
ORTH_C = 8.0


def unit_roundoff(dtype):
    return {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24,
            np.dtype(np.complex128): 2.0 ** -53, np.dtype(np.complex64): 2.0 ** -24}[np.dtype(dtype)]


def chunk_elems(dtype):
    """elements per chunk of the sweep: 64 vectors of 16 B"""
    return 64 * 16 // np.dtype(dtype).itemsize


def sweep(Q, w, coef, scale, j, N, dtype):
    """Q (cap, >=N) rows, w (>=N,), coef (j,) or None, scale float or None, all in float64 / complex128.
    Returns dst (N,) as stored (rounded to dtype, then widened), its bound (N,), part (nval, nchunk) with nval = j
    (complex: 2j, re / im interleaved) + 1, and the bound of part."""
    cplx = np.dtype(dtype).kind == "c"
    wide = np.complex128 if cplx else np.float64
    u = unit_roundoff(dtype)
    s = 1.0 if scale is None else float(scale)
    Qj = np.asarray(Q[:j, :N], dtype=wide)
    x = np.asarray(w[:N], dtype=wide).copy()
    mag = np.abs(x)
    if coef is not None and j > 0:
        c = np.asarray(coef[:j], dtype=wide)
        x = x - c @ Qj
        mag = mag + np.abs(c) @ np.abs(Qj)
    exact = s * x
    dst = exact.astype(dtype).astype(wide)
    dst_bound = u * np.abs(exact) + (j + 3) * U64 * abs(s) * mag * (2.0 if cplx else 1.0)
    L = chunk_elems(dtype)
    nchunk = (N + L - 1) // L
    nval = (2 * j if cplx else j) + 1
    part = np.zeros((nval, nchunk))
    pbound = np.zeros((nval, nchunk))
    for ch in range(nchunk):
        sl = slice(ch * L, min(N, (ch + 1) * L))
        d, db = dst[sl], dst_bound[sl]
        for i in range(j):
            q = Qj[i, sl]
            dot = np.sum(np.conj(q) * d)
            bnd = np.sum(np.abs(q) * db) + (2 * L + 2) * U64 * np.sum(np.abs(q) * np.abs(d))
            if cplx:
                part[2 * i, ch], part[2 * i + 1, ch] = dot.real, dot.imag
                pbound[2 * i, ch] = pbound[2 * i + 1, ch] = bnd
            else:
                part[i, ch] = dot
                pbound[i, ch] = bnd
        part[nval - 1, ch] = np.sum(np.abs(d) ** 2)
        pbound[nval - 1, ch] = 2.0 * np.sum(np.abs(d) * db) + (2 * L + 2) * U64 * part[nval - 1, ch]
    return dst, dst_bound, part, pbound


def finish(part):
    """(coefficients (nval - 1,), norm) of one sweep's partials (nval, nchunk)"""
    sums = part.sum(axis=1)
    return sums[:-1], float(np.sqrt(max(sums[-1], 0.0)))


def _fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic, then one rounding)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _pair_sums(W, p, q, fused):
    """(|w_p|^2, |w_q|^2, w_p . w_q); fused: as the kernel forms them — 8 lanes take rows l, l + 8, ... with fused
    multiply-adds, then a butterfly over the lanes"""
    if not fused:
        return W[:, p] @ W[:, p], W[:, q] @ W[:, q], W[:, p] @ W[:, q]
    acc = [[0.0] * 8 for _ in range(3)]
    for i in range(W.shape[0]):
        x, y = W[i, p], W[i, q]
        lane = i % 8
        acc[0][lane], acc[1][lane], acc[2][lane] = _fma(x, x, acc[0][lane]), _fma(y, y, acc[1][lane]), \
            _fma(x, y, acc[2][lane])
    for msk in (1, 2, 4):
        acc = [[v[i] + v[i ^ msk] for i in range(8)] for v in acc]
    return acc[0][0], acc[1][0], acc[2][0]


def jacobi_values(B, max_sweeps=40, fused=False):
    """one-sided Jacobi on the columns of the square matrix B, round-robin pairs, the kernel's threshold
    sqrt(n) * eps and its rule for null columns; fused: sums and rotations with fused multiply-adds, as the compiler
    contracts them on the device (slow: exact rational arithmetic).  Returns (singular values descending, sweeps)"""
    W = np.array(B, dtype=np.float64)
    n = W.shape[0]
    m = n + (n & 1)
    tol = np.sqrt(n) * np.finfo(np.float64).eps
    dnull = np.finfo(np.float64).eps * np.linalg.norm(W)       # columns this short are null columns: left alone
    sweeps = 0
    while sweeps < max_sweeps:
        rotated = False
        for r in range(max(m - 1, 1) if n > 1 else 0):
            for g in range(m // 2):
                p = (r + g) % (m - 1)
                q = m - 1 if g == 0 else (r + (m - 1) - g) % (m - 1)
                p, q = min(p, q), max(p, q)
                if q >= n:
                    continue
                a, d, c = _pair_sums(W, p, q, fused)
                sa, sd = np.sqrt(a), np.sqrt(d)
                if c != 0.0 and sa > dnull and sd > dnull and abs(c) > tol * sa * sd:
                    zeta = (d - a) / (2.0 * c)
                    t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    if t == 0.0:
                        continue
                    rotated = True
                    cs = 1.0 / np.sqrt(1.0 + t * t)
                    sn = cs * t
                    wp, wq = W[:, p].copy(), W[:, q].copy()
                    if fused:
                        for i in range(n):
                            W[i, p], W[i, q] = _fma(cs, wp[i], -(sn * wq[i])), _fma(sn, wp[i], cs * wq[i])
                    else:
                        W[:, p], W[:, q] = cs * wp - sn * wq, sn * wp + cs * wq
        sweeps += 1
        if not rotated:
            break
    return np.sort(np.linalg.norm(W, axis=0))[::-1], sweeps


def jacobi_bound(B, sweeps):
    """absolute bound of the singular values / of |P diag(s) Q^T - B| entries / of the vectors' orthonormality times
    sigma_max: every rotation perturbs its two columns by at most 6 u64 of their length, a column meets n - 1 rotations
    per sweep:  6 u64 n sweeps |B|_F; a column left alone because it is no longer than eps |B|_F = 2 u64 |B|_F moves the
    values by at most its length, which the bound covers"""
    n = B.shape[0]
    return 6.0 * U64 * n * max(sweeps, 1) * max(np.linalg.norm(B), np.finfo(np.float64).tiny)


def arrow_bidiagonal(n, keep, rng, graded=False):
    """upper triangular n x n: diag(keep values) with the arrow in column `keep`, upper bidiagonal after it"""
    B = np.zeros((n, n))
    d = rng.uniform(0.5, 2.0, n)
    e = rng.uniform(0.1, 1.0, n)
    if graded:
        g = 10.0 ** (-12.0 * np.arange(n) / max(n - 1, 1))
        d, e = d * g, e * g
    keep = min(keep, n - 1)
    for i in range(n):
        B[i, i] = d[i]
        if i < keep:
            B[i, keep] = e[i] * (-1.0) ** i
        elif i + 1 < n:
            B[i, i + 1] = e[i]
    return B


def projected_cases():
    """name -> matrix: the orders and kinds the issue lists"""
    rng = np.random.default_rng(20051)
    cases = {}
    for n in (2, 3, 17, 64):
        cases["arrow%d" % n] = arrow_bidiagonal(n, n // 3, rng)
        cases["graded%d" % n] = arrow_bidiagonal(n, n // 3, rng, graded=True)
    cases["zero17"] = np.zeros((17, 17))
    rep = np.diag([3.0, 3.0, 3.0, 1.0, 1.0, 0.5, 0.5, 0.5])
    rep[0, 5] = 0.0
    cases["repeated8"] = rep
    rep64 = arrow_bidiagonal(64, 20, rng)
    rep64[:20, 20] = 0.0
    rep64[np.arange(20), np.arange(20)] = 2.0
    cases["repeated64"] = rep64
    # rank 8 with 20 zero rows: 28 columns inside an 8-dimensional space, what a basis that outgrew the rank of the
    # operator leaves (every later alpha and beta a breakdown); the null columns are noise inside the span of the others
    low = np.triu(rng.standard_normal((28, 28)))
    low[8:, :] = 0.0
    cases["rankdef28"] = low
    return cases
