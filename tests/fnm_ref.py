"""Float64 restatement of f(A) b by two-pass Lanczos (xk_fnm.hip, linalg/native_fnm.py, host_slq.funm), written from
the formulas, with the error bounds the tests use.

Pass 1 is the recurrence of tests/slq_ref.py on the UN-normalised vectors r2_k = beta_k v_k; it records alpha_k, beta_k
and m.  With T = Q diag(theta) Q^T the m x m Jacobi matrix,
    c = |b| Q f(theta) Q^T e_1,       f(A) b ~ sum_k c_k v_k = sum_k (c_k / beta_k) r2_k.
Pass 2 runs the recurrence again from the recorded scalars -- the same expressions on the same numbers, so the same
bits -- and accumulates X.

`funm` is the whole iteration for one system: the vector operations rounded to `arith` (float64 / float32 / complex128 /
complex64), the scalars in double, the small problem by numpy.linalg.eigh (or by `ql_vectors`, the plain-Python
statement of xk_fnm_eig: the implicit QL of slq_ref.ql_first_row with every row of the rotation product carried).
`step` restates xk_fnm_step per entry, `coeff` xk_fnm_coeff.

Bounds.  eps_T is the machine epsilon of the kernel dtype, EPS64 = 2^-52.
  * xk_fnm_step, X: C_X eps_T (|X_i| + sum of the |products| added to it), C_X = 4: the cast of c_k / beta_k, one
    product and one addition per term are at most 3 (real) or 6 (complex, two products) roundings of eps_T / 2 on
    partial sums no larger than the sum of the magnitudes.  y: the bound of slq_ref.step.
  * xk_fnm_coeff after xk_fnm_eig, against numpy.linalg.eigh of the same T, in the 2-norm:
    C_K m EPS64 |b| (max_k |f(theta_k)| + |T|_inf max_k |f'(theta_k)|): the eigenvectors of a tridiagonal matrix are not
    individually stable, but f(T) e_1 is a smooth function of T and QL is backward stable: the computed Q, theta are
    exact for T + E with |E| = O(m EPS64 |T|) and Q orthogonal to O(m EPS64).  C_K = 4 is the smallest power of two
    that leaves the Python QL a margin of at least 4 on the inputs of the kernel test (`eig_cases`: nsteps in {1, 2, 3,
    17, 64, 128}, S in {1, 70}, kappa in {1e2, 1e6}, mixed m_s, every named function): tests/test_fnm_ref.py measures
    the worst ratio 0.168 (margin 6.0; at nsteps = 3, S = 70, on a system with m = 2, where the factor m understates
    the handful of roundings of f itself; C_K = 2 would leave a margin of 3.0) and asserts the margin.  On full-length
    matrices alone (m = nsteps) the worst ratio is 0.050.
"""
import math
import numpy as np
import torch
from tests import slq_ref as sref

EPS64 = sref.EPS64
BREAK = sref.BREAK
C_X = 4.0
C_Y = sref.C_Y
C_K = 4.0
C_QORTH = 64.0
FN_CODES = sref.FN_CODES
NEEDS_POSITIVE = sref.NEEDS_POSITIVE
ARITH = {torch.float64: np.float64, torch.float32: np.float32, torch.complex128: np.complex128,
         torch.complex64: np.complex64}
_c = lambda t: t.unsqueeze(-1)


def eps_arith(arith):
    return float(np.finfo(arith).eps)


# ------------------------------------------------------------------------------------------------ the small problem
def ql_vectors(d, e):
    """implicit QL of the symmetric tridiagonal (d, e) with the whole rotation product accumulated: eigenvalues
    (unsorted), Z with Z[j, k] = component j of the eigenvector of d[k], and `ok` (False when an eigenvalue took more
    than 60 iterations).  The statement of xk_fnm_eig, operation for operation."""
    n = len(d)
    d = np.array(d, dtype=np.float64)
    e = np.append(np.array(e, dtype=np.float64), 0.0)
    Z = np.eye(n)
    eps = np.finfo(np.float64).eps
    for l in range(n):
        it = 0
        while True:
            m = l
            while m < n - 1:
                dd = abs(d[m]) + abs(d[m + 1])
                if not abs(e[m]) > eps * dd:
                    break
                m += 1
            if m == l:
                break
            if it == 60:
                return d, Z, False
            it += 1
            g = (d[l + 1] - d[l]) / (2 * e[l])
            r = math.hypot(g, 1.0)
            g = d[m] - d[l] + e[l] / (g + math.copysign(r, g))
            s = c = 1.0
            p = 0.0
            for i in range(m - 1, l - 1, -1):
                f, b = s * e[i], c * e[i]
                r = math.hypot(f, g)
                e[i + 1] = r
                if r == 0:
                    d[i + 1] -= p
                    e[m] = 0.0
                    break
                s, c = f / r, g / r
                g = d[i + 1] - p
                r = (d[i] - g) * s + 2 * c * b
                p = s * r
                d[i + 1] = g + p
                g = c * r - b
                lo, hi = Z[:, i].copy(), Z[:, i + 1].copy()
                Z[:, i + 1] = s * lo + c * hi
                Z[:, i] = c * lo - s * hi
            else:
                d[l] -= p
                e[l] = g
                e[m] = 0.0
    return d, Z, True


def coeff_of(theta, Z, f, bnorm):
    """c_j = |b| sum_k Z[j, k] f_k Z[0, k], k ascending (the order of xk_fnm_coeff)"""
    c = np.zeros(len(theta), dtype=np.result_type(f.dtype, np.float64))
    for k in range(len(theta)):
        c = c + (Z[:, k] * Z[0, k]) * f[k]
    return bnorm * c


def tail_of(c):
    m = len(c)
    return float(np.linalg.norm(c[m - 4:]) / np.linalg.norm(c)) if m > 4 else 0.0


def coeff(al, be, m, zz, name=None, t=1.0, fvals=None, eig=None):
    """xk_fnm_eig + xk_fnm_coeff for one system by `ql_vectors` (`eig`: its result, where the caller has it already):
    (theta, Z, C, tail, flag)"""
    d, Z, ok = ql_vectors(al[:m], be[1:m]) if eig is None else eig
    flag = 0 if ok else 2
    with np.errstate(all="ignore"):
        if fvals is not None:
            f = np.asarray(fvals)[:m]
        else:
            if name in NEEDS_POSITIVE and not bool((d > 0).all()):
                flag |= 1
            f = sref.fn_of(name, t)[0](d)
        c = coeff_of(d, Z, f, math.sqrt(zz))
    if flag:
        c = np.full(m, math.nan)
    return d, Z, c, (tail_of(c) if not flag else math.nan), flag


def coeff_truth(al, be, m, zz, name, t=1.0):
    """numpy.linalg.eigh of the same T: (C, bound of its 2-norm error as in the module docstring)"""
    if m == 0:
        return np.zeros(0), 0.0
    T = sref.jacobi(al, be, m)
    th, U = np.linalg.eigh(T)
    f, df = sref.fn_of(name, t)
    with np.errstate(all="ignore"):
        c = math.sqrt(zz) * (U @ (f(th) * U[0]))
        tn = np.abs(T).sum(1).max()
        bound = float(C_K * m * EPS64 * math.sqrt(zz) * (np.abs(f(th)).max() + tn * np.abs(df(th)).max()))
    return c, bound


DECOUPLED, INDEFINITE, ZERO = 5, 9, 11


def eig_cases(lanczos_T, nsteps, S):
    """the inputs of the xk_fnm_eig / xk_fnm_coeff tests: S Lanczos-shaped Jacobi matrices (`lanczos_T(rng, m, kappa)`
    of tests/test_gpu_slq_kernels.py, kappa 1e6 and 1e2 in turn) of mixed m_s <= nsteps (system 0: the full count),
    system DECOUPLED with a zero off-diagonal entry, system INDEFINITE with its smallest node at -0.5, system ZERO
    with b = 0.  Returns Tal, Tbe (S, nsteps) and state (2, S, NST), NaN where nothing is to be read, the state slot
    k = nsteps & 1, and the lists of m_s and |b_s|^2."""
    rng = np.random.default_rng(nsteps * 100 + S)
    k = nsteps & 1
    Tal = np.full((S, nsteps), math.nan)
    Tbe = np.full((S, nsteps), math.nan)
    state = np.full((2, S, sref.NST), math.nan)
    ms, zzs = [], []
    for s in range(S):
        m = nsteps if s == 0 else 1 + (7 * s) % nsteps
        if s == ZERO:
            m = 0
        al, be, zz = lanczos_T(rng, max(m, 1), 1e2 if s % 2 else 1e6)
        if s == DECOUPLED and m >= 3:
            be[m // 2] = 0.0
        if s == INDEFINITE:
            al = al - (np.linalg.eigvalsh(sref.jacobi(al, be, m)).min() + 0.5)
        Tal[s, :m], Tbe[s, :m] = al[:m], be[:m]
        state[k, s] = 0.0
        state[k, s, sref.M], state[k, s, sref.ZNORM2] = m, (zz if m else 0.0)
        state[k, s, sref.FLAG] = 0.0 if m else 2.0
        ms.append(m)
        zzs.append(zz if m else 0.0)
    return Tal, Tbe, state, k, ms, zzs


# ------------------------------------------------------------------------------------------------ whole iteration
def lanczos(A, b, nsteps, arith):
    """pass 1 for one system (slq_ref.forms, real or complex): alpha, beta (nsteps,), m, |b|^2 and, for the replay
    tests, the list of the vectors r2_0 .. r2_{m-1} the steps ran on"""
    A, b = np.asarray(A).astype(arith), np.asarray(b).astype(arith)
    eps = float(np.finfo(arith).eps)
    rd = np.finfo(arith).dtype
    dot = lambda x, y: float((np.conj(x) * y).sum(dtype=arith).real)
    zz = dot(b, b)
    beta, oldb, m, tnorm, rowp = math.sqrt(zz), 0.0, 0, 0.0, 0.0
    r2, r1 = b.copy(), np.zeros_like(b)
    al, be = np.zeros(nsteps), np.zeros(nsteps)
    vecs = []
    for k in range(nsteps):
        if zz == 0:
            break
        W = A @ r2
        first = m == 0
        if not first:
            nb = math.sqrt(dot(r2, r2))
            tnorm = max(tnorm, rowp + nb)
            if nb <= BREAK * eps * tnorm:
                break
            oldb, beta = beta, nb
        alpha = dot(r2, W) / (beta * beta)
        vecs.append(r2)
        y = W * rd.type(1.0 / beta) - rd.type(alpha / beta) * r2
        if not first:
            y = y - rd.type(beta / oldb) * r1
        r1, r2 = r2, y
        al[m], be[m] = alpha, beta
        rowp = abs(alpha) + (0.0 if first else beta)
        m += 1
    return al, be, m, zz, vecs


def replay(A, b, al, be, m, c, arith):
    """pass 2 for one system: X = sum_k (c_k / beta_k) r2_k with the vectors regenerated from al, be.  Returns X and the
    list of the regenerated vectors."""
    A, b = np.asarray(A).astype(arith), np.asarray(b).astype(arith)
    rd = np.finfo(arith).dtype
    r2, r1 = b.copy(), np.zeros_like(b)
    X = np.zeros_like(b)
    vecs = []
    for k in range(m):
        alpha, beta = al[k], be[k]
        vecs.append(r2)
        X = X + np.asarray(c[k] / beta).astype(arith) * r2
        if k + 1 == m:
            break
        W = A @ r2
        y = W * rd.type(1.0 / beta) - rd.type(alpha / beta) * r2
        if k > 0:
            y = y - rd.type(beta / be[k - 1]) * r1
        r1, r2 = r2, y
    return X, vecs


def funm(A, b, nsteps, f, arith=np.float64, ql=False):
    """f(A) b for one system; `f` maps a float64 array of nodes to values (real or complex).  Returns (x, m, tail)."""
    al, be, m, zz, _ = lanczos(A, b, nsteps, arith)
    if m == 0:
        return np.zeros_like(np.asarray(b).astype(arith)), 0, 0.0
    if ql:
        th, Z, ok = ql_vectors(al[:m], be[1:m])
    else:
        th, Z = np.linalg.eigh(sref.jacobi(al, be, m))
    with np.errstate(all="ignore"):
        c = coeff_of(th, Z, np.asarray(f(th)), math.sqrt(zz))
    x, _ = replay(A, b, al, be, m, c, arith)
    return x, m, tail_of(c)


def dense_truth(A, b, f):
    """f(A) b by a dense eigendecomposition in double"""
    A = np.asarray(A).astype(np.complex128 if np.iscomplexobj(A) else np.float64)
    lam, U = np.linalg.eigh(A)
    return U @ (np.asarray(f(lam)) * (U.conj().T @ np.asarray(b).astype(A.dtype)))


def hpd_matrix(rng, n, kappa, cplx=False):
    """A = Q diag(geomspace(1, kappa, n)) Q^H with a random unitary Q"""
    lam = np.geomspace(1.0, kappa, n)
    G = rng.standard_normal((n, n))
    if cplx:
        G = G + 1j * rng.standard_normal((n, n))
    Q, _ = np.linalg.qr(G)
    A = (Q * lam) @ Q.conj().T
    return (A + A.conj().T) / 2


# ------------------------------------------------------------------------------------------------ xk_fnm_step
def step(env, W, r2, r1, X, C, Tal, Tbe, state, k, kstate, last):
    """xk_fnm_step on the real views W, r2, r1, X (S, n) float64 of the kernel's arrays (complex: interleaved), C
    (S, nsteps) or (S, nsteps, 2), Tal, Tbe (S, nsteps), state (2, S, NST).  Returns X: (value, bound), y: (value,
    bound) of what r1 holds afterwards, and the masks live (X updated) and moved (r1 written)."""
    eps = sref.eps_of(env.dtype)
    st = state[kstate & 1].detach().cpu().to(torch.float64)
    md = st[:, sref.M]
    live = (st[:, sref.FLAG] != 2) & (md > k)
    moved = live & (md > k + 1) & (not last)
    one = torch.ones_like(md)
    beta = torch.where(live, Tbe[:, k], one)
    alpha = torch.where(live, Tal[:, k], one)
    oldb = torch.where(live, Tbe[:, k - 1], one) if k > 0 else one
    if env.cplx:
        cr, ci = C[:, k, 0] / beta, C[:, k, 1] / beta
        a = r2.reshape(env.S, env.N, 2)
        pr = torch.stack([_c(cr) * a[..., 0], _c(cr) * a[..., 1]], -1).reshape(env.S, env.n)
        pi = torch.stack([-_c(ci) * a[..., 1], _c(ci) * a[..., 0]], -1).reshape(env.S, env.n)
    else:
        pr, pi = _c(C[:, k] / beta) * r2, torch.zeros_like(r2)
    L = _c(live)
    xn = torch.where(L, X + pr + pi, X)
    ex = torch.where(L, C_X * eps * (X.abs() + pr.abs() + pi.abs()), torch.zeros_like(X))
    c0, c2 = 1.0 / beta, alpha / beta
    c1 = beta / oldb if k > 0 else torch.zeros_like(beta)
    r1z = r1 if k > 0 else torch.zeros_like(r1)
    t0, t2, t1 = W * _c(c0), _c(c2) * r2, _c(c1) * r1z
    Mv = _c(moved)
    y = torch.where(Mv, (t0 - t2) - t1, r1)
    ey = torch.where(Mv, C_Y * eps * (t0.abs() + t2.abs() + t1.abs()), torch.zeros_like(y))
    return {"X": (xn, ex), "y": (y, ey), "live": live, "moved": moved}
