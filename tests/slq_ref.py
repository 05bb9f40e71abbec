"""Float64 restatement of the Lanczos quadrature kernels of xk_slq.hip (xk_slq_init, xk_slq_step, xk_slq_quad) and of
the whole iteration, with per-entry error bounds, in the manner of tests/lsmr_ref.py.

The recurrence is Lanczos on the UN-normalised vectors r2 = beta_k v_k:
    beta  = |r2|  (first step: the state's beta_1 = |z|; later: sqrt of the sum of the partials the step before wrote)
    tnorm = max(tnorm, rowp + beta)              (not on a first step; rowp = |alpha| + beta of the last row)
    beta <= BREAK eps_T tnorm: the system is frozen (flag 1), nothing else of it is written
    alpha = sum Pa / beta^2                      (Pa: partials of <r2, W>, W = A r2)
    y     = (W (1/beta) - (alpha/beta) r2) - (beta/oldb) r1      over r1 (first step: no r1 term, r1 is not read)
    T[m]  = (alpha, beta), m <- m + 1, rowp = |alpha| + beta (first step: |alpha|)
Complex systems: every scalar is real, so the kernels run on the interleaved (re, im) storage as real vectors of length
2N; so do the functions here (`Env.vec`, from tests/minres_ref.py).  Pb and Pa are xk_kry_dots partials: (re, im) pairs
for the complex types, of which the real part is summed.

Bounds.  eps_T is the machine epsilon of the kernel dtype, EPS64 = 2^-52.
  * y:  C_Y eps_T (|W_i| / beta + |alpha / beta| |r2_i| + (beta / oldb) |r1_i|), C_Y = 4: two casts, two or three
    products and two subtractions are at most 7 roundings of eps_T / 2 each on the largest term.  Nothing is added
    for the double scalars 1/beta, alpha/beta, beta/oldb: `psum` adds the partials in the kernels' own fixed order (the
    64-lane butterfly of reduce_partials_d), so the restatement forms them from the very sums the kernel forms.
  * block partials of |y|^2, against the sum of the squares of the y the kernel itself wrote:
    (elements per block + 4) eps_T sum y_i^2.
  * alpha, beta, the state: 8 EPS64 relative to the value itself (the sums are the kernels' bit for bit; what is left
    is a square root, a division and a few additions).
  * xk_slq_quad against numpy.linalg.eigh of the same T:
    C_Q m EPS64 |z|^2 sum_k tau_k^2 (|f(theta_k)| + |T|_inf |f'(theta_k)|), C_Q = 4: eigenvalues of a symmetric
    tridiagonal matrix move by O(m EPS64 |T|) under the QL iteration and so do the weights relative to themselves.
    Measured with C_Q = 4 over every fn code: the Python QL below reaches 0.164 of the bound (tests/test_slq_ref.py: m in
    {1, 2, 3, 8, 16, 33, 64, 128}, kappa in {1e2, 1e6}; 0.66 with constant 1) and xk_slq_quad 0.178 on an MI355X
    (0.71 with constant 1): the margin over the constant 1 is about 1.4, not 4.
"""
import math
import numpy as np
import torch
from tests import krylov_ref as kref
from tests import minres_ref as mref

NST = 8
BETA, OLDB, FLAG, M, TNORM, ROWP, ZNORM2, ALPHA = range(NST)
BREAK = 64.0
MAX_STEPS = 128
EPS64 = 2.0 ** -52
C_Y = 4.0
C_Q = 4.0
C_ST = 8.0
FN_CODES = {"log": 0, "inv": 1, "sqrt": 2, "invsqrt": 3, "exp": 4, "identity": 5}
NEEDS_POSITIVE = ("log", "inv", "sqrt", "invsqrt")

Env = mref.Env
_c = lambda t: t.unsqueeze(-1)


def eps_of(dtype):
    return float(torch.finfo(kref.REAL_OF[dtype]).eps)


_LANES = torch.arange(64)


def psum(P, nblk):
    """the kernels' double sum of the real parts of the used partial slots, in the kernels' own order: lane i of a wave
    holds partial i (0 beyond nblk) and wave_sum (xk_common.h) is the butterfly v += v[partner], partner = lane ^ 32,
    ^ 16, ^ 8, then lane ^ 7 (the row_half_mirror exchange of the stage over bit 2), ^ 2, ^ 1; lane 0's total is used"""
    P = P.detach().cpu().to(torch.float64)
    if P.dim() == 3:
        P = P[..., 0]
    v = torch.zeros(P.shape[0], 64, dtype=torch.float64)
    v[:, :nblk] = P[:, :nblk]
    for d in (32, 16, 8, 7, 2, 1):
        v = v + v[:, _LANES ^ d]
    return v[:, 0]


# ------------------------------------------------------------------------------------------------ the kernels
def init(env, Pb):
    """xk_slq_init: the start state (value, bound); r2 is a bit copy of z"""
    bb = psum(Pb, env.nblk)
    st = torch.zeros(env.S, NST, dtype=torch.float64)
    est = torch.zeros_like(st)
    st[:, BETA], st[:, ZNORM2] = bb.clamp(min=0).sqrt(), bb
    st[:, FLAG] = torch.where(bb == 0, 2.0, 0.0).to(torch.float64)
    est[:, ZNORM2] = C_ST * EPS64 * bb.abs()
    est[:, BETA] = C_ST * EPS64 * st[:, BETA]
    return {"state": (st, est)}


def step(env, W, r2, r1, Pa, Pin, state, k, nsteps):
    """xk_slq_step on the real views W, r2, r1 (S, n) float64 of the kernel's inputs.  Returns
    y: (value, bound) of what r1 holds afterwards (frozen systems: r1 itself, bound 0), state: (value, bound) of slot
    (k + 1) & 1, alpha / beta: (value, bound) of the T entries written, col: the column of T written, and the masks
    frozen (on entry), broke (frozen by this step), live."""
    eps = eps_of(env.dtype)
    st = state[k & 1].detach().cpu().to(torch.float64)
    md = st[:, M]
    frozen = (st[:, FLAG] != 0) | ~((md >= 0) & (md < nsteps))
    first = md == 0
    pin = psum(Pin, env.nblk)
    pin = torch.where(first | frozen, torch.ones_like(pin), pin)
    beta = torch.where(first, st[:, BETA], pin.clamp(min=0).sqrt())
    oldb = torch.where(first, torch.zeros_like(beta), st[:, BETA])
    tnorm = torch.maximum(st[:, TNORM], st[:, ROWP] + torch.where(first, torch.zeros_like(beta), beta))
    broke = ~frozen & ~first & (beta <= BREAK * eps * tnorm)
    live = ~frozen & ~broke
    sb = torch.where(live, beta, torch.ones_like(beta))
    alpha = psum(Pa, env.nblk) / (sb * sb)
    ealpha = C_ST * EPS64 * alpha.abs()
    ebeta = C_ST * EPS64 * beta
    c0, c2 = 1.0 / sb, alpha / sb
    c1 = torch.where(first, torch.zeros_like(beta), sb / torch.where(first | ~live, torch.ones_like(oldb), oldb))
    r1z = torch.where(_c(first), torch.zeros_like(r1), r1)
    t0, t2, t1 = W * _c(c0), _c(c2) * r2, _c(c1) * r1z
    y = (t0 - t2) - t1
    ey = C_Y * eps * (t0.abs() + t2.abs() + t1.abs())
    L = _c(live)
    out_y = torch.where(L, y, r1)
    ey = torch.where(L, ey, torch.zeros_like(ey))
    so, eso = st.clone(), torch.zeros_like(st)
    so[:, FLAG] = torch.where(broke, 1.0, st[:, FLAG].double())
    so[:, TNORM] = torch.where(frozen, st[:, TNORM], tnorm)
    rowp = alpha.abs() + torch.where(first, torch.zeros_like(beta), beta)
    for i, (v, e) in ((BETA, (beta, ebeta)), (OLDB, (oldb, torch.zeros_like(beta))), (M, (md + 1, torch.zeros_like(md))),
                      (ROWP, (rowp, ealpha + ebeta)), (ALPHA, (alpha, ealpha))):
        so[:, i] = torch.where(live, v, st[:, i])
        eso[:, i] = torch.where(live, e, torch.zeros_like(e))
    eso[:, TNORM] = torch.where(frozen, torch.zeros_like(beta), C_ST * EPS64 * tnorm)
    return {"y": (out_y, ey), "state": (so, eso), "alpha": (alpha, ealpha), "beta": (beta, ebeta),
            "col": md.to(torch.int64), "frozen": frozen, "broke": broke, "live": live}


def block_sums(env, y):
    """(S, nblk) float64 sums of y^2 over the kernel's block ranges and the number of elements of each block"""
    ctx = env.rctx
    sums = kref._block_dots(ctx, y, y)
    cnt = []
    for blk in range(ctx.nblk):
        lo, hi = kref.block_range(ctx.N, ctx.nblk, blk, ctx.vn)
        cnt.append(max(0, min(hi, ctx.N) - min(lo, ctx.N)))
    return sums, torch.tensor(cnt, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ the quadrature
def ql_first_row(d, e):
    """implicit QL of the symmetric tridiagonal (d, e) with the first row of the rotations carried along (Golub &
    Welsch): eigenvalues (unsorted) and squared first eigenvector components; `ok` False when an eigenvalue took more
    than 60 iterations.  The statement of xk_slq_quad, operation for operation."""
    n = len(d)
    d = np.array(d, dtype=np.float64)
    e = np.append(np.array(e, dtype=np.float64), 0.0)
    z = np.zeros(n)
    if n:
        z[0] = 1.0
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
                return d, z * z, False
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
                f = z[i + 1]
                z[i + 1] = s * z[i] + c * f
                z[i] = c * z[i] - s * f
            else:
                d[l] -= p
                e[l] = g
                e[m] = 0.0
    return d, z * z, True


def fn_of(name, t=1.0):
    """(f, |f'|) of a named function on numpy arrays"""
    return {"log": (np.log, lambda x: 1 / np.abs(x)),
            "inv": (lambda x: 1 / x, lambda x: 1 / x ** 2),
            "sqrt": (np.sqrt, lambda x: 0.5 / np.sqrt(x)),
            "invsqrt": (lambda x: 1 / np.sqrt(x), lambda x: 0.5 * np.abs(x) ** -1.5),
            "exp": (lambda x: np.exp(t * x), lambda x: abs(t) * np.exp(t * x)),
            "identity": (lambda x: x, lambda x: np.ones_like(x))}[name]


def jacobi(al, be, m):
    """the m x m Jacobi matrix of one system: diag(al[:m]), off-diagonal be[1:m]"""
    al, be = np.asarray(al, dtype=np.float64), np.asarray(be, dtype=np.float64)
    T = np.diag(al[:m])
    if m > 1:
        T = T + np.diag(be[1:m], 1) + np.diag(be[1:m], -1)
    return T


def quad(al, be, m, zz, name, t=1.0):
    """xk_slq_quad for one system by `ql_first_row`: (theta, weight, out, flag)"""
    d, w, ok = ql_first_row(al[:m], be[1:m])
    flag = 0 if ok else 2
    if name in NEEDS_POSITIVE and not bool((d > 0).all()):
        flag |= 1
    with np.errstate(all="ignore"):
        out = math.nan if flag else float(zz * (w * fn_of(name, t)[0](d)).sum()) if m else 0.0
    return d, w, out, flag


def quad_truth(al, be, m, zz, name, t=1.0):
    """numpy.linalg.eigh of the same T: (theta, weight, out, bound); bound as in the module docstring"""
    if m == 0:
        return np.zeros(0), np.zeros(0), 0.0, 0.0
    T = jacobi(al, be, m)
    th, U = np.linalg.eigh(T)
    w = U[0] ** 2
    f, df = fn_of(name, t)
    with np.errstate(all="ignore"):
        out = float(zz * (w * f(th)).sum())
        tn = np.abs(T).sum(1).max()
        bound = float(C_Q * m * EPS64 * zz * (w * (np.abs(f(th)) + tn * df(th))).sum())
    return th, w, out, bound


# ------------------------------------------------------------------------------------------------ whole iteration
def forms(A, z, nsteps, arith=np.float64, name="log", t=1.0):
    """z^T f(A) z for one real system by the kernels' iteration chained as the driver chains it: vectors and their
    inner products in `arith`, the scalars in double, the quadrature by `quad`.  Returns (form, m, flag)."""
    A, z = np.asarray(A).astype(arith), np.asarray(z).astype(arith)
    eps = float(np.finfo(arith).eps)
    dot = lambda x, y: float((x * y).sum(dtype=arith))
    zz = dot(z, z)
    beta, oldb, m, tnorm, rowp = math.sqrt(zz), 0.0, 0, 0.0, 0.0
    r2, r1 = z.copy(), np.zeros_like(z)
    al, be = np.zeros(nsteps), np.zeros(nsteps)
    for k in range(nsteps):
        if zz == 0:
            break
        W = A @ r2
        first = m == 0
        if not first:
            oldb, beta = beta, math.sqrt(dot(r2, r2))
            tnorm = max(tnorm, rowp + beta)
            if beta <= BREAK * eps * tnorm:
                break
        alpha = dot(r2, W) / (beta * beta)
        y = W * arith(1.0 / beta) - arith(alpha / beta) * r2
        if not first:
            y = y - arith(beta / oldb) * r1
        r1, r2 = r2, y
        al[m], be[m] = alpha, beta
        rowp = abs(alpha) + (0.0 if first else beta)
        m += 1
    _, _, out, flag = quad(al, be, m, zz, name, t)
    return out, m, flag


def spd_matrix(rng, n, lo=1.0, hi=100.0):
    """A = Q diag(geomspace(lo, hi, n)) Q^T with a random orthogonal Q: (A, Q, eigenvalues)"""
    lam = np.geomspace(lo, hi, n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * lam) @ Q.T
    return (A + A.T) / 2, Q, lam


def rand_state(g, S, k, frozen=(), first=()):
    """(2, S, NST) float64 state: slot k & 1 a plausible mid-iteration state, the other slot NaN-poisoned; `frozen`
    systems carry flag 1, `first` systems the start state xk_slq_init leaves"""
    st = torch.full((2, S, NST), math.nan, dtype=torch.float64)
    r = lambda: 0.5 + torch.rand(S, dtype=torch.float64, generator=g)
    s = st[k & 1]
    s[:, BETA], s[:, OLDB], s[:, FLAG], s[:, M] = r(), r(), 0.0, 3.0
    s[:, TNORM], s[:, ROWP], s[:, ZNORM2], s[:, ALPHA] = 2 * r(), r(), 40 * r(), r()
    for i in first:
        b = s[i, BETA].item()
        s[i] = 0.0
        s[i, BETA], s[i, ZNORM2] = b, b * b
    for i in frozen:
        s[i, FLAG] = 1.0
    return st
