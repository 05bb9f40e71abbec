"""numpy complex128 restatement of the Krylov-Schur Arnoldi pieces: what xk_arn_schur computes from one projected
matrix (steps 1-7 of its header comment) and the driver's cycle.  Written from the algorithm's description with whole-row
and whole-column numpy operations; it shares no code with the kernel.

    small = schur_restart(H, neig, keep, which, real_op)      # H (m + 1, m)
    lam, X, info = arnoldi(matvec, n, neig, which, ncv, v0, real_op)
"""
import numpy as np

EPS = np.finfo(np.float64).eps
FLAG_NONFINITE, FLAG_QR_LIMIT, FLAG_NOT_CLOSED, FLAG_KEEP_MOVED = 1, 2, 4, 8
PAIR_RTOL = 1e-6
CLOSED_TOL = 1e-8


def _abs1(z):
    return abs(z.real) + abs(z.imag)


def _givens(a, b):
    """c real, s complex with [c s; -conj(s) c] (a, b)^T = (r, 0)^T"""
    na, nb = abs(a), abs(b)
    if nb == 0.0:
        return 1.0, 0.0j
    if na == 0.0:
        return 0.0, np.conj(b) / nb
    r = np.hypot(na, nb)
    return na / r, (a / na) * np.conj(b) / r


def hessenberg(T, Z):
    """in place: T <- P T P, Z <- Z P by Householder reflectors; columns already reduced are skipped"""
    m = T.shape[0]
    for k in range(m - 2):
        x = T[k + 1:, k].copy()
        if not np.any(x[1:] != 0):
            continue
        nx = np.linalg.norm(x)
        ph = x[0] / abs(x[0]) if x[0] != 0 else 1.0
        alpha = -ph * nx
        v = x
        v[0] -= alpha
        v = v / np.linalg.norm(v)
        T[k + 1:, k:] -= 2.0 * np.outer(v, v.conj() @ T[k + 1:, k:])
        T[k + 1, k], T[k + 2:, k] = alpha, 0.0
        T[:, k + 1:] -= 2.0 * np.outer(T[:, k + 1:] @ v, v.conj())
        Z[:, k + 1:] -= 2.0 * np.outer(Z[:, k + 1:] @ v, v.conj())


def qr_iteration(T, Z, fro):
    """in place single-shift QR on a Hessenberg T: Wilkinson shift, exceptional shifts at iterations 10 and 20 of a
    block, 30 m iterations in all.  Returns (iterations, failed)."""
    m = T.shape[0]
    ihi, its, total = m - 1, 0, 0
    while ihi >= 1:
        lo = ihi
        while lo >= 1:
            s = _abs1(T[lo - 1, lo - 1]) + _abs1(T[lo, lo])
            if s == 0.0:
                s = fro
            if _abs1(T[lo, lo - 1]) <= EPS * s:
                T[lo, lo - 1] = 0.0
                break
            lo -= 1
        if lo == ihi:
            ihi, its = ihi - 1, 0
            continue
        if total >= 30 * m:
            return total, True
        its, total = its + 1, total + 1
        a, b, c, d = T[ihi - 1, ihi - 1], T[ihi - 1, ihi], T[ihi, ihi - 1], T[ihi, ihi]
        if its in (10, 20):
            mu = d + 0.75 * _abs1(c)
        else:
            delta, bc = 0.5 * (a - d), b * c
            disc = np.sqrt(delta * delta + bc + 0j)
            den = delta + disc if _abs1(delta + disc) >= _abs1(delta - disc) else delta - disc
            mu = d if den == 0 else d - bc / den
        idx = np.arange(lo, ihi + 1)
        T[idx, idx] -= mu
        rots = []
        for k in range(lo, ihi):
            c_, s_ = _givens(T[k, k], T[k + 1, k])
            rk, rk1 = T[k, k:].copy(), T[k + 1, k:].copy()
            T[k, k:] = c_ * rk + s_ * rk1
            T[k + 1, k:] = -np.conj(s_) * rk + c_ * rk1
            T[k + 1, k] = 0.0
            rots.append((k, c_, s_))
        for k, c_, s_ in rots:
            for Mx, top in ((T, k + 2), (Z, m)):
                ck, ck1 = Mx[:top, k].copy(), Mx[:top, k + 1].copy()
                Mx[:top, k] = c_ * ck + np.conj(s_) * ck1
                Mx[:top, k + 1] = -s_ * ck + c_ * ck1
        T[idx, idx] += mu
    return total, False


def rank_key(lam, which):
    return {"LM": np.abs(lam), "LR": lam.real, "SR": -lam.real, "LI": lam.imag, "SI": -lam.imag}[which]


def ranking(lam, which, real_op):
    """(order best first, partner): conjugate partners of a real operator share the larger key and stay adjacent"""
    m = len(lam)
    partner = [-1] * m
    if real_op:
        for i in range(m):
            if partner[i] >= 0 or lam[i].imag == 0.0:
                continue
            cand = [(abs(lam[j] - np.conj(lam[i])), j) for j in range(m)
                    if j != i and partner[j] < 0 and lam[j].imag * lam[i].imag < 0.0]
            if not cand:
                continue
            bd, best = min(cand)
            if bd <= PAIR_RTOL * max(abs(lam[i]), abs(lam[best])):
                partner[i], partner[best] = best, i
    key = rank_key(lam, which)
    skey = [max(key[i], key[partner[i]]) if partner[i] >= 0 else key[i] for i in range(m)]
    lead = [min(i, partner[i]) if partner[i] >= 0 else i for i in range(m)]
    order = sorted(range(m), key=lambda i: (-skey[i], lead[i], -lam[i].imag, i))
    return order, partner


def cut(order, partner, keep, m):
    kp = min(keep, m - 1)
    if partner[order[kp - 1]] == order[kp]:
        kp += 1
    if kp > m - 1:
        kp = m - 1
        if partner[order[kp - 1]] == order[kp]:
            kp -= 1
    return kp


def swap_adjacent(T, Z, k):
    """exchange T[k, k] and T[k+1, k+1] of an upper triangular T by one unitary 2 x 2 similarity"""
    x, y = T[k, k + 1], T[k + 1, k + 1] - T[k, k]
    r = np.hypot(abs(x), abs(y))
    if r > 0.0:
        G = np.array([[x, -np.conj(y)], [y, np.conj(x)]]) / r
        T[k:k + 2, k:] = G.conj().T @ T[k:k + 2, k:]
        T[:k + 2, k:k + 2] = T[:k + 2, k:k + 2] @ G
        Z[:, k:k + 2] = Z[:, k:k + 2] @ G
    T[k + 1, k] = 0.0


def real_basis(Zk, kp):
    """real orthonormal basis of span(Zk) for a conjugation-closed span: column-pivoted Gram-Schmidt on [Re | Im], every
    projection applied twice; returns (Q (m, nq), largest column norm left)"""
    if kp == 0:
        return np.zeros((Zk.shape[0], 0)), 0.0
    S = np.concatenate([Zk.real, Zk.imag], axis=1)
    free = np.ones(S.shape[1], bool)
    cols = []
    left = 0.0
    for c in range(kp + 1):
        n2 = np.where(free, (S * S).sum(axis=0), -1.0)
        p = int(np.argmax(n2))
        if c == kp:
            left = np.sqrt(max(n2[p], 0.0))
            break
        if not n2[p] > 1e-28:
            left = 1.0
            break
        S[:, p] /= np.sqrt(n2[p])
        free[p] = False
        cols.append(p)
        for _ in range(2):
            S[:, free] -= np.outer(S[:, p], S[:, p] @ S[:, free])
    return S[:, cols], left


def schur_restart(H, neig, keep, which, real_op, tol=0.0, u=EPS, keep_add=0):
    """everything xk_arn_schur returns for one member: dict with theta (m,), Y (m, neig), res (neig,), Q (m, keep'),
    Hnext (m + 1, m), nconv, iters, flags, keep, and the Schur factors T, Z (of the unscaled B, after the reordering)"""
    H = np.asarray(H)
    m = H.shape[1]
    B, beta = H[:m].astype(np.complex128), complex(H[m, m - 1])
    out = dict(nconv=0, iters=0, flags=0, keep=0)
    if not (np.all(np.isfinite(B)) and np.isfinite(beta)):
        out["flags"] = FLAG_NONFINITE
        return out
    mx = max(np.abs(B.real).max(), np.abs(B.imag).max())
    ex = int(np.floor(np.log2(mx))) if mx > 0 else 0
    if mx > 0 and not (1.0 <= np.ldexp(mx, -ex) < 2.0):       # (log2 rounds at the powers of two)
        ex += 1 if np.ldexp(mx, -ex) >= 2.0 else -1
    T = np.ldexp(B.real, -ex) + 1j * np.ldexp(B.imag, -ex)
    fro = np.linalg.norm(T)
    Z = np.eye(m, dtype=np.complex128)
    hessenberg(T, Z)
    iters, failed = qr_iteration(T, Z, fro)
    out["iters"] = iters
    if failed:
        out["flags"] = FLAG_QR_LIMIT
        return out
    order, partner = ranking(np.diag(T).copy(), which, real_op)
    kp = min(keep + keep_add, m - 1)
    if real_op:
        kp = cut(order, partner, kp, m)
    flags = FLAG_KEEP_MOVED if kp != keep else 0
    pos = list(np.argsort(order))                   # pos[i]: rank of the eigenvalue now at position i
    for p in range(kp):
        c = pos.index(p)
        for k in range(c - 1, p - 1, -1):
            swap_adjacent(T, Z, k)
            pos[k], pos[k + 1] = pos[k + 1], pos[k]
    theta = np.empty(m, np.complex128)
    theta[pos] = np.ldexp(np.diag(T).real, ex) + 1j * np.ldexp(np.diag(T).imag, ex)
    smin = max(EPS * fro, np.finfo(np.float64).tiny)
    Y = np.zeros((m, neig), np.complex128)
    for i in range(neig):
        x = np.zeros(i + 1, np.complex128)
        x[i] = 1.0
        for r in range(i - 1, -1, -1):
            den = T[r, r] - T[i, i]
            if _abs1(den) < smin:
                den = smin
            x[r] = -(T[r, r + 1:i + 1] @ x[r + 1:]) / den
        y = Z[:, :i + 1] @ x
        Y[:, i] = y / np.linalg.norm(y)
    res = abs(beta) * np.abs(Y[m - 1])
    scale = np.ldexp(1.0, ex)
    nconv = int(np.sum(res <= tol * np.maximum(np.abs(theta[:neig]), u * fro * scale)))
    Hnext = np.zeros((m + 1, m), np.float64 if real_op else np.complex128)
    if real_op:
        Q, left = real_basis(Z[:, :kp], kp)
        if left > CLOSED_TOL or Q.shape[1] < kp:
            flags |= FLAG_NOT_CLOSED
        nq = Q.shape[1]
        Hnext[:nq, :nq] = Q.T @ (H[:m].real @ Q)
        Hnext[kp, :nq] = beta.real * Q[m - 1]
    else:
        Q = Z[:, :kp].copy()
        Hnext[:kp, :kp] = np.triu(T[:kp, :kp]) * scale
        Hnext[kp, :kp] = beta * Q[m - 1]
    out.update(theta=theta, Y=Y, res=res, Q=Q, Hnext=Hnext, nconv=nconv, flags=flags, keep=kp, T=T * scale, Z=Z)
    return out


def arnoldi(matvec, n, neig, which, ncv, v0, real_op, min_eps=1e-6, max_niter=100, u=EPS):
    """the driver's cycle for one member: CGS2 Arnoldi steps, schur_restart at j = ncv, restart on keep' vectors.
    Returns (lam (neig,), X (n, neig) unit columns, dict(niter, converged, resid))."""
    dt = np.float64 if real_op else np.complex128
    m = ncv
    V = np.zeros((n, m + 1), dt)
    H = np.zeros((m + 1, m), dt)
    V[:, 0] = v0 / np.linalg.norm(v0)
    start, hmax = 0, 0.0
    rng = np.random.default_rng(12421)
    for cycle in range(max_niter):
        for j in range(start, m):
            w = matvec(V[:, j])
            c1 = V[:, :j + 1].conj().T @ w
            w = w - V[:, :j + 1] @ c1
            c2 = V[:, :j + 1].conj().T @ w
            w = w - V[:, :j + 1] @ c2
            H[:j + 1, j] = c1 + c2
            nrm = np.linalg.norm(w)
            if not nrm > u * hmax:                   # breakdown: a random direction orthogonal to the basis
                nrm = 0.0
                w = rng.standard_normal(n).astype(dt)
                for _ in range(2):
                    w = w - V[:, :j + 1] @ (V[:, :j + 1].conj().T @ w)
                w /= np.linalg.norm(w)
            else:
                w = w / nrm
            hmax = max(hmax, nrm)
            H[j + 1, j] = nrm
            V[:, j + 1] = w
        small = schur_restart(H, neig, neig + (m - neig) // 2, which, real_op, tol=min_eps, u=u)
        if small["flags"] & (FLAG_NONFINITE | FLAG_QR_LIMIT):
            raise RuntimeError("arn_ref: the small problem failed with flags %d" % small["flags"])
        if small["nconv"] >= neig or cycle + 1 == max_niter:
            break
        kp = small["Q"].shape[1]
        Vn = np.zeros_like(V)
        Vn[:, :kp] = V[:, :m] @ small["Q"]
        Vn[:, kp] = V[:, m]
        V, H, start = Vn, small["Hnext"].copy(), kp
    X = V[:, :m] @ small["Y"]
    X = X / np.linalg.norm(X, axis=0)
    lam = small["theta"][:neig]
    AX = np.stack([matvec(X[:, i].real) + 1j * matvec(X[:, i].imag) if real_op else matvec(X[:, i])
                   for i in range(neig)], axis=1)
    resid = np.linalg.norm(AX - X * lam, axis=0)
    return lam, X, dict(niter=cycle + 1, converged=small["nconv"] >= neig, resid=resid)
