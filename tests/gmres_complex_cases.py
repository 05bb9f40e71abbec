"""Cases, residual rule and textbook reference shared by tests/test_host_gmres_complex.py (host memory) and
tests/test_gpu_gmres_complex.py (the same cases on the device).

The textbook: GMRES without restarts, with modified Gram-Schmidt Arnoldi and Givens rotations, as in Saad & Schultz
(1986) and Saad, "Iterative Methods for Sparse Linear Systems", Alg. 6.9 + section 6.5.3, written here in complex128
numpy from the literature.  The literature's complex rotation is c = |a| / r, s = (a / |a|) conj(b) / r with
r = sqrt(|a|^2 + |b|^2); here b = h[k+1,k] is a norm, hence real, and conj(b) = b.  It
returns the residual norms |g[k+1]| after every step; the drivers' `arnoldi_steps` must equal the first step whose
residual is below the threshold, on cases where that residual and the one before it are each a factor 2 away from it.
"""
import numpy as np
import torch
import xitorch_amd as xa

U128 = 2.0 ** -53
RTOL = {torch.complex128: 1e-9, torch.complex64: 1e-4}
ATOL = {torch.complex128: 1e-14, torch.complex64: 1e-8}


class MvOperator(xa.LinearOperator):
    """a generic operator: only `_mv` (and the adjoint's) — served through `.mm` on the strided view"""

    def __init__(self, mat):
        super().__init__(shape=tuple(mat.shape), is_hermitian=False, dtype=mat.dtype, device=mat.device)
        self.mat = mat

    def _mv(self, x):
        return torch.matmul(self.mat, x.unsqueeze(-1)).squeeze(-1)

    def _rmv(self, x):
        return torch.matmul(self.mat.transpose(-2, -1).conj(), x.unsqueeze(-1)).squeeze(-1)

    def _getparamnames(self, prefix=""):
        return [prefix + "mat"]


def _crand(g, *shape):
    return torch.complex(torch.randn(shape, dtype=torch.float64, generator=g),
                         torch.randn(shape, dtype=torch.float64, generator=g))


def make(case):
    """-> dict(A (dense complex128 tensor, batch dims allowed), B, E, M, kind, dtype, kw) in host memory, in complex128
    rounded to the case dtype (so that every precision sees the same numbers)"""
    g = torch.Generator().manual_seed(case["seed"])
    n, dt = case["n"], case["dtype"]
    ab, bb = case.get("abatch", ()), case.get("bbatch", ())
    A = case.get("scale", 0.5) * _crand(g, *ab, n, n) / np.sqrt(n) + \
        torch.diag_embed((1.0 + 0.3j) * torch.ones(n, dtype=torch.complex128))
    if case["kind"] == "csr":
        keep = torch.rand(n, n, generator=g) < case.get("density", 0.2)
        keep |= torch.eye(n, dtype=torch.bool)
        A = A * keep
    B = _crand(g, *bb, n, case.get("ncols", 1))
    E = M = None
    if case.get("E"):
        E = 0.2 * _crand(g, *bb, case.get("ncols", 1))
        if case.get("M"):
            R = _crand(g, n, n) / np.sqrt(n)
            M = torch.eye(n, dtype=torch.complex128) + 0.1 * (R + R.conj().T)
    rnd = lambda t: None if t is None else t.to(dt).to(torch.complex128)
    return dict(A=rnd(A), B=rnd(B), E=rnd(E), M=rnd(M))


def operators(case, data, device):
    dt = case["dtype"]
    A = data["A"].to(dt).to(device)
    if case["kind"] == "dense":
        Aop = xa.LinearOperator.m(A, is_hermitian=False)
    elif case["kind"] == "csr":
        t = A.cpu().to_sparse_csr()
        Aop = xa.SparseLinearOperator(t.crow_indices().to(device), t.col_indices().to(device), t.values().to(device),
                                      tuple(A.shape), is_hermitian=False)
    else:
        Aop = MvOperator(A)
    Mop = None if data["M"] is None else xa.LinearOperator.m(data["M"].to(dt).to(device), is_hermitian=True)
    B = data["B"].to(dt).to(device)
    E = None if data["E"] is None else data["E"].to(dt).to(device)
    return Aop, B, E, Mop


def residual_rule(case, data, X, rtol, atol):
    """the method's own rule on the returned X, recomputed in complex128 on the CPU:
    |b - (A x - M x E)| <= max(rtol |b|, atol) + slack per column.

    slack = gamma u (|A|_1 |x|_1 + |b|), u = 2^-53: a component of (A x)_i is a sum of 2 n real products (n complex
    products of 2 real terms each): product (1), the additions inside and between the products (2 n), the subtraction
    from b (1); with a shift the same again for M x, a complex product with E (2) and one more addition:
    gamma = 2 n + 2, or 4 n + 7 with E and M (2 n + 5 with E alone).  The column norm adds n more additions of squares,
    relative to the norm: covered by the + |b| term with gamma >= n."""
    A, B, E, M = data["A"], data["B"], data["E"], data["M"]
    n = A.shape[-1]
    Xh = X.detach().cpu().to(torch.complex128)
    AX = A @ Xh
    gamma = 2 * n + 2
    if E is not None:
        MX = Xh if M is None else M @ Xh
        AX = AX - MX * E.unsqueeze(-2)
        gamma = (4 * n + 7) if M is not None else (2 * n + 5)
    Bx = B.expand(*AX.shape)
    r = torch.linalg.vector_norm(Bx - AX, dim=-2)
    bn = torch.linalg.vector_norm(Bx, dim=-2)
    a1 = A.abs().sum(-2).max(-1)[0]                              # |A|_1 (per batch member)
    if E is not None:
        m1 = 1.0 if M is None else M.abs().sum(-2).max().item()
        a1 = a1.unsqueeze(-1) + m1 * E.abs()
    else:
        a1 = a1.unsqueeze(-1)
    x1 = Xh.abs().sum(-2)
    slack = gamma * U128 * (a1 * x1 + bn)
    lim = torch.maximum(rtol * bn, torch.full_like(bn, atol)) + slack
    return r, lim


def textbook_gmres(Amat, b, stop, maxit):
    """MGS-GMRES from x0 = 0 on one system (complex128 numpy).  Returns the residual norms rho[k] = |g[k+1]| after k + 1
    Arnoldi steps, k = 0 .. (until rho < stop / 4 or a breakdown or maxit)."""
    n = b.shape[0]
    beta = np.linalg.norm(b)
    V = [b / beta]
    H = np.zeros((maxit + 1, maxit), dtype=np.complex128)
    cs, sn = np.zeros(maxit), np.zeros(maxit, dtype=np.complex128)
    g = np.zeros(maxit + 1, dtype=np.complex128)
    g[0] = beta
    rho = []
    for k in range(maxit):
        w = Amat @ V[k]
        for i in range(k + 1):
            H[i, k] = np.vdot(V[i], w)
            w = w - H[i, k] * V[i]
        H[k + 1, k] = np.linalg.norm(w)
        for i in range(k):                                        # previous rotations on the new column
            t = cs[i] * H[i, k] + sn[i] * H[i + 1, k]
            H[i + 1, k] = -np.conj(sn[i]) * H[i, k] + cs[i] * H[i + 1, k]
            H[i, k] = t
        a, bb = H[k, k], H[k + 1, k].real
        r = np.sqrt(abs(a) ** 2 + bb ** 2)
        if abs(a) == 0:
            cs[k], sn[k] = 0.0, 1.0
        else:
            cs[k], sn[k] = abs(a) / r, (a / abs(a)) * bb / r
        H[k, k] = cs[k] * a + sn[k] * bb
        H[k + 1, k] = 0
        g[k + 1] = -np.conj(sn[k]) * g[k]
        g[k] = cs[k] * g[k]
        rho.append(abs(g[k + 1]))
        if rho[-1] < stop / 4 or bb == 0:
            break
        V.append(w / bb)
    return rho


def textbook_steps(case, data, rtol, atol):
    """-> (steps, ok): the lock-step count of Arnoldi steps after which EVERY system is below its threshold, and
    whether the factor-2 condition holds: at that step every system's residual <= stop / 2, and at the step before at
    least one system's residual >= 2 stop."""
    A, B, E, M = (None if t is None else t.numpy() for t in (data["A"], data["B"], data["E"], data["M"]))
    n = A.shape[-1]
    bshape = np.broadcast_shapes(A.shape[:-2], B.shape[:-2], () if E is None else E.shape[:-1])
    Ab = np.broadcast_to(A, (*bshape, n, n)).reshape(-1, n, n)
    Bb = np.broadcast_to(B, (*bshape, n, B.shape[-1])).reshape(-1, n, B.shape[-1])
    Eb = None if E is None else np.broadcast_to(E, (*bshape, B.shape[-1])).reshape(-1, B.shape[-1])
    hist = []
    for s in range(Ab.shape[0]):
        for c in range(Bb.shape[-1]):
            Amat = Ab[s]
            if Eb is not None:
                Amat = Amat - Eb[s, c] * (np.eye(n) if M is None else M)
            b = Bb[s, :, c]
            stop = max(rtol * np.linalg.norm(b), atol)
            hist.append((textbook_gmres(Amat, b, stop, n - 1), stop))
    first = [next((k for k, r in enumerate(rho) if r < stop), None) for rho, stop in hist]
    if any(f is None for f in first):
        return None, False
    kstar = max(first)
    at = lambda rho, k: rho[min(k, len(rho) - 1)]
    ok = all(at(rho, kstar) <= stop / 2 for rho, stop in hist) and \
        (kstar == 0 or any(at(rho, kstar - 1) >= 2 * stop and len(rho) > kstar - 1 for rho, stop in hist))
    return kstar + 1, ok


C128, C64 = torch.complex128, torch.complex64
# the cases of the residual rule (all of them) — operator kinds, E / M, batch dims with broadcasting, both dtypes
RULE_CASES = [
    dict(name="dense_c128", kind="dense", dtype=C128, n=48, seed=1),
    dict(name="dense_c64", kind="dense", dtype=C64, n=48, seed=2),
    dict(name="csr_c128", kind="csr", dtype=C128, n=60, seed=3),
    dict(name="csr_c64", kind="csr", dtype=C64, n=60, seed=4),
    dict(name="mv_c128", kind="mv", dtype=C128, n=40, seed=5),
    dict(name="mv_c64", kind="mv", dtype=C64, n=40, seed=6),
    dict(name="dense_E_c128", kind="dense", dtype=C128, n=48, seed=7, E=True, ncols=3),
    dict(name="dense_EM_c128", kind="dense", dtype=C128, n=48, seed=8, E=True, M=True, ncols=2),
    dict(name="dense_EM_c64", kind="dense", dtype=C64, n=48, seed=9, E=True, M=True, ncols=2),
    dict(name="csr_E_c128", kind="csr", dtype=C128, n=60, seed=10, E=True, ncols=2),
    dict(name="batch_c128", kind="dense", dtype=C128, n=33, seed=11, abatch=(2, 1), bbatch=(3,), ncols=2),
    dict(name="batch_E_c64", kind="dense", dtype=C64, n=33, seed=12, abatch=(2,), bbatch=(1,), ncols=2, E=True),
    dict(name="mv_batch_c128", kind="mv", dtype=C128, n=31, seed=13, abatch=(2,), bbatch=(2,), ncols=1),
]
# The step-count comparison: one system each, fast convergence (a small random part), and a threshold rtol placed at
# the geometric mean of two consecutive textbook residuals that are more than a factor 4 apart — so the residual at the
# crossing step is below stop / 2 and the one before above 2 stop (test_step_cases_meet_the_factor_2 verifies this).
# Dropped for missing the factor 2 (ratio 3.88 at every usable step): dense, complex128, n = 200, scale 0.2, seed 41.
STEP_ATOL = 1e-30
STEP_CASES = [
    dict(name="s_dense_c128", kind="dense", dtype=C128, n=48, seed=31, scale=0.15, rtol=3.72e-06, steps=8),
    dict(name="s_dense_c64", kind="dense", dtype=C64, n=48, seed=32, scale=0.15, rtol=6.53e-04, steps=5),
    dict(name="s_csr_c128", kind="csr", dtype=C128, n=60, seed=33, scale=0.3, rtol=6.57e-07, steps=9),
    dict(name="s_csr_c64", kind="csr", dtype=C64, n=60, seed=34, scale=0.3, rtol=3.65e-04, steps=5),
    dict(name="s_mv_c128", kind="mv", dtype=C128, n=40, seed=35, scale=0.15, rtol=2.83e-05, steps=7),
    dict(name="s_mv_c64", kind="mv", dtype=C64, n=40, seed=36, scale=0.15, rtol=3.28e-03, steps=4),
    dict(name="s_dense_E_c128", kind="dense", dtype=C128, n=48, seed=37, scale=0.15, E=True, rtol=1.24e-05, steps=7),
    dict(name="s_dense_EM_c128", kind="dense", dtype=C128, n=48, seed=38, scale=0.15, E=True, M=True, rtol=1.83e-05,
         steps=7),
    dict(name="s_dense_EM_c64", kind="dense", dtype=C64, n=48, seed=39, scale=0.15, E=True, M=True, rtol=2.33e-03,
         steps=4),
    dict(name="s_csr_E_c128", kind="csr", dtype=C128, n=60, seed=40, scale=0.3, E=True, rtol=1.04e-07, steps=8),
    dict(name="s_csr_big_c64", kind="csr", dtype=C64, n=300, seed=42, scale=0.4, density=0.05, rtol=7.38e-05, steps=5),
]
