"""Complex128 restatement of the Hermitian Davidson kernels (xk_herm_davidson.hip: xk_herm_ritz, xk_herm_cholqr,
xk_herm_eigh) and of kernels.dense_outer_complex, with error bounds.

Same shape as tests/davidson_ref.py: for every kernel a function computes, from the very inputs the kernel is given
(read back in the kernel dtype, widened to complex128 / float64), what the kernel must write, as
{name: (value, bound)}.  `bound` is a real tensor: a per-entry absolute bound that holds for the real AND the imaginary
part of |kernel - value| separately.  `check()` compares, `WORST` keeps the worst |kernel - value| / bound per
(dtype, kernel), `fault=` produces the plausible kernel bugs of `FAULTS`, which tests/test_herm_ref.py shows rejected.

Bounds: C_TOL * u * n * sum|terms| with davidson_ref's C_TOL (its comment gives the derivation).  u is the unit
roundoff of the REAL element type.  The complex count: cfma (xk_herm_davidson.hip) is two real FMAs per component, so
a sum of k complex products accumulated in one register pair goes through n = 2k sequential roundings per component,
and |Re(a b)|, |Im(a b)| <= |a| |b|, so sum|terms| is the sum of the products of the moduli.
"""
import functools
import math
import torch
from tests import davidson_ref as dref
from tests import solver_ref as sref

C_TOL = dref.C_TOL
KAPPA2_MAX = dref.KAPPA2_MAX
c128, c64 = torch.complex128, torch.complex64
REAL = {c128: torch.float64, c64: torch.float32}
DNAME = {c128: "c128", c64: "c64"}
RITZ_PC = 16          # columns of Y per launch of herm_ritz_kernel
CHOL_CH = 32          # vector elements per LDS chunk of herm_gram_chol_kernel
GRAM_WRAP = 256       # Gram entries are dealt to the 256 threads as tid + 256 e

FAULTS = (
    # xk_herm_ritz
    "chunk_y", "chunk_lam", "chunk_out",        # second column chunk (c0 = 16) without its offset in Y / lam / output row
    "y_transposed",                             # Y[c, a] read where Y[a, c] is meant
    "lam_x",                                    # lam * X where lam * (Y^T MV) is meant
    "tn_sign",                                  # Tn = +R
    "conj_y",                                   # conj(Y) used
    "drop_last_block",                          # the last partial block of 256 elements of N neither computed nor written
    "status_nan_dropped",                       # a floating-point max: NaN residuals vanish from status
    "status_wrong_member",                      # per-member maximum written to the next member's slot
    # xk_herm_cholqr
    "mw_not_transformed",                       # apply: MW left as it was
    "rinv_transposed",                          # apply: Rinv[c, a] read for Rinv[a, c]
    "gram_no_conj",                             # G = W^T MW
    "no_shift",                                 # shift_rel ignored
    "gram_drop_256", "gram_drop_512",           # Gram entries with index >= 256 / >= 512 never summed
    "drop_tail_chunk",                          # the N % 32 tail chunk left out of the Gram sums
    # xk_herm_eigh
    "upper_read",                               # the upper triangle read
    "imag_diag_used",                           # the imaginary part of the diagonal taken into the matrix
    "uppest_lowest",                            # uppest = 1 returns the lowest block
    "y_conj",                                   # eigenvectors returned conjugated
    # dense_outer_complex
    "outer_no_conj",                            # G = sum U W (W not conjugated)
)

# worst |kernel - reference| / bound (or measured / tolerance for xk_herm_eigh) per (dtype name, kernel)
WORST = {}


def unit_roundoff(dtype):
    return torch.finfo(REAL.get(dtype, dtype)).eps / 2


def _cu(dtype):
    return C_TOL * unit_roundoff(dtype)


def hp(t):
    """complex128 (float64 for real tensors) copy on the CPU"""
    t = t.detach().cpu()
    return t.to(c128) if t.is_complex() else t.to(torch.float64)


def rnd(t, dtype):
    """what the kernel reads: rounded to its dtype (complex dtype for complex data, its real type for real data),
    widened again"""
    if t.is_complex():
        return t.to(dtype).to(c128)
    return t.to(REAL[dtype]).to(torch.float64)


def cast(x, dtype):
    """a double argument as the C entry point sees it after `(T)x`, T the real element type"""
    return dref.cast(x, REAL[dtype])


def gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k) + 12345) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def crand(g, *shape):
    return torch.complex(torch.randn(shape, dtype=torch.float64, generator=g),
                         torch.randn(shape, dtype=torch.float64, generator=g))


def _csum(spec, A, Bm):
    """sum of complex products by real contractions (the kernel's own formulas: an Inf or NaN operand propagates as it
    does in cfma, which a library complex product does not promise)"""
    ar, ai, br, bi = A.real, A.imag, Bm.real, Bm.imag
    e = lambda x, y: torch.einsum(spec, x, y)
    return torch.complex(e(ar, br) - e(ai, bi), e(ar, bi) + e(ai, br))


def _cscale(l, Z):
    """real l times complex Z, component-wise (as the kernel does it)"""
    return torch.complex(l * Z.real, l * Z.imag)


# ------------------------------------------------------------------------------------------------ xk_herm_ritz
def ritz(V, AV, MV, Y, lam, dtype, prev=None, fault=None):
    """xk_herm_ritz: X[c] = sum_a Y[a,c] V[a];  R[c] = sum_a Y[a,c] AV[a] - lam_c (sum_a Y[a,c] MV[a]) (MV absent: the
    kernel reuses X[c], the same sum);  Tn = -R;  status[1+b] = max_{n,c} |R| (modulus), status[0] = max_b; a NaN
    in R of member b gives NaN there and in status[0], else an Inf gives Inf.
    V, AV, MV (B, k, N), Y (B, k, p) indexed [b, a, c], lam (B, p).
    Counts per component: X: k cfma = 2k roundings.  Tn: two such sums (2k each, side by side, not in sequence), the
    product lam * m and the difference: 2k + 2.  status: the modulus of an entry whose components are each within
    the Tn bound is within sqrt(2) of it, plus the modulus' own rounding in the kernel's real type (two squares,
    their sum, the square root: 3 roundings after FMA contraction, taken as n = 4)."""
    B, k, p = Y.shape
    N = V.shape[-1]
    Yu, lamu = Y, lam
    idx = torch.arange(p)
    wrapped = torch.where(idx >= RITZ_PC, idx % RITZ_PC, idx)
    if fault == "chunk_y":
        Yu = Y[:, :, wrapped]
    if fault == "chunk_lam":
        lamu = lam[:, wrapped]
    if fault == "y_transposed":
        m = min(k, p)                                   # the leading square block read with its indices exchanged
        Yu = Y.clone()
        Yu[:, :m, :m] = Y[:, :m, :m].transpose(1, 2)
    if fault == "conj_y":
        Yu = Y.conj().resolve_conj()
    spec = "bac,ban->bcn"
    X = _csum(spec, Yu, V)
    AX = _csum(spec, Yu, AV)
    MX = X if (MV is None or fault == "lam_x") else _csum(spec, Yu, MV)
    R = AX - _cscale(lamu.unsqueeze(-1), MX)
    Tn = R if fault == "tn_sign" else -R
    Ya = Y.abs()
    e = lambda x, y: torch.einsum(spec, x, y)
    sv, sav = e(Ya, V.abs()), e(Ya, AV.abs())
    smv = sv if MV is None else e(Ya, MV.abs())
    cu = _cu(dtype)
    bx = cu * (2 * k) * sv
    bt = cu * (2 * k + 2) * (sav + lam.abs().unsqueeze(-1) * smv)
    live = torch.ones(N, dtype=torch.bool)
    if fault == "drop_last_block":
        live[N // 256 * 256:] = False
    if fault == "chunk_out" and p > RITZ_PC:
        X, Tn = X.clone(), Tn.clone()
        for t, t0 in ((X, prev["X"] if prev else None), (Tn, prev["Tn"] if prev else None)):
            t[:, wrapped[RITZ_PC:]] = t[:, RITZ_PC:].clone()
            t[:, RITZ_PC:] = t0[:, RITZ_PC:] if t0 is not None else 0
    if not bool(live.all()):
        X, Tn = X.clone(), Tn.clone()
        X[..., ~live] = prev["X"][..., ~live] if prev else 0
        Tn[..., ~live] = prev["Tn"][..., ~live] if prev else 0
    Ra = torch.sqrt(R.real ** 2 + R.imag ** 2)[..., live].flatten(1)
    if Ra.shape[1] == 0:
        Ra = torch.zeros(B, 1, dtype=torch.float64)
    nanrow = torch.isnan(Ra).any(1)
    clean = torch.where(torch.isnan(Ra), torch.zeros_like(Ra), Ra).max(1).values
    rmax = clean if fault == "status_nan_dropped" else torch.where(nanrow, torch.full_like(clean, math.nan), clean)
    if fault == "status_wrong_member":
        rmax = rmax.roll(1)
    top = torch.full((1,), math.nan, dtype=torch.float64) if bool(torch.isnan(rmax).any()) else rmax.max().view(1)
    status = torch.cat([top, rmax])
    fin = torch.where(torch.isfinite(Ra), Ra, torch.zeros_like(Ra)).max(1).values
    brm = math.sqrt(2.0) * bt.flatten(1).max(1).values + cu * 4 * fin
    brm = torch.where(torch.isfinite(brm), brm, torch.zeros_like(brm))
    bstat = torch.cat([brm.max().view(1), brm])
    return {"X": (X, bx), "Tn": (Tn, bt), "status": (status, bstat)}


def status_consistent(st):
    """status[0] == max(status[1:]) exactly, a NaN member making status[0] NaN"""
    st = st.detach().cpu().double()
    if bool(torch.isnan(st[1:]).any()):
        return bool(torch.isnan(st[0]))
    return st[0].item() == st[1:].max().item()


# ------------------------------------------------------------------------------------------------ xk_herm_cholqr
def cholqr_apply(W, MW, Rinv, dtype, fault=None):
    """herm_cholqr_apply_kernel, given the kernel's own Rinv: W_out[c] = sum_{a<=c} Rinv[a,c] W_in[a] (and the same
    for MW).  W, MW (B, q, N) before the call, Rinv (B, q, q).  c + 1 cfma in one register pair: n = 2 (c + 1).
    Exact bookkeeping: holds whatever the conditioning."""
    q = W.shape[1]
    Ru = torch.triu(Rinv.transpose(1, 2) if fault == "rinv_transposed" else Rinv)
    n = 2 * (torch.arange(q, dtype=torch.float64).view(1, q, 1) + 1)
    out = {}
    for name, P in (("W", W), ("MW", MW)):
        if P is None:
            continue
        val = P if (name == "MW" and fault == "mw_not_transformed") else _csum("bac,ban->bcn", Ru, P)
        mag = torch.einsum("bac,ban->bcn", torch.triu(Rinv).abs(), P.abs())
        out[name] = (val, _cu(dtype) * n * mag)
    return out


def _gram_entry_index(q):
    """index of the upper-triangle entry (i, j), j >= i, in the kernel's dealing order (row i holds q - i entries)"""
    idx = torch.full((q, q), -1, dtype=torch.long)
    n = 0
    for i in range(q):
        for j in range(i, q):
            idx[i, j] = n
            n += 1
    return idx


def herm_chol(G):
    """the kernel's right-looking Cholesky of the upper triangle of (B, q, q) G, G = R^H R: only the real part of a
    pivot is read, a pivot that is not > 0 sets bad = index + 1 (first one) and is taken as 1.  Returns R, bad."""
    B, q = G.shape[0], G.shape[1]
    A = G.clone()
    R = torch.zeros_like(G)
    bad = torch.zeros(B, dtype=torch.long)
    for j in range(q):
        d = A[:, j, j].real.clone()
        nb = ~(d > 0)
        bad = torch.where(nb & (bad == 0), torch.full_like(bad, j + 1), bad)
        d = torch.where(nb, torch.ones_like(d), d)
        rjj = d.sqrt()
        R[:, j, j] = rjj.to(G.dtype)
        if j + 1 < q:
            R[:, j, j + 1:] = A[:, j, j + 1:] / rjj.unsqueeze(-1)
            row = R[:, j, j + 1:]
            A[:, j + 1:, j + 1:] -= row.conj().unsqueeze(-1) * row.unsqueeze(-2)
    return R, bad


def cholqr_gram(W, MW, shift_rel, dtype, fault=None):
    """The matrix herm_gram_chol_kernel factors: G[i][j] = sum_n conj(W[i,n]) MW[j,n] for j >= i (MW absent: W), the
    lower triangle its conjugate mirror, the diagonal real (only .re is read), plus shift_rel * trace(G) on the
    diagonal when shift_rel > 0 (shift_rel as the kernel sees it: `cast`)."""
    q, N = W.shape[1], W.shape[2]
    Mw = W if MW is None else MW
    Wu = W
    if fault == "drop_tail_chunk":
        Wu = W[..., :N // CHOL_CH * CHOL_CH]
        Mw = Mw[..., :N // CHOL_CH * CHOL_CH]
    G = _csum("bin,bjn->bij", Wu if fault == "gram_no_conj" else Wu.conj().resolve_conj(), Mw)
    for f, lim in (("gram_drop_256", GRAM_WRAP), ("gram_drop_512", 2 * GRAM_WRAP)):
        if fault == f:
            G = torch.where((_gram_entry_index(q) >= lim).unsqueeze(0), torch.zeros_like(G), G)
    up = torch.triu(G, 1)
    d = torch.diagonal(G, dim1=1, dim2=2).real
    if shift_rel > 0 and fault != "no_shift":
        d = d + shift_rel * d.sum(-1, keepdim=True)
    return up + up.transpose(1, 2).conj() + torch.diag_embed(d).to(c128)


def kappa2(G):
    ev = torch.linalg.eigvalsh(G)
    lo = ev[:, 0]
    return torch.where(lo > 0, ev[:, -1] / lo.clamp(min=1e-300), torch.full_like(lo, math.inf))


def orth_bound(dtype, N, q, k2):
    """CholeskyQR's loss of orthogonality, |Rinv^H G Rinv - I| per entry: C_TOL u (2N + q) kappa_2(G) (the form of
    davidson_ref.orth / orth_properties; 2N roundings per component of a Gram entry, q for the factorisation)"""
    return _cu(dtype) * (2 * N + q) * k2


def cholqr_factor(W, MW, shift_rel, dtype, fault=None):
    """Gram + Cholesky half: Rinv = inv(R), G = R^H R.  Returns {"Rinv": (value, bound), "_meta": {G, kappa2, info}}.
    The entry bound is the first-order perturbation of the inverse factor, |d Rinv| <= kappa_2(G) eps |Rinv|_2 with
    eps = C_TOL u (2N + q) the relative size of the Gram and factorisation roundings: orth_bound(...) * |Rinv|_2 for
    every entry on or above the diagonal, 0 below (exact zeros).  Meaningful for kappa_2(G) <= KAPPA2_MAX only; the
    caller asserts that."""
    q, N = W.shape[1], W.shape[2]
    G = cholqr_gram(W, MW, shift_rel, dtype)
    k2 = kappa2(G)
    Rinv = torch.triu(torch.linalg.inv(torch.linalg.cholesky(G).transpose(1, 2).conj()))
    bad = torch.zeros(W.shape[0], dtype=torch.long)
    nrm = torch.linalg.matrix_norm(Rinv, ord=2).view(-1, 1, 1)
    if fault is not None:                               # what the kernel's own steps make of the faulty Gram matrix
        R, bad = herm_chol(cholqr_gram(W, MW, shift_rel, dtype, fault=fault))
        ok = bool(torch.isfinite(torch.view_as_real(R)).all())
        Rinv = torch.triu(torch.linalg.inv(R)) if ok else torch.full_like(R, math.nan)
    bnd = torch.triu(torch.ones(q, q, dtype=torch.float64)) * (orth_bound(dtype, N, q, k2).view(-1, 1, 1) * nrm)
    return {"Rinv": (Rinv, bnd), "_meta": {"G": G, "kappa2": k2, "info": bad}}


def cholesky_must_succeed(G, N, dtype):
    """per member: orth_bound < 1.  Cholesky in floating point is only guaranteed to run to completion when
    c n u kappa_2(G) < 1 (Higham, Accuracy and Stability, Theorem 10.7); this is that condition with the constants of
    orth_bound.  Beyond it a non-positive pivot (info != 0) is a legitimate outcome and the orthogonality bound, being
    >= 1, says nothing."""
    return orth_bound(dtype, N, G.shape[1], kappa2(G)) < 1.0


def cholqr_properties(Rinv, G, N, dtype, what="", kernel="herm_cholqr:orth", members=None):
    """What must hold for every block, whatever its conditioning: Rinv upper triangular with EXACT zeros below the
    diagonal, a diagonal with imaginary part exactly 0 and a positive real part (the code writes these without
    rounding), and |Rinv^H G Rinv - I| <= orth_bound per entry (for the members of the boolean mask `members`, all by
    default).  Returns the worst ratio of the last."""
    Rinv = hp(Rinv)
    q = Rinv.shape[1]
    low = torch.tril(torch.ones(q, q, dtype=torch.bool), -1)
    assert bool((Rinv[:, low].real == 0).all() and (Rinv[:, low].imag == 0).all()), what + ": Rinv below the diagonal"
    dg = torch.diagonal(Rinv, dim1=1, dim2=2)
    assert bool((dg.imag == 0).all()), what + ": imaginary diagonal of Rinv"
    assert bool((dg.real > 0).all()), what + ": diagonal of Rinv not positive"
    E = torch.matmul(Rinv.transpose(1, 2).conj(), torch.matmul(G, Rinv)) - torch.eye(q, dtype=c128)
    err = torch.maximum(E.real.abs(), E.imag.abs()).flatten(1).max(1).values
    bnd = orth_bound(dtype, N, q, kappa2(G))
    if members is not None:                             # (members whose factorisation legitimately broke down: structure only)
        err, bnd = err[members], bnd[members]
        if err.numel() == 0:
            return 0.0
    ratio = float((err / bnd).max())
    assert ratio <= 1.0, "%s: |Rinv^H G Rinv - I| %s > bound %s" % (what, err.tolist(), bnd.tolist())
    _record(dtype, kernel, ratio)
    return ratio


# ------------------------------------------------------------------------------------------------ xk_herm_eigh
EIGH_TOL = {  # the project's tolerances: test_rr_kernel_vs_eigh (lam, res, orth), the K3t test (projector, gap)
    c128: {"lam": 1e-12, "res": 1e-12, "orth": 1e-12, "proj": 1e-8},
    c64: {"lam": 1e-5, "res": 2e-5, "orth": 5e-5, "proj": 1e-2},
}
EIGH_GAP = 1e-6


def contracted(T):
    """the matrix xk_herm_eigh is contracted to see in T (.., n, n): lower triangle as stored, its conjugate mirror
    above, the real part of the diagonal"""
    lo = torch.tril(T, -1)
    d = torch.diagonal(T, dim1=-2, dim2=-1).real
    return lo + lo.transpose(-2, -1).conj() + torch.diag_embed(d).to(T.dtype)


def eigh_model(T, p, uppest, fault=None):
    """(lam (B, p), Y (B, p, n)) a kernel with `fault` would return for the stored T (B, n, n): complex128 library
    eigendecomposition of the matrix that kernel sees"""
    n = T.shape[-1]
    if fault == "upper_read":
        A = contracted(T.transpose(-2, -1).conj())
    elif fault == "imag_diag_used":
        A = contracted(T) + torch.diag_embed(torch.complex(torch.zeros(T.shape[:-1], dtype=torch.float64),
                                                           torch.diagonal(T, dim1=-2, dim2=-1).imag))
    else:
        A = contracted(T)
    if fault == "imag_diag_used":                      # no longer Hermitian: the general decomposition, real parts sorted
        w, Z = torch.linalg.eig(A)
        order = torch.argsort(w.real, dim=-1)
        lam = torch.gather(w.real, -1, order)
        Z = torch.gather(Z, -1, order.unsqueeze(-2).expand_as(Z))
        Z = Z / torch.linalg.vector_norm(Z, dim=-2, keepdim=True)
    else:
        lam, Z = torch.linalg.eigh(A)
    sl = slice(n - p, n) if (uppest and fault != "uppest_lowest") else slice(0, p)
    Y = Z[..., sl].transpose(-2, -1)
    if fault == "y_conj":
        Y = Y.conj().resolve_conj()
    return lam[..., sl], Y.contiguous()


def eigh_check(T, lam, Y, p, uppest, dtype, what=""):
    """lam (B, p), Y (B, p, n) of xk_herm_eigh against torch.linalg.eigh of contracted(T) in complex128: eigenvalues,
    ascending order, residual, orthonormality and, per member whose wanted block is separated from the rest by more
    than EIGH_GAP |T|, equality of the spectral projectors.  Raises AssertionError; records measured / tolerance."""
    A = contracted(hp(T))
    n = A.shape[-1]
    lam, Y = hp(lam), hp(Y)
    tol = EIGH_TOL[dtype]
    ref_l, ref_Z = torch.linalg.eigh(A)
    sl = slice(n - p, n) if uppest else slice(0, p)
    tnorm = max(ref_l.abs().max().item(), 1e-300)       # |T|_2 of a Hermitian matrix, the largest over the batch
    assert bool(torch.isfinite(lam).all() and torch.isfinite(torch.view_as_real(Y)).all()), what + ": non-finite"
    r = {"lam": (lam - ref_l[:, sl]).abs().max().item() / (tol["lam"] * tnorm)}
    assert bool((lam[:, 1:] >= lam[:, :-1]).all()), what + ": eigenvalues not ascending"
    Yc = Y.transpose(-2, -1)
    res = torch.matmul(A, Yc) - Yc * lam.unsqueeze(-2).to(c128)
    r["res"] = res.abs().max().item() / (tol["res"] * n * tnorm)
    Gm = torch.matmul(Yc.transpose(-2, -1).conj(), Yc) - torch.eye(p, dtype=c128)
    r["orth"] = Gm.abs().max().item() / tol["orth"]
    r["proj"] = 0.0
    for b in range(A.shape[0]):
        if p < n:
            edge = (ref_l[b, p] - ref_l[b, p - 1]) if not uppest else (ref_l[b, n - p] - ref_l[b, n - p - 1])
            if not edge.item() > EIGH_GAP * tnorm:
                continue
        Zb = ref_Z[b][:, sl]
        P1, P2 = Yc[b] @ Yc[b].conj().T, Zb @ Zb.conj().T
        r["proj"] = max(r["proj"], (P1 - P2).abs().max().item() / tol["proj"])
    for name, v in r.items():
        assert v <= 1.0, "%s: %s is %.3e of its tolerance" % (what, name, v)
        _record(dtype, "herm_eigh:" + name, v)
    return r


# ------------------------------------------------------------------------------------------------ dense_outer_complex
def outer_embedding(U, W, fault=None):
    """the two real panels kernels.dense_outer_complex hands to xk_dense_outer: (B, 2C, M) and (B, 2C, 2N)"""
    B, C, N = W.shape
    Ur = torch.cat([U.real, U.imag], dim=1)
    Wr = torch.empty((B, 2 * C, N, 2), dtype=torch.float64)
    s = 1.0 if fault == "outer_no_conj" else -1.0
    Wr[:, :C, :, 0] = W.real
    Wr[:, :C, :, 1] = s * W.imag
    Wr[:, C:, :, 0] = -s * W.imag
    Wr[:, C:, :, 1] = W.real
    return Ur, Wr.reshape(B, 2 * C, 2 * N)


def dense_outer_complex(U, W, dtype, fault=None):
    """G[i,j] = sum_c U[c,i] conj(W[c,j]): a real outer product with 2C columns in the interleaved storage, so the
    term count is solver_ref.dense_outer's on that embedding (2C products over ceil(2C / 8) passes).  Returns the
    value as the real (B, M, 2N) interleaved array, to be compared with view_as_real of the kernel's output."""
    Ur, Wr = outer_embedding(U, W, fault)
    Ur0, Wr0 = outer_embedding(U, W)
    val = sref.dense_outer(REAL[dtype], Ur, Wr)["G"][0]
    bnd = sref.dense_outer(REAL[dtype], Ur0, Wr0)["G"][1]
    return {"G": (val, bnd)}


# ------------------------------------------------------------------------------------------------ checking
def _record(dtype, kernel, ratio):
    key = (DNAME.get(dtype, str(dtype)), kernel)
    WORST[key] = max(WORST.get(key, 0.0), ratio)


def _realview(t, like_complex):
    t = hp(t)
    return torch.view_as_real(t.to(c128)) if like_complex else t


def check(got, ref, dtype, what="", kernel=None):
    """Compare kernel outputs (name -> tensor) with the reference (name -> (value, bound); names starting with "_" are
    skipped).  Complex values are compared component-wise: real and imaginary part each within `bound`.  Finite
    reference components must be within the bound, non-finite ones matched exactly (the same infinity, or NaN).
    Raises AssertionError on the first violation; returns the worst ratio and records it in WORST."""
    worst = 0.0
    for name, vb in ref.items():
        if name.startswith("_"):
            continue
        val, bnd = vb
        assert name in got, "%s: no kernel output %r" % (what, name)
        cx = val.is_complex()
        g = _realview(got[name].reshape(val.shape), cx)
        v = torch.view_as_real(val) if cx else val
        b = bnd.unsqueeze(-1).expand_as(v) if cx else bnd
        fin = torch.isfinite(v)
        nf_ok = torch.where(torch.isnan(v), torch.isnan(g), g == v)
        if not bool((fin | nf_ok).all()):
            idx = (~(fin | nf_ok)).nonzero()[0].tolist()
            raise AssertionError("%s: %s at %s: got %r, want non-finite %r" % (what, name, idx, g[tuple(idx)].item(),
                                                                               v[tuple(idx)].item()))
        err = torch.where(fin, (g - v).abs(), torch.zeros_like(v))
        err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
        b = torch.where(fin, b, torch.zeros_like(b))
        ok = err <= b
        if not bool(ok.all()):
            idx = (~ok).nonzero()[0].tolist()
            raise AssertionError("%s: %s out of bounds at %s: got %r, want %r, |err| %.3e > bound %.3e (%d entries)"
                                 % (what, name, idx, g[tuple(idx)].item(), v[tuple(idx)].item(),
                                    err[tuple(idx)].item(), b[tuple(idx)].item(), int((~ok).sum())))
        nz = b > 0
        if bool(nz.any()):
            worst = max(worst, float((err[nz] / b[nz]).max()))
    _record(dtype, kernel or what.split(" ")[0], worst)
    return worst


def values(ref, dtype=None):
    """the reference values alone (rounded to the kernel dtype when given): what a kernel would write.  float64
    outputs of every kernel (`status`) are not rounded."""
    out = {}
    for name, vb in ref.items():
        if name.startswith("_"):
            continue
        val = vb[0]
        out[name] = rnd(val, dtype) if (dtype is not None and name != "status") else val
    return out


# ------------------------------------------------------------------------------------------------ configurations
# tests/test_gpu_herm_kernels.py and tests/test_herm_ref.py both iterate these lists and build their inputs with the
# *_case functions, so the CPU test sees the GPU test's very inputs.
RITZ_B = (1, 3)
RITZ_K = (1, 5, 40, 128)
RITZ_P = (1, 6, 15, 16, 17, 32)
RITZ_N = (1, 255, 256, 257, 1037)
RITZ_LONG = (3, 5, 17, 65536 + 300, True, "transposed")       # one N beyond 65536 elements
Y_LAYOUTS = ("contiguous", "transposed", "strided")


def ritz_configs(k):
    """(B, k, p, N, with_m, y_layout) for one k: every (p, N) twice, B / with_m / layout dealt round-robin so that
    each value meets every p and every N"""
    out = []
    i = 0
    for p in RITZ_P:
        for N in RITZ_N:
            for B in RITZ_B:
                out.append((B, k, p, N, bool((i // 2 + i) % 2), Y_LAYOUTS[i % 3]))
                i += 1
    return out


def ritz_case(dtype, B, k, p, N, with_m):
    """inputs as the kernel reads them (rounded to dtype), complex128 / float64 on the CPU"""
    g = gen(1, B, k, p, N, with_m)
    c = {"V": rnd(crand(g, B, k, N), dtype), "AV": rnd(crand(g, B, k, N), dtype),
         "MV": rnd(crand(g, B, k, N), dtype) if with_m else None,
         "Y": rnd(crand(g, B, k, p), dtype), "lam": rnd(torch.randn(B, p, dtype=torch.float64, generator=g), dtype)}
    return c


def ritz_plant(c, value):
    """the case with one non-finite real part planted in AV of the last member"""
    AV = c["AV"].clone()
    B, k, N = AV.shape
    AV[B - 1, k // 2, N // 3] = complex(value, 0.25)
    return dict(c, AV=AV)


CHOL_Q = (1, 2, 6, 17, 22, 23, 31, 32)
CHOL_N = (64, 255, 256, 257, 777, 1037, 4099)
CHOL_B = 2


def shift_rel(N, q, dtype):
    """the driver's first-pass shift (native_eig_herm._shift_rel, restated so that the CPU suite needs no device
    module; tests/test_gpu_herm_kernels.py asserts the two agree)"""
    return min(11.0 * (N * q + q * (q + 1)) * unit_roundoff(dtype), 1e-3)


def cholqr_entry_configs(N):
    """(q, N, with_m, shifted) of the per-entry family for one N (N = 33 goes with q <= 17: beyond, kappa_2(G) of a
    Gaussian block reaches 1e3 .. 1e4)"""
    qs = [q for q in CHOL_Q if (N != 33 or q <= 17)]
    return [(q, N, m, s) for q in qs for m in (False, True) for s in (False, True)]


# properties family: (kind, q, N, with_m, shifted); "dep": W[:, 1] = W[:, 0] + 1e-3 noise
CHOL_PROP_CONFIGS = tuple(
    [("gauss", q, 33, m, s) for q in (31, 32) for m in (False, True) for s in (False, True)] +
    [("gauss", q, 20, False, s) for q in (1, 6, 17) for s in (False, True)] +
    [("dep", q, N, m, s) for q in (2, 6, 32) for N in (257, 1037) for m in (False, True) for s in (False, True)])


@functools.lru_cache(maxsize=1)
def _cholqr_block(N):
    """(W, M W, L) for the widest block of length N, complex128: narrower blocks take its first rows.  M = L L^H + I with
    L = 0.3 / sqrt(N) times a Gaussian matrix, one M for both members (as tests/test_gpu_davidson_hermitian.py builds
    it); applied as L (L^H w) + w"""
    g = gen(2, N)
    W = crand(g, CHOL_B, 32, N)
    L = crand(g, N, N) * (0.3 / N ** 0.5)
    Wc = W.transpose(1, 2)                                              # (B, N, q) columns
    MWc = torch.matmul(L, torch.matmul(L.transpose(0, 1).conj(), Wc)) + Wc
    return W, MWc.transpose(1, 2).contiguous(), L


def cholqr_case(dtype, q, N, with_m, kind="gauss"):
    W, MW, L = _cholqr_block(N)
    W, MW = W[:, :q].clone(), MW[:, :q].clone()
    if kind == "dep":
        g = gen(3, q, N)
        noise = 1e-3 * crand(g, CHOL_B, N)
        W[:, 1] = W[:, 0] + noise
        MW[:, 1] = MW[:, 0] + torch.matmul(torch.matmul(noise, L.conj()), L.transpose(0, 1)) + noise   # + (M noise)^T
    return {"W": rnd(W, dtype), "MW": rnd(MW, dtype) if with_m else None}


EIGH_N = (1, 2, 3, 7, 33, 63, 64, 65, 100, 127, 128)
EIGH_P = (1, 6, 16)
EIGH_B = 3
EIGH_KINDS = ("generic", "separated", "cluster", "diagonal", "real", "imaginary")


def _unitary(g, B, n):
    Q, _ = torch.linalg.qr(crand(g, B, n, n))
    return Q


def eigh_matrix(kind, n, g, B=EIGH_B):
    """exactly Hermitian (B, n, n) complex128 matrices; None where the construction needs a larger n.  `separated` and
    `cluster` are the constructions of tests/test_gpu_davidson_hermitian.py."""
    if kind == "generic":
        H = crand(g, B, n, n)
        return (H + H.transpose(-2, -1).conj()) * 0.5
    if kind == "separated":
        if n < 17:
            return None
        ends = torch.tensor([-10.0, -9.0, -8.2, -7.5, -6.7, -6.0, -5.4, -4.8], dtype=torch.float64)
        d = torch.cat((ends, torch.rand(n - 16, dtype=torch.float64, generator=g) * 2 - 1, -ends.flip(0)))
    elif kind == "cluster":
        if n < 7:
            return None
        d = torch.cat((torch.full((5,), -3.0, dtype=torch.float64), torch.rand(n - 5, dtype=torch.float64, generator=g)))
    elif kind == "diagonal":
        return torch.diag_embed(torch.randn(B, n, dtype=torch.float64, generator=g)).to(c128)
    elif kind == "real":
        H = torch.randn(B, n, n, dtype=torch.float64, generator=g)
        return ((H + H.transpose(-2, -1)) * 0.5).to(c128)
    elif kind == "imaginary":
        H = torch.randn(B, n, n, dtype=torch.float64, generator=g)
        S = (H - H.transpose(-2, -1)) * 0.5                     # i S is Hermitian with a zero diagonal
        return torch.complex(torch.diag_embed(torch.randn(B, n, dtype=torch.float64, generator=g)), S)
    else:
        raise ValueError(kind)
    Q = _unitary(g, B, n)
    A = torch.matmul(Q * d.to(c128), Q.transpose(-2, -1).conj())
    return (A + A.transpose(-2, -1).conj()) * 0.5


def eigh_case(dtype, kind, n, garbage="nan"):
    """The stored (B, n, n) block handed to the kernel, rounded to dtype: lower triangle of the matrix, an imaginary
    diagonal of finite garbage of the size of |T|, and above the diagonal NaN (`garbage="nan"`) or finite garbage
    (`"finite"`: for the CPU model of a kernel that reads it)."""
    g = gen(4, n, EIGH_KINDS.index(kind))
    A = eigh_matrix(kind, n, g)
    if A is None:
        return None
    scale = max(A.abs().max().item(), 1.0)
    T = torch.tril(A)
    up = torch.triu(torch.ones(n, n, dtype=torch.bool), 1)
    T[:, up] = complex(math.nan, math.nan) if garbage == "nan" else crand(g, EIGH_B, int(up.sum())) * scale
    sign = torch.where(torch.rand(EIGH_B, n, dtype=torch.float64, generator=g) < 0.5, -1.0, 1.0)
    im = sign * (0.5 + torch.rand(EIGH_B, n, dtype=torch.float64, generator=g)) * scale
    T = T + torch.diag_embed(torch.complex(torch.zeros_like(im), im))
    return rnd(T, dtype)


OUTER_C = (1, 2, 7, 16)
OUTER_MN = ((1, 1), (24, 24), (130, 70), (257, 513))
OUTER_B = (1, 3)


def outer_case(dtype, B, C, M, N):
    g = gen(5, B, C, M, N)
    return rnd(crand(g, B, C, M), dtype), rnd(crand(g, B, C, N), dtype)
