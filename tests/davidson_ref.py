"""Float64 restatement of the block-Davidson basis and chain kernels (xk_basis.hip, xk_chain.hip), with error bounds.

For every kernel (xk_lincomb, xk_ritz_residual, xk_diag_precond, xk_panel_transform, xk_davidson_extend_t,
xk_davidson_orth, xk_davidson_ritz) a function computes, from the very inputs the kernel is given (read back in the
kernel dtype, widened to float64), what the kernel must write.  The formulas are those of the header comments of
include/xitorch_amd.h and of the C sequence in xk_chain.hip (davidson_orth_block, panel_cholqr).

Each function returns {name: (value, bound)}: `value` in float64, `bound` a per-entry absolute bound on
|kernel - value| derived from the unit roundoff u of the KERNEL dtype.  A non-finite reference value must be
matched exactly (same infinity, or NaN); its bound is ignored.  `check()` compares kernel outputs with that and
raises AssertionError naming the first output out of bounds.

The `fault=` argument produces plausible kernel bugs (FAULTS).  tests/test_davidson_ref.py feeds those outputs to
`check()` (or to the exact relations the GPU tests assert) and shows that every one of them is rejected.
"""
import math
import torch

# C_TOL: every bound is C_TOL * u * (number of sequential roundings a term goes through) * (sum of the magnitudes of
# the terms).  A sum of n products accumulated in one register has |err| <= gamma_n sum|terms|, gamma_n = n u / (1 -
# n u) (Higham, Accuracy and Stability, 3.1); a reduction tree of depth d adds d to n.  The longest elementwise chains
# after such a sum are two more roundings (beta*Out + alpha*acc; AX - lam*X then the product lam*X), and the float64
# reference carries its own rounding of the same order, which for the float64 kernels at most doubles the first-order
# error.  The (k + 2), (terms + 6 + nsplit) counts below already include the trailing roundings, so C_TOL = 8 leaves a
# factor of two above both contributions while staying tight enough that every fault of FAULTS moves an output by
# many bounds at the shapes of tests/test_davidson_ref.py.
C_TOL = 8.0

# elements per 16 B vector: the kernels' VN
VEC_ELEMS = {torch.float64: 2, torch.float32: 4}

# xk_davidson_orth: CholeskyQR outputs are compared entry-wise only for panels whose Gram matrix has condition
# number kappa^2 <= KAPPA2_MAX (kappa: condition number of the panel after its projection).  The bound on Q grows
# like kappa^2 (one CholeskyQR loses orthogonality ~ kappa^2 u, Yamamoto et al. 2015); panels beyond the limit are
# checked by their properties (`orth_properties`) and by the exact `info` / `cond` relations instead.
KAPPA2_MAX = {torch.float64: 1e6, torch.float32: 1e2}

FAULTS = (
    "drop_k8", "drop_k4", "drop_k2",            # remainder of the k loop dropped (rows k - k % m .. k - 1)
    "drop_last_vec",                            # the last 16 B vector of N neither read nor written
    "chunk_coef", "chunk_lam", "chunk_out",     # P > 8: column chunk c0 >= 8 without its offset in C / Y, lam, output
    "swap_layout",                              # lincomb: C[b,c,a] read where C[b,a,c] is meant
    "beta_ignored",                             # lincomb: Out = alpha * sum, without beta * Out
    "w_lower",                                  # panel_transform: W read from its lower triangle
    "no_mirror", "mirror_off",                  # extend_t: no mirrored columns / mirror at column c instead of k0 + c
    "drop_last_row",                            # extend_t: the last row of the K1 Gram block masked away
    "no_second_projection", "no_shift",         # orth: projection of round 2 skipped / first round not shifted
    "cond_round",                               # orth: cond taken from the last CholeskyQR round, not the first
    "nan_dropped",                              # ritz_residual: NaN residual entries dropped from rmax (the old kernel)
    "floor_sign",                               # diag_precond: the floored denominator with the opposite sign
    "d_stride",                                 # diag_precond: broadcast d read with a member stride
)

# worst |kernel - reference| / bound seen by check(), per (kernel dtype, kernel) (reported by the GPU runs)
WORST = {}


def unit_roundoff(dtype):
    return torch.finfo(dtype).eps / 2


def hp(t):
    """float64 copy on the CPU"""
    return t.detach().cpu().to(torch.float64)


def cast(x, dtype):
    """a double argument as the C entry point sees it after `(T)x`"""
    return float(torch.tensor(x, dtype=torch.float64).to(dtype).item())


def _cu(dtype):
    return C_TOL * unit_roundoff(dtype)


def _keep_rows(k, fault):
    for m in (8, 4, 2):
        if fault == "drop_k%d" % m:
            return k - k % m
    return k


def _last_vec(N, dtype):
    vn = VEC_ELEMS[dtype]
    return (N - 1) // vn * vn


def sentinel_columns(N, dtype):
    """element indices that carry sentinels: N - 1 and the first element of the last 256 * VN column tile (the
    streaming kernels give each thread VN elements, 256 threads per column tile)"""
    tile = 256 * VEC_ELEMS[dtype]
    return sorted({N - 1, (N - 1) // tile * tile})


# ------------------------------------------------------------------------------------------------ K1 Gram terms
def _choose_nsplit(B, M, N, R, vn):
    """replica of xk_dense.hip choose_nsplit"""
    waves = B * ((M + R - 1) // R)
    nsteps = (N + 64 * vn - 1) // (64 * vn)
    if waves >= 2048 or nsteps < 16:
        return 1
    ns = (4096 + waves - 1) // waves
    ns = min(ns, max(nsteps // 8, 1), 64)
    return max(ns, 1)


def dense_dot_terms(dtype, B, M, N):
    """the n of gamma_n for one entry of a K1 row-sweep Gram block (xk_dense_mm, trans = 0), derived from
    xk_dense.hip:
      * dense_mm_rows: lane l of a wave reads VN elements per step of 64 * VN columns and accumulates them in one
        register: at most VN * ceil(N / (64 VN)) sequential terms (the scalar fallback for N % VN != 0 takes one
        element per lane per step of 64: ceil(N / 64), never more);
      * wave_reduce_scatter: a transposing butterfly over the 64 lanes, 6 levels;
      * with a split contraction (choose_nsplit, only for few waves and >= 16 steps) each split sums fewer steps and
        fold_splits adds the nsplit partials sequentially in fixed order: + nsplit.  The row count R per wave is
        RowsFor<P> (4 .. 16); the largest nsplit over those R is taken, as xk_dense_mm_workspace_elems does."""
    vn = VEC_ELEMS[dtype]
    per_thread = vn * ((N + 64 * vn - 1) // (64 * vn))
    nsplit = max(_choose_nsplit(B, M, N, R, vn) for R in (4, 8, 12, 16)) if N % vn == 0 else 1
    return per_thread + 6 + nsplit


def fused_gram_terms(dtype, N):
    """the same for the Gram entries of the fused CholeskyQR (panel_cholqr_kernel, q <= 8): 1024 threads stride the
    padded panel VN elements at a time (VN * ceil(Npad / (1024 VN)) terms per thread), wave_sum (6 levels), then the
    16 wave partials added in fixed order (16)"""
    vn = VEC_ELEMS[dtype]
    return vn * ((N + 1024 * vn - 1) // (1024 * vn)) + 6 + 16


# ------------------------------------------------------------------------------------------------ the kernels
def lincomb(V, C, Out, alpha, beta, dtype, fault=None):
    """xk_lincomb: Out[b,c,:] = beta*Out[b,c,:] + alpha * sum_{a<k} C[b,a,c] V[b,a,:].
    V (B, k, N), C (B, k, P) indexed [b, a, c] whatever the layout the kernel was given, Out (B, P, N) the values
    before the call.  alpha, beta as the kernel sees them (`cast`).  The kernel accumulates the k terms of an entry
    sequentially in one register (8-, 4-, 1-row trips, no reduction tree), then one product and one add."""
    k, P = C.shape[1], C.shape[2]
    if fault == "swap_layout":
        C = C.transpose(1, 2)                   # a square block read with its two indices exchanged
    if fault == "chunk_coef" and P > 8:
        C = torch.cat([C[:, :, :8], C[:, :, torch.arange(8, P) % 8]], 2)
    keep = _keep_rows(k, fault)
    Vk, Ck = V[:, :keep], C[:, :keep]
    acc = torch.einsum("bac,ban->bcn", Ck, Vk)
    be = 0.0 if fault == "beta_ignored" else beta
    val = alpha * acc + (be * Out if be != 0 else 0 * acc)
    mag = abs(alpha) * torch.einsum("bac,ban->bcn", C.abs(), V.abs())
    if beta != 0:                               # beta == 0: Out is not read (it may hold NaN)
        mag = mag + abs(beta) * Out.abs()
    bnd = _cu(dtype) * (k + 3) * mag
    if fault == "chunk_out" and P > 8:
        val = val.clone()
        val[:, torch.arange(8, P) % 8] = val[:, 8:].clone()
        val[:, 8:] = Out[:, 8:]
    if fault == "drop_last_vec":
        val = val.clone()
        val[..., _last_vec(V.shape[-1], dtype):] = Out[..., _last_vec(V.shape[-1], dtype):]
    return {"Out": (val, bnd)}


def rmax_of(R):
    """max |R| over (P, N) per member, a NaN entry counting as +inf (the header's contract)"""
    a = R.abs().flatten(1)
    a = torch.where(torch.isnan(a), torch.full_like(a, math.inf), a)
    return a.max(1).values if a.shape[1] else torch.zeros(a.shape[0], dtype=a.dtype)


def ritz_residual(V, AV, Y, lam, dtype, fault=None):
    """xk_ritz_residual: X = Y^T V, AX = Y^T AV, Tn = -(AX - lam X), rmax[b] = max |AX - lam X| (NaN as +inf).
    V, AV (B, k, N), Y (B, k, P) [b, a, c], lam (B, P).  Per entry: two sequential k-term sums in registers, the
    product lam * X and the difference: the bound on Tn is C u (k + 2) (sum|Y||AV| + |lam| sum|Y||V|)."""
    k, P = Y.shape[1], Y.shape[2]
    keep = _keep_rows(k, fault)
    Yu, lamu = Y, lam
    if P > 8 and fault == "chunk_coef":
        Yu = torch.cat([Y[:, :, :8], Y[:, :, torch.arange(8, P) % 8]], 2)
    if P > 8 and fault == "chunk_lam":
        lamu = torch.cat([lam[:, :8], lam[:, torch.arange(8, P) % 8]], 1)
    X = torch.einsum("bac,ban->bcn", Yu[:, :keep], V[:, :keep])
    AX = torch.einsum("bac,ban->bcn", Yu[:, :keep], AV[:, :keep])
    R = AX - lamu.unsqueeze(-1) * X
    Tn = -R
    Ya = Y.abs()
    sv = torch.einsum("bac,ban->bcn", Ya, V.abs())
    sav = torch.einsum("bac,ban->bcn", Ya, AV.abs())
    cu = _cu(dtype)
    bx = cu * (k + 1) * sv
    bt = cu * (k + 2) * (sav + lam.abs().unsqueeze(-1) * sv)
    if fault == "drop_last_vec":
        lv = _last_vec(V.shape[-1], dtype)
        X, Tn, R = X.clone(), Tn.clone(), R.clone()
        X[..., lv:] = 0
        Tn[..., lv:] = 0
        R[..., lv:] = 0
    if fault == "chunk_out" and P > 8:
        X, Tn = X.clone(), Tn.clone()
        for t in (X, Tn):
            t[:, torch.arange(8, P) % 8] = t[:, 8:].clone()
            t[:, 8:] = 0
    if fault == "nan_dropped":
        a = R.abs().flatten(1)
        rmax = torch.where(torch.isnan(a), torch.zeros_like(a), a).max(1).values
    else:
        rmax = rmax_of(R)
    brm = bt.flatten(1).max(1).values
    return {"X": (X, bx), "Tn": (Tn, bt), "rmax": (rmax, brm)}


def diag_precond(Tn, d, m, lam, floor, dtype, fault=None, d_wrong=None):
    """xk_diag_precond: Tn[b,c,n] /= den, den = d[b,n] - lam[b,c] * m[b,n] (m absent: 1); |den| < floor gives
    den = -floor for den < 0, +floor otherwise (so an exact zero, either sign, gives +floor); a NaN den fails the
    comparison and passes through.  d, m (1 or B, N), floor as the kernel sees it (`cast`).  d_wrong (B, N): what a
    member would read with the "d_stride" fault."""
    B, P, N = Tn.shape
    dd = d.expand(B, N)
    if fault == "d_stride":
        dd = d_wrong
    mm = torch.ones(B, N, dtype=torch.float64) if m is None else m.expand(B, N)
    den = dd.unsqueeze(1) - lam.unsqueeze(-1) * mm.unsqueeze(1)
    eden = _cu(dtype) * (dd.abs().unsqueeze(1) + (lam.unsqueeze(-1) * mm.unsqueeze(1)).abs())
    small = den.abs() < floor
    sgn = -1.0 if fault == "floor_sign" else 1.0
    fl = torch.where(den < 0, torch.full_like(den, -floor * sgn), torch.full_like(den, floor * sgn))
    den_eff = torch.where(small, fl, den)
    q = Tn / den_eff
    bnd = _cu(dtype) * q.abs() + torch.where(small, torch.zeros_like(q), q.abs() * eden / den.abs())
    # within rounding of the floor the kernel may take either branch: accept both
    amb = ((den.abs() - floor).abs() <= eden) & (den != 0)
    both = (Tn / floor).abs() + q.abs()
    bnd = torch.where(amb, both, bnd)
    return {"Tn": (q, bnd)}


def panel_transform(Tp, W, dtype, fault=None):
    """xk_panel_transform: Tp[c] <- sum_{a<=c} W[a,c] Tp[a], only the upper triangle of W (B, P, P) read.  One
    register per output row, c + 1 sequential terms."""
    P = W.shape[1]
    Wu = torch.triu(W.transpose(1, 2) if fault == "w_lower" else W)
    val = torch.einsum("bac,ban->bcn", Wu, Tp)
    mag = torch.einsum("bac,ban->bcn", torch.triu(W).abs(), Tp.abs())
    bnd = _cu(dtype) * (torch.arange(P, dtype=torch.float64).view(1, P, 1) + 2) * mag
    if fault == "drop_last_vec":
        val = val.clone()
        val[..., _last_vec(Tp.shape[-1], dtype):] = 0
    return {"Tp": (val, bnd)}


def extend_t(V, AV, k0, q, dtype, fault=None):
    """xk_davidson_extend_t: Tn[b,c,a] = <V_a, AV_{k0+c}> (a < k0+q) on K1 (`dense_dot_terms`), the rows
    T[b, k0+c, a] = Tn[b,c,a] (a < k0+q) and the mirrored columns T[b, a, k0+c] = Tn[b,c,a] (a < k0).
    V (B, >=k0+q, N), AV (B, >=k0+q, N).  Returns Tn (B, q, kq), Trows = T[:, k0:kq, :kq], Tcols = T[:, :k0, k0:kq]."""
    B, N, kq = V.shape[0], V.shape[-1], k0 + q
    Vr, AVr = V[:, :kq], AV[:, k0:kq]
    if fault == "drop_last_vec":
        lv = _last_vec(N, dtype)
        Vr = Vr.clone()
        Vr[..., lv:] = 0
    G = torch.einsum("ban,bcn->bca", Vr, AVr)
    bnd = _cu(dtype) * dense_dot_terms(dtype, B, kq, N) * torch.einsum("ban,bcn->bca", V[:, :kq].abs(), AVr.abs())
    if fault == "drop_last_row":
        G = G.clone()
        G[:, :, kq - 1] = 0
    cols = G[:, :, :k0].transpose(1, 2)
    if fault == "no_mirror":
        cols = torch.zeros_like(cols)
    if fault == "mirror_off":
        cols = torch.zeros_like(cols)
        for c in range(q):                        # written at column c: lands in the block only where c >= k0
            if c >= k0:
                cols[:, :, c - k0] = G[:, c, :k0]
    out = {"Tn": (G, bnd), "Trows": (G, bnd)}
    if k0 > 0:
        out["Tcols"] = (cols, bnd[:, :, :k0].transpose(1, 2))
    return out


def _chol(G):
    """the kernels' column-by-column Cholesky of (B, q, q) G: pivots s <= 0 (or NaN) set bad = first index + 1 and
    are replaced by 1; returns R (upper), squared pivots, bad (B,)"""
    B, q = G.shape[0], G.shape[1]
    R = torch.zeros_like(G)
    piv = torch.zeros(B, q, dtype=G.dtype)
    bad = torch.zeros(B, dtype=torch.long)
    for j in range(q):
        for r in range(j + 1):
            s = G[:, r, j] - (R[:, :r, r] * R[:, :r, j]).sum(-1)
            if r == j:
                nb = ~(s > 0)
                bad = torch.where(nb & (bad == 0), torch.full_like(bad, j + 1), bad)
                s = torch.where(nb, torch.ones_like(s), s)
                piv[:, j] = s
                R[:, j, j] = s.sqrt()
            else:
                R[:, r, j] = s / R[:, r, r]
    return R, piv, bad


def orth(V, k0, q, passes, dtype, info=None, cond=None, fault=None, work=torch.float64):
    """xk_davidson_orth, the exact sequence of xk_chain.hip (davidson_orth -> davidson_orth_block -> panel_cholqr):
      * the panel is taken in chunks of <= 32 rows; chunk `off` uses passes_c = passes (first chunk) or
        max(passes, 2) (later chunks), rounds = max(passes_c, 1);
      * each round: a projection against rows [0, k0 + off) when passes_c >= 1 and k0 + off > 0
        (C = P V^T on K1, P -= C V), then CholeskyQR of the chunk: G = P P^T, shifted by
        (T) min(1e-3, 11 (N qc + qc (qc + 1)) u) * trace(G) on the diagonal in the first round when rounds >= 2, R =
        chol(G), P <- R^-T P;
      * info[b] = first bad pivot + 1 of any CholeskyQR that breaks down (kept otherwise: sticky);
      * cond[b] = max(cond[b], pmax / pmin of the squared pivots) for chunks of <= 8 rows, first round only (inf on a
        breakdown).
    V (B, >=k0+q, N) before the call; info (B,) long, cond (B,) or None.  `work` is the arithmetic of the restatement:
    float64 for the reference; the kernel dtype lets tests/test_davidson_ref.py show the effect of faults that only
    act through rounding (`no_second_projection`, `no_shift`).
    Returns {"Q": (rows [k0, k0+q) after the call, bound), "info": (.., 0), "cond": (.., bound)} and, under "_meta",
    kappa2 (B,) of the projected raw panel."""
    B, N = V.shape[0], V.shape[-1]
    u = unit_roundoff(dtype)
    Vw = V[:, :k0 + q].to(work).clone()
    info = torch.zeros(B, dtype=torch.long) if info is None else info.clone().long()
    cond_v = None if cond is None else cond.clone().to(torch.float64)
    cond_b = torch.zeros(B, dtype=torch.float64)
    kappa2 = torch.ones(B, dtype=torch.float64)
    rho = torch.zeros(B, dtype=torch.float64)
    g_terms = 0
    for off in range(0, q, 32):
        qc = min(32, q - off)
        pc = passes if off == 0 else max(passes, 2)
        rounds = max(pc, 1)
        kk = k0 + off
        sh = cast(min(1e-3, 11.0 * (N * qc + qc * (qc + 1)) * u), dtype)
        g_terms = max(g_terms, fused_gram_terms(dtype, N) if qc <= 8 else dense_dot_terms(dtype, B, qc, N),
                      dense_dot_terms(dtype, B, max(kk, 1), N))
        cond_round = (rounds - 1) if fault == "cond_round" else 0
        for it in range(rounds):
            Pn = Vw[:, kk:kk + qc]
            cmax = torch.zeros(B, dtype=torch.float64)
            if kk > 0 and pc >= 1 and not (fault == "no_second_projection" and it == 1):
                Cm = torch.einsum("bcn,ban->bca", Pn, Vw[:, :kk])
                Pn = Pn - torch.einsum("bca,ban->bcn", Cm, Vw[:, :kk])
                cmax = Cm.abs().flatten(1).max(1).values.to(torch.float64)
            G = torch.einsum("bcn,bdn->bcd", Pn, Pn)
            G = 0.5 * (G + G.transpose(1, 2))
            if it == 0:
                # kappa^2 of the projected raw chunk, and rho = max|C| / sigma_min of it: the projection's rounding
                # error (~ u |C| |V| per entry) relative to the chunk that CholeskyQR then scales by 1 / sigma_min
                ev = torch.linalg.eigvalsh(G.to(torch.float64))
                lo = ev[:, 0].clamp(min=1e-300)
                kappa2 = torch.maximum(kappa2, torch.where(ev[:, 0] > 0, ev[:, -1] / lo, torch.full_like(lo, math.inf)))
                rho = torch.maximum(rho, cmax / lo.sqrt())
            if rounds >= 2 and it == 0 and fault != "no_shift":
                tr = torch.diagonal(G, dim1=1, dim2=2).sum(-1)
                G = G + (sh * tr).view(B, 1, 1) * torch.eye(qc, dtype=G.dtype)
            R, piv, bad = _chol(G)
            W = torch.linalg.inv(R)
            Vw[:, kk:kk + qc] = torch.einsum("bac,ban->bcn", W, Pn)
            info = torch.where(bad > 0, bad, info)
            if qc <= 8 and it == cond_round:
                ratio = piv.max(1).values / piv.min(1).values
                ratio = torch.where(bad > 0, torch.full_like(ratio, math.inf), ratio).to(torch.float64)
                if it == 0:
                    Gs = G.to(torch.float64)
                    evs = torch.linalg.eigvalsh(Gs)
                    cond_b = torch.maximum(cond_b, (evs[:, -1] / evs[:, 0].clamp(min=1e-300)))
                if cond_v is not None:
                    cond_v = torch.where(torch.isnan(cond_v) | (ratio > cond_v), ratio, cond_v)
    Q = Vw[:, k0:k0 + q].to(torch.float64)
    cu = _cu(dtype)
    scale = Q.abs().sum(1, keepdim=True) + (V[:, :k0].abs().sum(1, keepdim=True) * rho.view(B, 1, 1) if k0 else 0)
    qb = cu * kappa2.view(B, 1, 1) * (g_terms + k0 + q + 8) * scale
    out = {"Q": (Q, qb.expand_as(Q)), "info": (info.to(torch.float64), torch.zeros(B, dtype=torch.float64)),
           "_meta": {"kappa2": kappa2}}
    if cond_v is not None:
        cb = cu * (g_terms + q + 8) * cond_b * torch.where(torch.isfinite(cond_v), cond_v, torch.zeros_like(cond_v))
        out["cond"] = (cond_v, cb)
    return out


def orth_tolerance(dtype, N, k0, q):
    """|V_old Q^T| and |Q Q^T - I| after xk_davidson_orth with passes >= 2 (CholeskyQR2 is orthonormal to
    O(u (terms)) independently of the conditioning as long as the shifted first step succeeds, Fukaya et al. 2020)"""
    return _cu(dtype) * (dense_dot_terms(dtype, 1, max(k0 + q, 1), N) + k0 + q + 8) * 4


def orth_properties(V0, Q, k0, dtype):
    """(max |V_old Q^T|, max |Q Q^T - I|) per member: V0 (B, >=k0, N) rows before the call, Q (B, q, N) after"""
    B, q = Q.shape[0], Q.shape[1]
    po = (torch.einsum("ban,bcn->bac", V0[:, :k0], Q).abs().flatten(1).max(1).values if k0
          else torch.zeros(B, dtype=torch.float64))
    G = torch.einsum("bcn,bdn->bcd", Q, Q) - torch.eye(q, dtype=torch.float64)
    return po, G.abs().flatten(1).max(1).values


def status_of(rmax, info, flag=None, cond=None, orth=None):
    """xk_davidson_ritz's status from the values the kernel folded (each in its own dtype): {max_b rmax (NaN if any is
    NaN), max_b info, max_b flag or 0, max_b cond (NaN as inf), max_b orth (NaN as inf)} as doubles"""
    r = rmax.double().cpu()
    s = [math.nan if bool(torch.isnan(r).any()) else float(r.max()), float(info.max()),
         float(flag.max()) if flag is not None else 0.0]
    for v in (cond, orth):
        if v is None:
            s.append(None)
        else:
            v = v.double().cpu()
            s.append(math.inf if bool(torch.isnan(v).any()) else max(0.0, float(v.max())))
    return s


# ------------------------------------------------------------------------------------------------ checking
def check(got, ref, dtype, what="", kernel=None):
    """Compare kernel outputs (`got`: name -> tensor of the reference value's shape) with the reference (`ref`:
    name -> (value, bound); names starting with "_" are skipped).  Finite reference entries must be within their
    bound; non-finite ones must be matched exactly (the same infinity, or NaN).  Raises AssertionError on the first
    violation; returns the worst error / bound ratio and records it in WORST[(dtype, kernel)]."""
    worst = 0.0
    for name, vb in ref.items():
        if name.startswith("_"):
            continue
        val, bnd = vb
        assert name in got, "%s: no kernel output %r" % (what, name)
        g = hp(got[name]).reshape(val.shape)
        fin = torch.isfinite(val)
        nf_ok = torch.where(torch.isnan(val), torch.isnan(g), g == val)
        if not bool((fin | nf_ok).all()):
            idx = (~(fin | nf_ok)).nonzero()[0].tolist()
            raise AssertionError("%s: %s at %s: got %r, want non-finite %r" % (what, name, idx, g[tuple(idx)].item(),
                                                                               val[tuple(idx)].item()))
        err = torch.where(fin, (g - val).abs(), torch.zeros_like(val))
        err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
        b = torch.where(fin, bnd, torch.zeros_like(bnd))
        ok = err <= b
        if not bool(ok.all()):
            idx = (~ok).nonzero()[0].tolist()
            raise AssertionError("%s: %s out of bounds at %s: got %r, want %r, |err| %.3e > bound %.3e (%d entries)"
                                 % (what, name, idx, g[tuple(idx)].item(), val[tuple(idx)].item(),
                                    err[tuple(idx)].item(), b[tuple(idx)].item(), int((~ok).sum())))
        nz = b > 0
        if bool(nz.any()):
            worst = max(worst, float((err[nz] / b[nz]).max()))
    key = (str(dtype).replace("torch.", ""), kernel or what.split(" ")[0])
    WORST[key] = max(WORST.get(key, 0.0), worst)
    return worst


def values(ref, dtype=None):
    """the reference values alone (rounded to the kernel dtype when given): what a kernel would write"""
    out = {}
    for name, vb in ref.items():
        if name.startswith("_"):
            continue
        val = vb[0]
        out[name] = val.to(dtype) if dtype is not None else val
    return out


# ------------------------------------------------------------------------------------------------ inputs
def rand(g, *shape, scale=1.0):
    return torch.randn(*shape, dtype=torch.float64, generator=g) * scale


def add_sentinels(t, dtype, rows=(), cols=(), factor=1e3):
    """scale entries of the (B, R, N) / (B, R, C) array `t` in place by `factor`: every row of `rows`, and every column
    (last index) of `cols`"""
    for r in rows:
        t[:, r] *= factor
    for c in cols:
        t[..., c] *= factor
    return t
