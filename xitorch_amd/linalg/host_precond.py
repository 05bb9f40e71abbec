"""FSAI in torch ops: the pattern of G (every device) and its values for operators in host memory or of a dtype the HIP
kernel does not serve; `fsai_lu_values` is the same for the unsymmetric form (two factors, pivoted LU per block).

The values are the algorithm of xk_fsai_build (csrc/xk_fsai.hip) restated with batched library calls: the rows of G are
grouped by their length m, the m x m blocks A[S_i, S_i] of a group are gathered at once, factored by
`torch.linalg.cholesky_ex`, and L^H z = e_m is one triangular solve; row i of G is conj(z).  A block that is not
numerically positive definite gives the Jacobi row and is counted.  In float64 / complex128 this is the restatement the
kernel is tested against.  No Python loop runs over rows: one pass per distinct row length (at most 32), cut into chunks
that bound the memory of the gathered blocks.
"""
import torch

__all__ = ["fsai_pattern", "fsai_values", "fsai_lu_values"]

_CHUNK_ELEMS = 1 << 22          # elements of the gathered blocks held at once


def _row_ptr(rows, N):
    ptr = torch.zeros(N + 1, dtype=torch.int64, device=rows.device)
    ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
    return ptr


def fsai_pattern(row_of, col, N, power=1, max_row=32, full=False):
    """Pattern of G: row i takes the columns j <= i of row i of |A|^power — A's structure being its stored lower triangle
    mirrored (full=True, the unsymmetric FSAI: ALL its stored entries, both triangles, mirrored) — plus i itself; a row
    longer than max_row keeps its max_row LARGEST columns.  -> (g_ptr (N+1,), g_idx) int32, columns ascending and unique,
    the diagonal last in every row."""
    dev = col.device
    r, c = row_of.to(torch.int64), col.to(torch.int64)
    if not full:
        low = c <= r
        r, c = r[low], c[low]
    ar = torch.arange(N, dtype=torch.int64, device=dev)
    keys = torch.unique(torch.cat([r * N + c, c * N + r, ar * N + ar]))          # sorted: by row, then by column
    i1, j1 = keys // N, keys % N
    ptr1 = _row_ptr(i1, N)
    cnt1 = ptr1[1:] - ptr1[:-1]
    ci, cj = i1, j1
    for _ in range(power - 1):
        # structure of S * S1: every entry (i, k) of S spawns (i, j) for the j of row k of S1
        reps = cnt1[cj]
        tot = int(reps.sum())
        ii = torch.repeat_interleave(ci, reps, output_size=tot)
        first = torch.repeat_interleave(ptr1[cj] - (torch.cumsum(reps, 0) - reps), reps, output_size=tot)
        jj = j1[first + torch.arange(tot, dtype=torch.int64, device=dev)]
        keys = torch.unique(ii * N + jj)
        ci, cj = keys // N, keys % N
    low = cj <= ci
    ci, cj = ci[low], cj[low]
    ptr = _row_ptr(ci, N)
    cnt = ptr[1:] - ptr[:-1]
    pos = torch.arange(ci.numel(), dtype=torch.int64, device=dev) - ptr[ci]
    keep = pos >= cnt[ci] - max_row                                              # the columns nearest the diagonal
    ci, cj = ci[keep], cj[keep]
    return _row_ptr(ci, N).to(torch.int32), cj.to(torch.int32).contiguous()


def fsai_values(a_row, a_col, a_val, g_ptr, g_idx, N):
    """Values of G on the pattern (g_ptr, g_idx) for the Hermitian operator whose stored entries are (a_row, a_col,
    a_val (nb, nnz)): only entries with column <= row are read, duplicates add up, the imaginary part of a diagonal
    entry is ignored.  -> (g_val (nb, g_nnz), nfail (nb,) int64: rows that fell back to the Jacobi row)."""
    dev, dtype = a_val.device, a_val.dtype
    nb = a_val.shape[0]
    r, c = a_row.to(torch.int64), a_col.to(torch.int64)
    low = c <= r
    ukeys, inv = torch.unique(r[low] * N + c[low], return_inverse=True)
    nu = ukeys.numel()
    uval = torch.zeros((nb, nu), dtype=dtype, device=dev).index_add(1, inv, a_val[:, low])
    gp, gi = g_ptr.to(torch.int64), g_idx.to(torch.int64)
    lens = gp[1:] - gp[:-1]
    g_val = torch.zeros((nb, gi.numel()), dtype=dtype, device=dev)
    nfail = torch.zeros((nb,), dtype=torch.int64, device=dev)
    rdtype = torch.zeros((), dtype=dtype).real.dtype
    for m in torch.unique(lens).tolist():
        rows_m = torch.nonzero(lens == m).reshape(-1)
        am = torch.arange(m, dtype=torch.int64, device=dev)
        lower = am[:, None] >= am[None, :]
        e = torch.zeros((m, 1), dtype=dtype, device=dev)
        e[-1] = 1
        chunk = max(1, _CHUNK_ELEMS // (m * m * nb))
        for s in range(0, rows_m.numel(), chunk):
            slot = gp[rows_m[s:s + chunk]][:, None] + am                         # (nr, m) positions in G
            S = gi[slot]
            Q = S[:, :, None] * N + S[:, None, :]                                # key of A[S_r, S_c]
            if nu:
                p = torch.searchsorted(ukeys, Q.reshape(-1)).clamp_(max=nu - 1).reshape(Q.shape)
                hit = (ukeys[p] == Q) & lower
                blk = torch.where(hit, uval[:, p], torch.zeros((), dtype=dtype, device=dev))
            else:
                blk = torch.zeros((nb, *Q.shape), dtype=dtype, device=dev)
            dg = torch.diagonal(blk, dim1=-2, dim2=-1)
            if dtype.is_complex:
                dg.copy_(dg.real.to(dtype))
            full = blk + torch.tril(blk, -1).mH
            L, info = torch.linalg.cholesky_ex(full)
            z = torch.linalg.solve_triangular(L.mH, e, upper=True).squeeze(-1)   # L^H z = e_m
            g = z.conj()
            piv = torch.diagonal(L, dim1=-2, dim2=-1).real
            bad = (info != 0) | ~torch.isfinite(piv).all(-1) | (piv <= 0).any(-1) | ~torch.isfinite(g).all(-1)
            aii = dg[..., m - 1].real.abs()
            jd = torch.where((aii > 0) & torch.isfinite(aii), 1 / torch.sqrt(aii), torch.ones((), dtype=rdtype, device=dev))
            jac = torch.zeros_like(g)
            jac[..., m - 1] = jd.to(dtype)
            g = torch.where(bad[..., None], jac, g)
            g_val[:, slot] = g.resolve_conj()
            nfail += bad.sum(1)
    return g_val, nfail


def fsai_lu_values(a_row, a_col, a_val, g_ptr, g_idx, N):
    """Values of the unsymmetric FSAI factors on the one pattern (g_ptr, g_idx) for the operator whose stored entries are
    (a_row, a_col, a_val (nb, nnz)), the algorithm of xk_fsai_lu_build (csrc/xk_fsai_lu.hip) in batched library calls:
    per row the full block A[S, S] (duplicates add up, unstored entries are zero), one `torch.linalg.lu_factor_ex`, then
    A_SS u = e_m and A_SS^T g = e_m; row i of G_L is g / g_m with a unit diagonal, row i of W = G_U^H is conj(u).  A row
    with a zero or non-finite pivot, a non-finite u or g, or g_m = 0 falls back to G_L[i, .] = e_i, G_U[., i] = e_i / a_ii
    (e_i for a zero or non-finite a_ii).  -> (gl_val, w_val (nb, g_nnz), nfail (nb,) int64)."""
    dev, dtype = a_val.device, a_val.dtype
    nb = a_val.shape[0]
    r, c = a_row.to(torch.int64), a_col.to(torch.int64)
    ukeys, inv = torch.unique(r * N + c, return_inverse=True)
    nu = ukeys.numel()
    uval = torch.zeros((nb, nu), dtype=dtype, device=dev).index_add(1, inv, a_val)
    gp, gi = g_ptr.to(torch.int64), g_idx.to(torch.int64)
    lens = gp[1:] - gp[:-1]
    gl_val = torch.zeros((nb, gi.numel()), dtype=dtype, device=dev)
    w_val = torch.zeros((nb, gi.numel()), dtype=dtype, device=dev)
    nfail = torch.zeros((nb,), dtype=torch.int64, device=dev)
    zero, one = torch.zeros((), dtype=dtype, device=dev), torch.ones((), dtype=dtype, device=dev)
    for m in torch.unique(lens).tolist():
        rows_m = torch.nonzero(lens == m).reshape(-1)
        am = torch.arange(m, dtype=torch.int64, device=dev)
        e = torch.zeros((m, 1), dtype=dtype, device=dev)
        e[-1] = 1
        chunk = max(1, _CHUNK_ELEMS // (m * m * nb))
        for s in range(0, rows_m.numel(), chunk):
            slot = gp[rows_m[s:s + chunk]][:, None] + am                         # (nr, m) positions in the factors
            S = gi[slot]
            Q = S[:, :, None] * N + S[:, None, :]                                # key of A[S_r, S_c]
            if nu:
                p = torch.searchsorted(ukeys, Q.reshape(-1)).clamp_(max=nu - 1).reshape(Q.shape)
                blk = torch.where(ukeys[p] == Q, uval[:, p], zero)
            else:
                blk = torch.zeros((nb, *Q.shape), dtype=dtype, device=dev)
            aii = blk[..., m - 1, m - 1]
            # a block with a non-finite entry is decided here (its pivots or its solutions are not finite either way):
            # the library factorisation is not asked to work on NaN
            sick = ~torch.isfinite(blk).all(-1).all(-1)
            work = torch.where(sick[..., None, None], torch.eye(m, dtype=dtype, device=dev), blk)
            LU, piv, info = torch.linalg.lu_factor_ex(work)
            dg = torch.diagonal(LU, dim1=-2, dim2=-1)
            bad = sick | (info != 0) | (dg == 0).any(-1) | ~torch.isfinite(dg).all(-1)
            safe = torch.where(bad[..., None, None], torch.eye(m, dtype=dtype, device=dev), LU)
            spiv = torch.where(bad[..., None], (am + 1).to(piv.dtype), piv)
            eb = e.expand(nb, S.shape[0], m, 1)
            u = torch.linalg.lu_solve(safe, spiv, eb).squeeze(-1)
            g = torch.linalg.lu_solve(safe, spiv, eb, adjoint=True).squeeze(-1)  # A^H x = e_m: x = conj(g)
            g = g.conj()
            gm = g[..., m - 1]
            bad = bad | ~torch.isfinite(u).all(-1) | ~torch.isfinite(g).all(-1) | (gm == 0)
            gl = g / torch.where(bad, one, gm)[..., None]
            gl[..., m - 1] = 1
            ok_d = (aii != 0) & torch.isfinite(aii)
            unit = torch.zeros_like(gl)
            unit[..., m - 1] = 1
            wfb = unit * (1 / torch.where(ok_d, aii, one)).conj()[..., None]
            gl_val[:, slot] = torch.where(bad[..., None], unit, gl).resolve_conj()
            w_val[:, slot] = torch.where(bad[..., None], wfb, u.conj()).resolve_conj()
            nfail += bad.sum(1)
    return gl_val, w_val, nfail
