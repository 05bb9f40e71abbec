"""Thin typed wrappers over the C ABI (one Python function per entry point).

All tensors are device tensors; "panel" arguments are PANEL-MAJOR: shape
(B, P, N) with unit stride along N (the reference's Fortran-order (B, N, P)
view, xitorch/_utils/tensor.py:21-32, seen as its transpose).
"""
import os
import torch
from xitorch_amd import _capi
from xitorch_amd._capi import ptr, stream_ptr, check, suffix, fn, call, require_device
from ctypes import c_void_p as c_void_p_

__all__ = ["dense_mm"]


def _panel_strides(X):
    # X: (B, P, N) with stride(-1) == 1
    if X.dim() != 3 or (X.shape[-1] > 1 and X.stride(-1) != 1):
        raise _capi.NativeLibraryError("panel must be (B, P, N) with unit stride along N, got shape %s stride %s"
                                       % (tuple(X.shape), X.stride()))
    return X.stride(1), X.stride(0)


def _op_strides(A):
    """(lda, sA) of an operator (M, N) or (B or 1, M, N): row pitch and batch pitch (0 broadcasts the one operator)"""
    if A.dim() == 2:
        return A.stride(0), 0
    return A.stride(1), (A.stride(0) if A.shape[0] != 1 else 0)


def _esize(dtype):
    """element size in bytes the real-panel entry points are told"""
    return 8 if dtype == torch.float64 else 4


_ws_cache = {}


def _workspace(nelem, dtype, device):
    # one scratch buffer per (dtype, device, stream): launches on different streams may run concurrently
    key = (dtype, device, torch.cuda.current_stream().cuda_stream)
    w = _ws_cache.get(key)
    if w is None or w.numel() < nelem:
        # geometric growth: the Rayleigh-Ritz workspace of an un-restarted run grows with every iteration, and each
        # new size would be a fresh hipMalloc (milliseconds, and a device-wide stall) in a process that has not cached it
        grown = 0 if w is None else w.numel() + w.numel() // 2
        w = None
        _ws_cache.pop(key, None)
        w = torch.empty(max(nelem, grown, 1), dtype=dtype, device=device)
        _ws_cache[key] = w
    return w


def dense_mm(A, X, out=None, trans=False, rows_hint=0, stagger=1, wide=True):
    """Y[b,c,:] = A[b] @ X[b,c,:]  (trans=False)   or   A[b]^T @ X[b,c,:]  (trans=True).

    A: (B, M, N) or (M, N) (broadcast over the panel batch), unit stride along N.
    X: (B, P, N) (trans=False) / (B, P, M) (trans=True), panel-major.
    Returns Y: (B, P, M) / (B, P, N), panel-major.
    Replaces torch.matmul in MatrixLinearOperator._mm/_rmm (xitorch/_core/linop.py:695-702).
    """
    require_device(A, "operator matrix")
    require_device(X, "panel")
    if A.dtype != X.dtype:
        raise _capi.NativeLibraryError("dtype mismatch %s vs %s" % (A.dtype, X.dtype))
    B, P = X.shape[0], X.shape[1]
    if A.dim() == 3 and A.shape[0] != B and A.shape[0] != 1:
        raise _capi.NativeLibraryError("operator batch %d does not match panel batch %d" % (A.shape[0], B))
    M, N = A.shape[-2], A.shape[-1]
    lda, sA = _op_strides(A)
    if N > 1 and A.stride(-1) != 1:
        raise _capi.NativeLibraryError("operator matrix must have unit stride along its last dim")
    nin, nout = (M, N) if trans else (N, M)
    if X.shape[2] != nin:
        raise _capi.NativeLibraryError("panel length %d != operator dim %d" % (X.shape[2], nin))
    ldx, sX = _panel_strides(X)
    if out is None:
        out = torch.empty((B, P, nout), dtype=X.dtype, device=X.device)
    ldy, sY = _panel_strides(out)
    if not trans and wide and P >= WIDE_MIN_P and _rows_wide_ok(A, X, N, lda, sA, ldx, sX):
        # many columns in the ROW orientation: 64-row sub-tiles turned through LDS, 32 columns per pass (K1wr)
        return dense_rows_wide(A, X, out=out)
    if trans and wide and P >= WIDE_MIN_P and _wide_ok(A, N, lda, sA):
        # many columns: one MFMA pass per 32 columns instead of one VALU pass per 8/16
        for c0 in range(0, P, 32):
            pc = min(32, P - c0)
            dense_wide(A, X[:, c0:c0 + pc], out=out[:, c0:c0 + pc])
        return out
    ws, ws_n = None, 0
    ws_n = fn("xk_dense_mm_workspace_elems")(B, M, N, P, 1 if trans else 0)
    if ws_n > 0:
        ws = _workspace(ws_n, X.dtype, X.device)
    call("xk_dense_mm", X.dtype, ptr(A), ptr(X), ptr(out), ptr(ws), ws_n, B, M, N, P, lda, sA, ldx, sX, ldy, sY,
         1 if trans else 0, rows_hint, stagger)
    return out


# --------------------------------------------------------------------------- basis kernels
def _cstrides(C, a_dim, c_dim):
    """(batch, a, c) strides of a 3-D coefficient tensor whose `a` index is dim a_dim and `c` index dim c_dim."""
    return C.stride(0), C.stride(a_dim), C.stride(c_dim)


def lincomb(V, C, out, k, P, coef_layout="ac", alpha=1.0, beta=0.0):
    """out[b,c,:] = beta*out[b,c,:] + alpha * sum_{a<k} C[b,a,c] * V[b,a,:]

    V: (B, >=k, Npad) panel-major padded basis; out: (B, >=P, Npad) panel-major.
    C: 3-D coefficients; coef_layout "ac" means C[b,a,c], "ca" means C[b,c,a] (e.g. a Gram block
    straight out of dense_mm).  Replaces the Ritz rotations `V @ Y` (symeig.py:178,181) and the
    projections of the block Gram-Schmidt step that stands in for tallqr (_utils/tensor.py:15-18).
    """
    require_device(V, "basis")
    B, N = V.shape[0], V.shape[2]
    ldv, sV = V.stride(1), V.stride(0)
    ldo, sO = out.stride(1), out.stride(0)
    if coef_layout == "ac":
        sC, sCa, sCc = _cstrides(C, 1, 2)
    else:
        sC, sCa, sCc = _cstrides(C, 2, 1)
    call("xk_lincomb", V.dtype, ptr(V), ptr(C), ptr(out), B, k, N, P, ldv, sV, sC, sCa, sCc, ldo, sO, float(alpha),
         float(beta))
    return out


def _cplx_vec(dtype):
    """complex elements per 16 B vector"""
    return 1 if dtype == torch.complex128 else 2


def lincomb_c(V, C, out, k, P, alpha=1.0, beta=0.0, N=None):
    """out[b,c,:] = beta*out[b,c,:] + alpha * sum_{a<k} C[b,c,a] * V[b,a,:] for COMPLEX panels (xk_lincomb_c128/_c64):
    V (B, >=k, ld), out (B, >=P, ld) panel-major, C (B, >=P, >=k) with unit stride over a (the "ca" layout of
    `lincomb`), alpha / beta real; N: vector length (default: the whole pitch V.shape[2]).  The projections and the
    iterate x = Q y of the complex GMRES."""
    require_device(V, "basis")
    _require_resolved("lincomb_c", V, C, out)
    if V.dtype != out.dtype or C.dtype != V.dtype or not V.is_complex():
        raise _capi.NativeLibraryError("lincomb_c: complex V, C, out of one dtype expected")
    if V.stride(2) != 1 or out.stride(2) != 1 or (k > 1 and C.stride(2) != 1):
        raise _capi.NativeLibraryError("lincomb_c: unit stride along the vector / coefficient axis expected")
    B = V.shape[0]
    N = V.shape[2] if N is None else N
    call("xk_lincomb", V.dtype, ptr(V), ptr(C), ptr(out), B, k, N, P, V.stride(1), V.stride(0), C.stride(0),
         C.stride(1), out.stride(1), out.stride(0), float(alpha), float(beta), what="xk_lincomb_c")
    return out


def gmres_gram_tiles(N, dtype):
    """number of fixed reduction tiles (1024 16 B vectors each) xk_gmres_gram_c* cuts a length-N complex vector into"""
    tile = 1024 * _cplx_vec(dtype)
    return (N + tile - 1) // tile


def gmres_gram_c(Q, w, c, scratch, kq, N):
    """c[s, i] = <Q[s, i], w[s]> = sum conj(Q) w for i < kq, c[s, kq] = |w_s|^2 + 0i  (xk_gmres_gram_c128/_c64).
    Q (S, >=kq, ld), w (S, ld) (may be a row view of Q), c (S, >=kq+1) complex; scratch: float64, at least
    S * gmres_gram_tiles(N) * (kq + 1) * 2 elements.  Fixed-shape reduction: repeated calls are bit-identical."""
    require_device(Q, "basis")
    _require_resolved("gmres_gram_c", Q, w, c)
    S = Q.shape[0]
    nblk = gmres_gram_tiles(N, Q.dtype)
    if w.dtype != Q.dtype or c.dtype != Q.dtype or not Q.is_complex() or scratch.dtype != torch.float64:
        raise _capi.NativeLibraryError("gmres_gram_c: complex Q, w, c of one dtype and a float64 scratch expected")
    if Q.stride(2) != 1 or w.stride(1) != 1 or c.stride(1) != 1 or c.shape[1] < kq + 1 or Q.shape[1] < kq:
        raise _capi.NativeLibraryError("gmres_gram_c: bad layout")
    if scratch.numel() < S * nblk * (kq + 1) * 2:
        raise _capi.NativeLibraryError("gmres_gram_c: scratch holds %d doubles, %d needed"
                                       % (scratch.numel(), S * nblk * (kq + 1) * 2))
    call("xk_gmres_gram", Q.dtype, ptr(Q), ptr(w), ptr(c), ptr(scratch), S, N, kq, Q.stride(1), Q.stride(0),
         w.stride(0), c.stride(0), nblk)
    return c


def group_status(rmax, info, flag, status, orth=None):
    """status (3 doubles on the device) = {max rmax (NaN-propagating), max info, max flag or 0}: one launch instead of
    three reductions and three converting copies (the host reads it once per Davidson step, symeig.py:190-197).
    orth (B,), optional: the guard values of `ritz_guard`; status[4] = their maximum (status needs 5 doubles), orth is
    re-zeroed."""
    if orth is not None and status.numel() < 5:
        raise _capi.NativeLibraryError("group_status: status needs 5 doubles when orth is given")
    call("xk_group_status", rmax.dtype, ptr(rmax), ptr(info), ptr(flag) if flag is not None else None,
         ptr(orth) if orth is not None else None, ptr(status), rmax.shape[0])


def ritz_guard(X, orth, P, N, MX=None):
    """orth[b] = max(orth[b], max_{c,d} |<X_c, (M X)_d> - delta_cd|) over the first P rows of the panel-major Ritz
    block X (B, >=P, ld) (MX: the panel M X, default X itself).  The a-posteriori check of a Rayleigh-Ritz block: the
    reference's eigenvectors are orthonormal by construction (whole-basis CholeskyQR every iteration,
    _utils/tensor.py:8-19, symeig.py:207-223); here a block that is not is rolled back by the driver."""
    require_device(X, "Ritz block")
    B = X.shape[0]
    M_ = MX if MX is not None else X
    gs = _guard_scratch(B, P, X.dtype, X.device) if P > 8 else None
    ws, nws = (None, 0)
    if P > 8:
        nws = fn("xk_dense_mm_workspace_elems")(B, P, N, P, 0)
        ws = _workspace(max(nws, 1), X.dtype, X.device)
    call("xk_ritz_guard", X.dtype, ptr(X), ptr(M_), ptr(orth), B, N, P, X.stride(1), X.stride(0), M_.stride(1),
         M_.stride(0), ptr(gs), (gs.numel() if gs is not None else 0), ptr(ws), nws)


_gs_cache = {}


def _guard_scratch(B, P, dtype, device):
    key = (dtype, device, torch.cuda.current_stream().cuda_stream)
    g = _gs_cache.get(key)
    if g is None or g.numel() < B * P * P:
        g = _gs_cache[key] = torch.empty(B * P * P, dtype=dtype, device=device)
    return g


def _check_ritz_shapes(V, AV, Y, lam, X, Tn, k, P):
    """the kernels take raw pointers: a coefficient block narrower than P would be read past its end"""
    B = V.shape[0]
    if Y.dim() != 3 or Y.shape[0] != B or Y.shape[1] < k or Y.shape[2] < P or lam.shape[0] != B or lam.shape[-1] < P:
        raise _capi.NativeLibraryError("ritz_residual: Y must be (B, >=k, >=P) and lam (B, >=P); got %s / %s for "
                                       "k = %d, P = %d" % (tuple(Y.shape), tuple(lam.shape), k, P))
    if V.shape[1] < k or AV.shape[1] < k or X.shape[1] < P or Tn.shape[1] < P:
        raise _capi.NativeLibraryError("ritz_residual: basis / output panels are smaller than (k, P) = (%d, %d)" % (k, P))


def ritz_residual(V, AV, Y, lam, X, Tn, rmax, k, P):
    """Fused K4/K5 (symeig.py:178-188): X = Y^T V, AX = Y^T AV, Tn = -(AX - lam X), rmax[b] = max|AX - lam X|.

    Y: (B, k, >=P) eigenvector coefficients (any strides), lam: (B, >=P) with unit stride along P,
    rmax: (B,) zero-initialised by the caller.
    """
    B, N = V.shape[0], V.shape[2]
    if lam.stride(-1) != 1 and P > 1:
        raise _capi.NativeLibraryError("lam must have unit stride along its last dim")
    _check_ritz_shapes(V, AV, Y, lam, X, Tn, k, P)
    call("xk_ritz_residual", V.dtype, ptr(V), ptr(AV), ptr(Y), ptr(lam), ptr(X), ptr(Tn), ptr(rmax), B, k, N, P,
         V.stride(1), V.stride(0), AV.stride(1), AV.stride(0), Y.stride(0), Y.stride(1), Y.stride(2), lam.stride(0),
         X.stride(1), X.stride(0), Tn.stride(1), Tn.stride(0))


def diag_precond(Tn, d, lam, P, m=None, floor=None):
    """Davidson's diagonal correction in place: Tn[b,c,:] /= (d[b,:] - lam[b,c] * m[b,:]) with the magnitude of
    the denominator kept above ``floor`` (extension: the reference's davidson takes t = -resid, symeig.py:206-207).
    Tn: (B, >=P, ld) panel, d / m: (B or 1, N), lam: (B, >=P)."""
    B, N = Tn.shape[0], d.shape[-1]
    if floor is None:
        floor = float(torch.finfo(Tn.dtype).eps) ** 0.5
    d2 = d.reshape(-1, N)
    m2 = m.reshape(-1, N) if m is not None else None
    for t in (d2, m2):
        if t is not None and (t.stride(-1) != 1 or t.dtype != Tn.dtype or t.shape[0] not in (1, B)):
            raise _capi.NativeLibraryError("diag_precond: diagonals must be (B or 1, N), unit stride, dtype of the panel")
    sD = d2.stride(0) if d2.shape[0] == B and B > 1 else (0 if d2.shape[0] == 1 else d2.stride(0))
    sM = 0 if m2 is None or m2.shape[0] == 1 else m2.stride(0)
    call("xk_diag_precond", Tn.dtype, ptr(Tn), ptr(d2), ptr(m2) if m2 is not None else None, ptr(lam), B, N, P,
         Tn.stride(1), Tn.stride(0), sD, sM, lam.stride(0), float(floor))


def panel_chol(G, W, info, P):
    """W[b] = R^-1 with G[b] = R^T R (upper R); info[b] != 0 flags a non-positive pivot.
    G: (B, >=P, >=P) with unit stride along its last dim.  CholeskyQR step of tallqr (tensor.py:16-17)."""
    B = G.shape[0]
    call("xk_panel_chol", G.dtype, ptr(G), ptr(W), ptr(info), B, P, G.stride(1), G.stride(0))


def panel_transform(Tp, W, P):
    """In place Tp[b,c,:] <- sum_{a<=c} W[b,a,c] Tp[b,a,:]  (tensor.py:18, Q = V R^-1 for the new panel only)."""
    B, N = Tp.shape[0], Tp.shape[2]
    call("xk_panel_transform", Tp.dtype, ptr(Tp), ptr(W), B, P, N, Tp.stride(1), Tp.stride(0))


# --------------------------------------------------------------------------- Davidson chain (one C call per stage)
def davidson_ritz(V, AV, Y, lam, X, Tn, rmax, info, flag, status, k, P, cond=None, orth=None):
    """ritz_residual + (guard of the Ritz block) + group status in one C call (xk_davidson_ritz): X = Y^T V,
    Tn = -(Y^T AV - lam X), status = {max|resid| (NaN-propagating), max info, max flag[, max cond[, max orth]]}; rmax
    (and cond, orth) are left zeroed for the next step (symeig.py:178-197).  orth (B,): switches the a-posteriori guard
    on (see `ritz_guard`)."""
    B, N = V.shape[0], V.shape[2]
    if lam.stride(-1) != 1 and P > 1:
        raise _capi.NativeLibraryError("lam must have unit stride along its last dim")
    _check_ritz_shapes(V, AV, Y, lam, X, Tn, k, P)
    gs, ws, nws = None, None, 0
    if orth is not None:
        if status.numel() < 5:
            raise _capi.NativeLibraryError("davidson_ritz: status needs 5 doubles when orth is given")
        if P > 8:
            gs = _guard_scratch(B, P, V.dtype, V.device)
            nws = fn("xk_dense_mm_workspace_elems")(B, P, N, P, 0)
            ws = _workspace(max(nws, 1), V.dtype, V.device)
    call("xk_davidson_ritz", V.dtype, ptr(V), ptr(AV), ptr(Y), ptr(lam), ptr(X), ptr(Tn), ptr(rmax), ptr(info),
         ptr(flag) if flag is not None else None, ptr(cond) if cond is not None else None,
         ptr(orth) if orth is not None else None, ptr(status), B, k, N, P, V.stride(1), V.stride(0), AV.stride(1),
         AV.stride(0), Y.stride(0), Y.stride(1), Y.stride(2), lam.stride(0), X.stride(1), X.stride(0), Tn.stride(1),
         Tn.stride(0), ptr(gs), (gs.numel() if gs is not None else 0), ptr(ws), nws)


def davidson_ws(B, cap, N, q, dtype, device):
    """split-contraction workspace of the Gram products inside xk_davidson_orth / _extend_t for bases up to `cap`"""
    nws = fn("xk_dense_mm_workspace_elems")(B, cap, N, q, 0)
    return _workspace(max(nws, 1), dtype, device), nws


def davidson_orth(V, N, k0, q, C, W, info, passes=2, cond=None):
    """Rows [k0, k0+q) of the basis V (B, cap, ld) are orthogonalised against rows [0, k0) (`passes` rounds of block
    Gram-Schmidt) and orthonormalised among themselves (CholeskyQR) — tallqr of [V, t] restricted to the new block
    (_utils/tensor.py:8-19, symeig.py:207-220) — in one C call.  C: scratch of >= B*q*max(k0,q) elements, W: B*q*q.
    passes >= 2: [projection, CholeskyQR] per pass, the first CholeskyQR shifted.  cond (B,), optional, q <= 8: receives
    max(cond, squared pivot ratio of the raw panel)."""
    B = V.shape[0]
    ws, nws = davidson_ws(B, V.shape[1], N, q, V.dtype, V.device)
    call("xk_davidson_orth", V.dtype, ptr(V), B, N, k0, q, V.stride(1), V.stride(0), ptr(C), ptr(W), ptr(info),
         ptr(cond) if cond is not None else None, ptr(ws), nws, int(passes))


def davidson_extend_t(V, AV, Tm, Tn, N, k0, q):
    """T[:, k0:k0+q, :k0+q] = <V_a, (AV)_{k0+c}> and the mirrored block T[:, :k0, k0:k0+q] (symeig.py:170 restricted to
    the new rows / columns) in one C call.  Tn: scratch of >= B*q*(k0+q) elements."""
    B = V.shape[0]
    ws, nws = davidson_ws(B, V.shape[1], N, q, V.dtype, V.device)
    call("xk_davidson_extend_t", V.dtype, ptr(V), ptr(AV), ptr(Tm), ptr(Tn), B, N, k0, q, V.stride(1), V.stride(0),
         AV.stride(1), AV.stride(0), Tm.stride(1), Tm.stride(0), ptr(ws), nws)


# --------------------------------------------------------------------------- K3 small eigensolver
SMALL_EIGH_MAX_K = 128
SMALL_EIGH_MAX_P = 16


SMALL_EIGH_TRI_MIN_K = 16        # below this order the Jacobi kernel's fixed costs are lower


def small_eigh_tri_ok(k, p, dtype):
    """does the tridiagonalisation kernel (K3t) serve order k with p wanted pairs?  (LDS-resident: <= 160 KiB)"""
    if k > SMALL_EIGH_MAX_K or p > SMALL_EIGH_MAX_P or p > k:
        return False
    return fn("xk_small_eigh_tri_lds_bytes")(k, p, _esize(dtype)) <= 160 * 1024


SMALL_EIGH_BIG_MAX_K = 1536          # (r06: was 1024; fp64 beyond 614 and fp32 where the band does not fit: one launch per
                                     #  Householder step, 24 column slots per lane beyond order 1024)
SMALL_EIGH_BIG_MAX_P = 256          # (r06: was 64)
# launch shape of K3g's step kernels handed to every call (0 = the library's measured defaults).  Module attributes of
# the PYTHON layer, for measurement scripts; the C ABI itself has no state
K3G_WG = 0
K3G_THREADS = 0
K3G_ALGO = int(os.environ.get("XITORCH_K3G_ALGO", "0"))   # (the environment variable is a measurement knob)
                      # 0: the library's choice; -1: the r05 choice; 1: one launch per Householder step; 2: two-stage (band + bulge chasing);
                      # 3: persistent register-resident kernel (r06; step launches first beyond order 256 / 384)


def small_eigh_big_ok(k, p, dtype):
    """does the global-memory tridiagonalisation kernel (K3g) serve order k with p wanted pairs?"""
    if k < 8 or k > SMALL_EIGH_BIG_MAX_K or p > SMALL_EIGH_BIG_MAX_P or p > k:
        return False
    return fn("xk_small_eigh_big_batch")(k, p, _esize(dtype)) > 0


def small_eigh_big(T, k, p, uppest=False, wg=None, threads=None, algo=None):
    """K3g: lowest / uppermost p eigenpairs of the symmetric (B, k, k) matrices T[:, :k, :k] (lower triangle read) for
    orders beyond the LDS-resident kernels (129 .. 1536) or more than 16 wanted pairs (p <= 256, k >= 8): lam (B, p) ascending, Y (B, p, k), failure flags (B,) int32
    (nonzero -> redo with the library).  Replaces torch.linalg.eigh + _take_eigpairs (symeig.py:174-175) on the large
    bases of an un-restarted run."""
    require_device(T, "projected matrix")
    B = T.shape[0]
    if T.stride(2) != 1:
        raise _capi.NativeLibraryError("T must have unit stride along its last dim")
    lam = torch.empty((B, p), dtype=T.dtype, device=T.device)
    Y = torch.empty((B, p, k), dtype=T.dtype, device=T.device)
    info = torch.empty((B,), dtype=torch.int32, device=T.device)
    wg = K3G_WG if wg is None else int(wg)
    threads = K3G_THREADS if threads is None else int(threads)
    nws = fn("xk_small_eigh_big_workspace_elems")(B, k, wg)
    ws = _workspace(nws, T.dtype, T.device)
    algo = K3G_ALGO if algo is None else int(algo)
    if algo < 0:
        # measurement knob: the r05 choice (two-stage from order 192 on where its band fits the LDS, else step launches)
        algo = 2 if k >= 192 and (k <= 614 or T.dtype == torch.float32) else 1
    call("xk_small_eigh_big", T.dtype, ptr(T), ptr(lam), ptr(Y), ptr(ws), nws, ptr(info), B, k, p, 1 if uppest else 0,
         T.stride(1), T.stride(0), wg, threads, algo)
    return lam, Y, info


def small_eigh(T, k, p, uppest=False, max_sweeps=16, method="jacobi", threads=0, profile=None, out=None):
    """Lowest / uppermost `p` eigenpairs of the symmetric (B, k, k) matrices T[:, :k, :k] (lower
    triangle is read).  Returns lam (B, p) ascending, Y (B, p, k) with Y[b, c] the c-th eigenvector, and an int32
    (B,) tensor: Jacobi sweeps (method "jacobi") or the failure flags of the self-check (method "tri": K3t,
    Householder tridiagonalisation + bisection + inverse iteration; nonzero -> redo that call with "jacobi").
    `out`: contiguous (lam, Y, aux) of those shapes to write into instead of fresh tensors.
    Native replacement of `torch.linalg.eigh` + `_take_eigpairs` (symeig.py:174-175)."""
    require_device(T, "projected matrix")
    B = T.shape[0]
    if T.stride(2) != 1:
        raise _capi.NativeLibraryError("T must have unit stride along its last dim")
    if out is None:
        lam = torch.empty((B, p), dtype=T.dtype, device=T.device)
        Y = torch.empty((B, p, k), dtype=T.dtype, device=T.device)
        aux = torch.empty((B,), dtype=torch.int32, device=T.device)
    else:
        lam, Y, aux = out
        for t, shape, dtype in ((lam, (B, p), T.dtype), (Y, (B, p, k), T.dtype), (aux, (B,), torch.int32)):
            if tuple(t.shape) != shape or t.dtype != dtype or t.device != T.device or not t.is_contiguous():
                raise _capi.NativeLibraryError("small_eigh: out tensor is %s %s on %s, expected contiguous %s %s on %s"
                                               % (tuple(t.shape), t.dtype, t.device, shape, dtype, T.device))
    if method == "tri":
        call("xk_small_eigh_tri", T.dtype, ptr(T), ptr(lam), ptr(Y), ptr(aux), B, k, p, 1 if uppest else 0, T.stride(1),
             T.stride(0), int(threads), ptr(profile))
        return lam, Y, aux
    nws = fn("xk_small_eigh_workspace_elems")(B, k, max_sweeps)
    ws = _workspace(nws, T.dtype, T.device)
    call("xk_small_eigh", T.dtype, ptr(T), ptr(lam), ptr(Y), ptr(ws), nws, ptr(aux), B, k, p, 1 if uppest else 0,
         max_sweeps, T.stride(1), T.stride(0))
    return lam, Y, aux


# --------------------------------------------------------------------------- banded operator
def _rows_disjoint(B, C, N, sB, ld):
    """do the B * C rows of N elements of a (B, C, N) output at batch stride sB and row pitch ld occupy distinct
    memory?  (either index may be the slower one; an index of extent 1 has no stride to speak of)"""
    dims = sorted((s, n) for s, n in ((sB, B), (ld, C)) if n > 1)
    span = N
    for s, n in dims:
        if s < span:
            return False
        span = (n - 1) * s + N
    return True


def banded_mm(band, X, out=None, trans=False):
    """Y[b,c,:] = A_b X[b,c,:] for DIA-stored banded operators: band (B or 1, 2*hb+1, N),
    band[b,d,i] = A_b[i, i+d-hb].  X, Y panel-major (B, C, N)."""
    require_device(band, "band")
    require_device(X, "panel")
    ldx, sX = _panel_strides(X)
    B, C, N = X.shape
    if band.dim() not in (2, 3) or band.shape[-1] != N or band.shape[-2] % 2 != 1:
        raise _capi.NativeLibraryError("band shape %s does not match panel length %d" % (tuple(band.shape), N))
    nd = band.shape[-2]
    # the entry point reinterprets the band pointer by the panel's type and strides it by the panel's batch
    if band.dtype != X.dtype or band.device != X.device:
        raise _capi.NativeLibraryError("banded_mm: band is %s on %s, panel %s on %s"
                                       % (band.dtype, band.device, X.dtype, X.device))
    nb = band.shape[0] if band.dim() == 3 else 1
    if nb != 1 and nb != B:
        raise _capi.NativeLibraryError("banded_mm: band batch %d does not match panel batch %d" % (nb, B))
    if not band.is_contiguous():
        raise _capi.NativeLibraryError("band must be contiguous")
    sBand = nd * N if nb > 1 else 0             # one operator (a batch of 1 included) is broadcast over the panel batch
    if out is None:
        out = torch.empty((B, C, N), dtype=X.dtype, device=X.device)
    elif out.shape != X.shape or out.dtype != X.dtype or out.device != X.device:
        raise _capi.NativeLibraryError("banded_mm: out is %s %s on %s, expected %s %s on %s"
                                       % (tuple(out.shape), out.dtype, out.device, (B, C, N), X.dtype, X.device))
    ldy, sY = _panel_strides(out)
    if out.numel() > 0 and not _rows_disjoint(B, C, N, sY, ldy):
        raise _capi.NativeLibraryError("banded_mm: rows of out overlap (shape %s, strides %s)"
                                       % (tuple(out.shape), out.stride()))
    call("xk_banded_mm", X.dtype, ptr(band), ptr(X), ptr(out), B, N, nd // 2, C, sBand, ldx, sX, ldy, sY,
         1 if trans else 0)
    return out


def banded_grad(U, W, nd, out=None, accumulate=False):
    """G[b,d,i] (+)= sum_c U[b,c,i] * W[b,c,i+d-hb]  — the DIA band gradient of the banded apply
    (y = A x: U = grad_y, W = x; y = A^T x: U = x, W = grad_y).  U, W panel-major (B, C, N); returns (B, nd, N)."""
    require_device(U, "panel")
    require_device(W, "panel")
    B, C, N = U.shape
    if W.shape != U.shape or U.dtype != W.dtype or nd % 2 != 1:
        raise _capi.NativeLibraryError("banded_grad: panels must agree (got %s / %s), nd odd" % (tuple(U.shape), tuple(W.shape)))
    ldu, sU = _panel_strides(U)
    ldw, sW = _panel_strides(W)
    if out is None:
        out = torch.empty((B, nd, N), dtype=U.dtype, device=U.device)
        accumulate = False
    if not out.is_contiguous():
        raise _capi.NativeLibraryError("banded_grad: output must be contiguous")
    call("xk_banded_grad", U.dtype, ptr(U), ptr(W), ptr(out), B, N, nd // 2, C, ldu, sU, ldw, sW, out.stride(0),
         1 if accumulate else 0)
    return out


# --------------------------------------------------------------------------- CSR sparse operator
def csr_mm(pat, values, X, out=None, trans=False):
    """Y[b,c,:] = A_b X[b,c,:] (trans: A_b^H X[b,c,:]) for a CSR operator whose pattern `pat` (linop._CsrPattern:
    int32 device index arrays and the row bins) is shared by the batch.  values (B or 1, nnz) contiguous rows,
    X panel-major (B, C, N) (trans: (B, C, M)); returns Y (B, C, M) (trans: (B, C, N)).  fp64 / fp32 / complex128 /
    complex64; complex tensors must be resolved (no lazy conjugation bit) — the adjoint's conjugation of the values
    is the kernel's conj_val flag, nothing is copied."""
    require_device(values, "values")
    require_device(X, "panel")
    if values.dtype != X.dtype:
        raise _capi.NativeLibraryError("dtype mismatch %s vs %s" % (values.dtype, X.dtype))
    cplx = X.is_complex()
    if cplx:
        _require_resolved("csr_mm", values, X, out)
    B, C, nin = X.shape
    v = pat.csc() if trans else pat.csr()
    if nin != v.n_in:
        raise _capi.NativeLibraryError("panel length %d != operator dim %d" % (nin, v.n_in))
    if values.dim() != 2 or values.shape[-1] != pat.nnz or values.shape[0] not in (1, B) or \
            (pat.nnz > 1 and values.stride(-1) != 1):
        raise _capi.NativeLibraryError("values must be (1 or %d, %d) with unit stride, got %s"
                                       % (B, pat.nnz, tuple(values.shape)))
    if values.device != X.device or v.ptr.device != X.device:
        raise _capi.NativeLibraryError("values, pattern and panel must share one device")
    sV = values.stride(0) if values.shape[0] != 1 else 0
    ldx, sX = _panel_strides(X)
    if out is None:
        out = torch.empty((B, C, v.n_out), dtype=X.dtype, device=X.device)
    if out.shape != (B, C, v.n_out):
        raise _capi.NativeLibraryError("output must be (%d, %d, %d), got %s" % (B, C, v.n_out, tuple(out.shape)))
    ldy, sY = _panel_strides(out)
    ws = v.scratch(B * min(C, 8) * v.nseg, X.dtype) if v.nseg else None
    call("xk_csr_mm", X.dtype, ptr(v.ptr), ptr(v.idx), ptr(v.perm), ptr(values), sV, ptr(v.rows), v.bin_off,
         ptr(v.seg_q), ptr(v.seg_off), v.nseg, ptr(ws), ptr(X), ptr(out), B, v.n_out, nin, C,
         ldx if C > 1 else max(ldx, nin), sX, ldy if C > 1 else max(ldy, v.n_out), sY,
         *(((1 if trans else 0),) if cplx else ()))
    return out


def _require_resolved(what, *tensors):
    for t in tensors:
        if t is not None and (t.is_conj() or t.is_neg()):
            raise _capi.NativeLibraryError("%s: complex tensors must be resolved (resolve_conj / resolve_neg) before "
                                           "they reach the kernel" % what)


def csr_sddmm(pat, U, W, out=None):
    """G[b,k] = sum_c U[b,c,row_k] conj(W[b,c,col_k])  — the values gradient of the CSR apply (y = A x: U = grad y,
    W = x; y = A^H x: U = x, W = grad y); for real dtypes the conjugation is void.  U (B, C, M), W (B, C, N)
    panel-major; returns G (B, nnz).  Batch dims the values do not have are folded into C by the caller, so the
    kernel sums them in its fixed order.  Complex tensors must be resolved."""
    require_device(U, "panel")
    require_device(W, "panel")
    if U.is_complex():
        _require_resolved("csr_sddmm", U, W, out)
    B, C, M = U.shape
    if W.dim() != 3 or W.shape[:2] != U.shape[:2] or U.dtype != W.dtype or M != pat.M or W.shape[2] != pat.N:
        raise _capi.NativeLibraryError("csr_sddmm: panels (B, C, %d) / (B, C, %d) expected, got %s / %s"
                                       % (pat.M, pat.N, tuple(U.shape), tuple(W.shape)))
    ldu, sU = _panel_strides(U)
    ldw, sW = _panel_strides(W)
    if out is None:
        out = torch.empty((B, pat.nnz), dtype=U.dtype, device=U.device)
    if out.shape != (B, pat.nnz) or (pat.nnz > 1 and out.stride(-1) != 1):
        raise _capi.NativeLibraryError("csr_sddmm: output must be (%d, %d) with unit stride" % (B, pat.nnz))
    call("xk_csr_sddmm", U.dtype, ptr(pat.row_of), ptr(pat.col), ptr(U), ptr(W), ptr(out), pat.nnz, B, M, pat.N, C,
         ldu if C > 1 else max(ldu, M), sU, ldw if C > 1 else max(ldw, pat.N), sW, out.stride(0))
    return out


def dense_outer(U, W, out=None, accumulate=False):
    """G[b,i,j] (+)= sum_c U[b,c,i] * W[b,c,j]  — the dense-operator gradient (outer product of two panels).
    U (B, C, M), W (B, C, N) panel-major; returns (B, M, N) row-major."""
    require_device(U, "panel")
    require_device(W, "panel")
    B, C, M = U.shape
    N = W.shape[2]
    if W.shape[0] != B or W.shape[1] != C or U.dtype != W.dtype:
        raise _capi.NativeLibraryError("dense_outer: panels must agree (got %s / %s)" % (tuple(U.shape), tuple(W.shape)))
    ldu, sU = _panel_strides(U)
    ldw, sW = _panel_strides(W)
    if out is None:
        out = torch.empty((B, M, N), dtype=U.dtype, device=U.device)
        accumulate = False
    if out.stride(2) != 1 and N > 1:
        raise _capi.NativeLibraryError("dense_outer: output must have unit stride along its last dim")
    call("xk_dense_outer", U.dtype, ptr(U), ptr(W), ptr(out), B, M, N, C, ldu, sU, ldw, sW, out.stride(1),
         out.stride(0), 1 if accumulate else 0)
    return out


# --------------------------------------------------------------------------- fused BLAS-1 of the Broyden driver
_vd_scratch = {}


def vec_dots(pairs, out=None):
    """out[i] = <a_i, b_i> for up to 4 pairs of equal-length contiguous device vectors, one streaming pass and a
    deterministic device-side fold.  Returns a float64 device tensor of len(pairs) entries — NO host sync; read it
    with a single `.tolist()` when the values are needed (rootsolver.py:100,113,286-290,375-380 take one sync each)."""
    a0 = pairs[0][0]
    require_device(a0, "vector")
    L = a0.numel()
    np_ = len(pairs)
    if not 1 <= np_ <= 4:
        raise _capi.NativeLibraryError("vec_dots takes 1..4 pairs")
    flat = []
    for (a, b) in pairs:
        if a.numel() != L or b.numel() != L or a.dtype != a0.dtype or b.dtype != a0.dtype or \
                not a.is_contiguous() or not b.is_contiguous():
            raise _capi.NativeLibraryError("vec_dots: vectors must be contiguous, of one length and dtype")
        flat += [a, b]
    while len(flat) < 8:
        flat.append(None)
    key = (a0.device, torch.cuda.current_stream().cuda_stream)
    scratch = _vd_scratch.get(key)
    nws = fn("xk_vec_dots_workspace_elems")()
    if scratch is None:
        scratch = torch.empty(nws, dtype=torch.float64, device=a0.device)
        _vd_scratch[key] = scratch
    if out is None:
        out = torch.empty(np_, dtype=torch.float64, device=a0.device)
    call("xk_vec_dots", a0.dtype, *[ptr(t) for t in flat], np_, L, ptr(scratch), nws, ptr(out))
    return out


def broyden_axpy(out, u0=None, g0=0.0, u1=None, g1=0.0, V=None, coef=None, scale=None, k=0, gamma=1.0):
    """out = g0*u0 + g1*u1 + gamma * sum_{n<k} coef[n]*scale[n] * V[n]   (flat length-L vectors; V (>=k, ldv) rows).
    The low-rank apply and the rank-1 update of the Broyden inverse-Jacobian model (_jacobian.py:112-119,172-182)."""
    require_device(out, "vector")
    L = out.numel()
    ldv = V.stride(-2) if (V is not None and k > 0) else 0
    call("xk_broyden_axpy", out.dtype, ptr(out), ptr(u0), float(g0), ptr(u1), float(g1), ptr(V) if k > 0 else ptr(None),
         ldv, ptr(coef) if k > 0 else ptr(None), ptr(scale), int(k), float(gamma), L)
    return out


# --------------------------------------------------------------------------- MINRES step kernels (xk_minres.hip)
def minres_state(S, device):
    """zeroed per-system scalar state of the MINRES kernels: (2 slots, S, xk_minres_state_len()) doubles"""
    return torch.zeros((2, S, fn("xk_minres_state_len")()), dtype=torch.float64, device=device)


def minres_init(y0, v, Pb, state, phi2, S, N, ld, nblk, k):
    """beta = sqrt(<b, y0>) from the xk_kry_dots partials Pb, v = y0 / beta, state slot k & 1, phi2 <- beta^2"""
    require_device(v, "vector")
    call("xk_minres_init", v.dtype, ptr(y0), ptr(v), ptr(Pb), ptr(state), ptr(phi2), S, N, ld, nblk, int(k))


def minres_lanczos(Av, r2, r1, Palpha, state, Pbeta, S, N, ld, nblk, k):
    """r1 <- Av - (alpha / beta) r2 - (beta / beta_old) r1 with alpha from the partials Palpha; Pbeta <- |r1|^2
    partials (None: not wanted).  The caller swaps the roles of r1 and r2 afterwards."""
    require_device(r1, "vector")
    call("xk_minres_lanczos", r1.dtype, ptr(Av), ptr(r2), ptr(r1), ptr(Palpha), ptr(state), ptr(Pbeta), S, N, ld, nblk,
         int(k))


def minres_update(v, y, w1, w2, x, Palpha, Pbeta, beta_is_dot, state, phi2, S, N, ld, nblk, k):
    """rotation k; w1 <- (v - epsln w1 - delta w2) / gamma; x += phi w1; v <- y / beta_new; state slot (k + 1) & 1;
    phi2 <- phibar^2.  beta_is_dot: Pbeta holds xk_kry_dots partials of <r2, P r2> instead of xk_minres_lanczos' own."""
    require_device(x, "vector")
    call("xk_minres_update", x.dtype, ptr(v), ptr(y), ptr(w1), ptr(w2), ptr(x), ptr(Palpha), ptr(Pbeta),
         1 if beta_is_dot else 0, ptr(state), ptr(phi2), S, N, ld, nblk, int(k))


# --------------------------------------------------------------------------- LSMR step kernels (xk_lsmr.hip)
def lsmr_state(S, device):
    """zeroed per-system scalar state of the LSMR kernels: (2 slots, S, xk_lsmr_state_len()) doubles"""
    return torch.zeros((2, S, fn("xk_lsmr_state_len")()), dtype=torch.float64, device=device)


def lsmr_init(b, uh, Pb, state, run, S, N, ld, nblk, k, raw=False):
    """beta_1 = sqrt(sum Pb) from the |b|^2 partials, uh <- b, start state in slot k & 1, run <- 1 / 0 (b = 0)"""
    require_device(uh, "vector")
    return call("xk_lsmr_init", uh.dtype, ptr(b), ptr(uh), ptr(Pb), ptr(state), ptr(run), S, N, ld, nblk, int(k),
                raw=raw)


def lsmr_bidiag(Op, y, Pin, Pout, state, half, S, N, ld, nblk, nblk_in, k, raw=False):
    """y <- Op / nu_x - (nu_x / nu_y) y: nu_x from the nblk_in partials Pin, nu_y from the state (half 0, the u half:
    beta; half 1, the v half: alpha); Pout <- the nblk partials of |y|^2"""
    require_device(y, "vector")
    return call("xk_lsmr_bidiag", y.dtype, ptr(Op), ptr(y), ptr(Pin), ptr(Pout), ptr(state), int(half), S, N, ld, nblk,
                nblk_in, int(k), raw=raw)


def lsmr_update(vh, h, hbar, x, Pu, Pv, Pxin, Pxout, state, run, S, N, ld, nblk, nblk_u, k, damp=0.0, atol=1e-6,
                btol=1e-6, conlim=1e8, raw=False):
    """step k of LSMR on the v side: the rotations, hbar, x and h in one pass, the estimates and the stop code into
    state slot (k + 1) & 1, run <- 1 / 0, Pxout <- partials of |x|^2"""
    require_device(x, "vector")
    return call("xk_lsmr_update", x.dtype, ptr(vh), ptr(h), ptr(hbar), ptr(x), ptr(Pu), ptr(Pv), ptr(Pxin), ptr(Pxout),
                ptr(state), ptr(run), S, N, ld, nblk, nblk_u, int(k), float(damp), float(atol), float(btol),
                float(conlim), raw=raw)


# --------------------------------------------------------------------------- Lanczos quadrature (xk_slq.hip)
SLQ_MAX_STEPS = 128                      # the projected matrix of xk_slq_quad lives on chip
SLQ_FN = {"log": 0, "inv": 1, "sqrt": 2, "invsqrt": 3, "exp": 4, "identity": 5}


def slq_state(S, device):
    """zeroed per-system scalar state of the quadrature kernels: (2 slots, S, xk_slq_state_len()) doubles"""
    return torch.zeros((2, S, fn("xk_slq_state_len")()), dtype=torch.float64, device=device)


def slq_init(z, r2, Pb, state, S, N, ld, nblk, k, raw=False):
    """beta_1 = sqrt(<z, z>) from the xk_kry_dots partials Pb, r2 <- z, the start state in slot k & 1"""
    require_device(r2, "vector")
    return call("xk_slq_init", r2.dtype, ptr(z), ptr(r2), ptr(Pb), ptr(state), S, N, ld, nblk, int(k), raw=raw)


def slq_step(W, r2, r1, Pa, Pin, Pout, state, Tal, Tbe, S, N, ld, nblk, nsteps, k, raw=False):
    """Lanczos step k on un-normalised vectors: alpha from the xk_kry_dots partials Pa of <r2, W>, beta from the
    partials Pin of the step before; r1 <- W / beta - (alpha / beta) r2 - (beta / oldb) r1, Pout <- |r1|^2 partials,
    alpha and beta into Tal, Tbe, state slot (k + 1) & 1.  The caller swaps r1 and r2, Pin and Pout."""
    require_device(r1, "vector")
    return call("xk_slq_step", r1.dtype, ptr(W), ptr(r2), ptr(r1), ptr(Pa), ptr(Pin), ptr(Pout), ptr(state), ptr(Tal),
                ptr(Tbe), S, N, ld, nblk, int(nsteps), int(k), raw=raw)


def slq_quad(Tal, Tbe, state, k, fn_code=0, param=0.0, raw=False):
    """Gauss quadrature of every system's Jacobi matrix (m and |z|^2 from state slot k & 1) ->
    (theta (S, nsteps), weight (S, nsteps), out (S,) = |z|^2 sum weight f(theta), flag (S,) int32).  fn_code: SLQ_FN."""
    require_device(Tal, "Lanczos coefficients")
    S, nsteps = Tal.shape
    theta, weight = torch.empty_like(Tal), torch.empty_like(Tal)
    out = torch.empty((S,), dtype=torch.float64, device=Tal.device)
    flag = torch.empty((S,), dtype=torch.int32, device=Tal.device)
    rc = call("xk_slq_quad", None, ptr(Tal), ptr(Tbe), ptr(state), ptr(theta), ptr(weight), ptr(out), ptr(flag), S,
              nsteps, int(k), int(fn_code), float(param), raw=raw)
    if raw:
        return rc
    return theta, weight, out, flag


# --------------------------------------------------------------------------- f(A) B by two-pass Lanczos (xk_fnm.hip)
def fnm_eig(Tal, Tbe, state, k, raw=False):
    """eigenvalues and the whole eigenvector matrix of every system's Jacobi matrix (m from state slot k & 1) ->
    (theta (S, nsteps), Qt (S, nsteps, nsteps) column-major: Qt[s, i] is the eigenvector of theta[s, i], flag (S,)
    int32: 2 where QL did not converge)"""
    require_device(Tal, "Lanczos coefficients")
    S, nsteps = Tal.shape
    theta = torch.empty_like(Tal)
    Qt = torch.empty((S, nsteps, nsteps), dtype=torch.float64, device=Tal.device)
    flag = torch.empty((S,), dtype=torch.int32, device=Tal.device)
    rc = call("xk_fnm_eig", None, ptr(Tal), ptr(Tbe), ptr(state), ptr(theta), ptr(Qt), ptr(flag), S, nsteps, int(k),
              raw=raw)
    if raw:
        return rc
    return theta, Qt, flag


def fnm_coeff(Qt, theta, state, flag, k, fn_code=-1, param=0.0, fvals=None, cplx=False, raw=False):
    """C[s, j] = |b_s| sum_i Qt[s, i, j] f_i Qt[s, i, 0] -> (C (S, nsteps) float64, or (S, nsteps, 2) (re, im) pairs
    with cplx; tail (S,)).  fn_code: SLQ_FN (bit 0 of `flag` is set for a node <= 0 under a positivity function), or -1
    with fvals (S, nsteps) float64 / (S, nsteps, 2) pairs: the function already applied to theta.  `flag` is updated
    in place."""
    require_device(Qt, "eigenvectors")
    S, nsteps = theta.shape
    if fvals is not None and (fvals.dtype != torch.float64 or not fvals.is_contiguous()
                              or tuple(fvals.shape) != ((S, nsteps, 2) if cplx else (S, nsteps))):
        raise _capi.NativeLibraryError("fnm_coeff: fvals must be contiguous float64 %s"
                                       % ("(S, nsteps, 2)" if cplx else "(S, nsteps)"))
    C = torch.empty((S, nsteps, 2) if cplx else (S, nsteps), dtype=torch.float64, device=Qt.device)
    tail = torch.empty((S,), dtype=torch.float64, device=Qt.device)
    rc = call("xk_fnm_coeff", None, ptr(Qt), ptr(theta), ptr(state), ptr(fvals), ptr(C), ptr(tail), ptr(flag), S,
              nsteps, int(k), int(fn_code), float(param), 1 if cplx else 0, raw=raw)
    if raw:
        return rc
    return C, tail


def fnm_step(W, r2, r1, X, C, Tal, Tbe, state, S, N, ld, nblk, nsteps, k, kstate, last=False, raw=False):
    """step k of pass 2: X += (C[:, k] / Tbe[:, k]) r2, then (unless last) r1 <- the Lanczos vector of step k + 1 from
    the recorded Tal, Tbe, bit for bit the one xk_slq_step wrote.  m and the flag come from state slot kstate & 1.
    W = None means last.  The caller swaps r1 and r2."""
    require_device(X, "vector")
    return call("xk_fnm_step", X.dtype, ptr(W), ptr(r2), ptr(r1), ptr(X), ptr(C), ptr(Tal), ptr(Tbe), ptr(state), S, N,
                ld, nblk, int(nsteps), int(k), int(kstate), 1 if last else 0, raw=raw)


# --------------------------------------------------------------------------- Chebyshev filter step (xk_cheb.hip)
def cheb_step(AY, Y, Yprev, coef, out=None, N=None, raw=False):
    """out[b,c,:N] = coef[b,0] * AY[b,c,:N] + coef[b,1] * Y[b,c,:N] + coef[b,2] * Yprev[b,c,:N]  (xk_cheb_step_*): the
    three-term step of a Chebyshev filter on (Bt, p, ld) panels of one dtype (real or complex), unit stride along the
    vector.  coef: (Bt, 3) float64 on the device, read by the kernel (no host synchronisation).  out: None = Yprev
    itself (the driver's ring: the oldest panel is overwritten), or a panel apart from it; never AY or Y.  Where
    coef[b,2] == 0 exactly, Yprev[b] is not read.  N: vector length (default: the panels' whole last dimension); only
    out[:, :, :N] is written.  raw=True returns the status code instead of raising (tests of the argument checks)."""
    if out is None:
        out = Yprev
    for t in (AY, Y, Yprev, out):
        require_device(t, "panel")
        if t.dim() != 3 or t.shape[:2] != AY.shape[:2] or t.dtype != AY.dtype or (t.shape[2] > 1 and t.stride(2) != 1):
            raise _capi.NativeLibraryError("cheb_step: panels must be (Bt, p, ld) of one dtype and shape, unit stride "
                                           "along the vector")
    if AY.is_complex():
        _require_resolved("cheb_step", AY, Y, Yprev, out)
    Bt, p = AY.shape[0], AY.shape[1]
    require_device(coef, "coefficients")
    if coef.dtype != torch.float64 or coef.shape != (Bt, 3) or not coef.is_contiguous():
        raise _capi.NativeLibraryError("cheb_step: coef must be a contiguous (Bt, 3) float64 tensor")
    if N is None:
        N = min(t.shape[2] for t in (AY, Y, Yprev, out))
    elif any(t.shape[2] < N for t in (AY, Y, Yprev, out)) and N > 0:
        raise _capi.NativeLibraryError("cheb_step: a panel is shorter than N = %d" % N)
    args = []
    for t in (AY, Y, Yprev, out):
        # (a one-vector panel / a one-member batch may carry any stride there)
        args += [ptr(t), t.stride(1) if (p > 1 or t.stride(1) >= t.shape[2]) else t.shape[2],
                 t.stride(0) if Bt > 1 else 0]
    rc = call("xk_cheb_step", AY.dtype, *args, ptr(coef), Bt, p, int(N), raw=raw)
    return rc if raw else out


def cheb_clenshaw(AY, Y, Yprev, X0, coef, out=None, N=None, raw=False):
    """out[b,c,:N] = ((coef[b,0] * AY + coef[b,1] * Y) + coef[b,2] * Yprev) + coef[b,3] * X0  (xk_cheb_clenshaw_*): the
    Clenshaw step of a Chebyshev band-pass filter on (Bt, p, ld) panels of one dtype (real or complex), unit stride
    along the vector.  coef: (Bt, 4) float64 on the device, read by the kernel (no host synchronisation).  out: None =
    Yprev itself (the driver's ring: the oldest panel is overwritten), or a panel apart from it; never AY, Y or X0.
    Where coef[b,2] == 0 exactly, Yprev[b] is not read.  N: vector length (default: the panels' whole last dimension);
    only out[:, :, :N] is written.  raw=True returns the status code instead of raising (tests of the argument
    checks)."""
    if out is None:
        out = Yprev
    panels = (AY, Y, Yprev, X0, out)
    for t in panels:
        require_device(t, "panel")
        if t.dim() != 3 or t.shape[:2] != AY.shape[:2] or t.dtype != AY.dtype or (t.shape[2] > 1 and t.stride(2) != 1):
            raise _capi.NativeLibraryError("cheb_clenshaw: panels must be (Bt, p, ld) of one dtype and shape, unit "
                                           "stride along the vector")
    if AY.is_complex():
        _require_resolved("cheb_clenshaw", *panels)
    Bt, p = AY.shape[0], AY.shape[1]
    require_device(coef, "coefficients")
    if coef.dtype != torch.float64 or coef.shape != (Bt, 4) or not coef.is_contiguous():
        raise _capi.NativeLibraryError("cheb_clenshaw: coef must be a contiguous (Bt, 4) float64 tensor")
    if N is None:
        N = min(t.shape[2] for t in panels)
    elif any(t.shape[2] < N for t in panels) and N > 0:
        raise _capi.NativeLibraryError("cheb_clenshaw: a panel is shorter than N = %d" % N)
    args = []
    for t in panels:
        # (a one-vector panel / a one-member batch may carry any stride there)
        args += [ptr(t), t.stride(1) if (p > 1 or t.stride(1) >= t.shape[2]) else t.shape[2],
                 t.stride(0) if Bt > 1 else 0]
    rc = call("xk_cheb_clenshaw", AY.dtype, *args, ptr(coef), Bt, p, int(N), raw=raw)
    return rc if raw else out


# --------------------------------------------------------------------------- LOBPCG rotation (xk_lobpcg.hip)
def lobpcg_max_rows():
    """largest order k of the Rayleigh-Ritz problem `lobpcg_rotate` accepts"""
    return int(fn("xk_lobpcg_max_rows")())


def lobpcg_blocks(N, dtype):
    """column chunks of `lobpcg_rotate` = length of the partial-sum axis of Pnorm / Pmax"""
    return int(fn("xk_lobpcg_blocks")(int(N), torch.empty((), dtype=dtype).element_size()))


def lobpcg_rotate(S, AS, MS, C, lam, k, q, w, N=None, Pnorm=None, Pmax=None, raw=False):
    """The in-place rotation of LOBPCG's stacks (xk_lobpcg_rotate_*).  S, AS, MS (None: no overlap operator):
    (Bt, rows >= q + w, ld) stacks of one dtype, unit stride along the vector.  For c < q every stack's row c becomes
    sum_{a<k} C[b,a,c] * row a (C (Bt, k, q) in the stacks' dtype, any strides, plain — not conjugated), and rows
    [q, q+w) of S receive the residual AS'_c - lam[b,c] * (MS'_c or S'_c).  lam: (Bt, >= w) float64 on the device, unit
    stride along c.  Returns (Pnorm (Bt, w, nblk), Pmax (Bt, nblk)) float64: the partial sums of |residual|^2 per column
    and the largest |residual| entry, per column chunk (nblk = lobpcg_blocks(N, dtype)).  N: vector length (default: the
    stacks' whole last dimension); nothing at n >= N is written.  raw=True returns the status code instead of raising
    (tests of the argument checks) and checks nothing itself."""
    stacks = (S, AS) if MS is None else (S, AS, MS)
    for t in stacks:
        require_device(t, "stack")
    if not raw:
        for t in stacks:
            if t.dim() != 3 or t.dtype != S.dtype or t.shape[0] != S.shape[0] or (t.shape[2] > 1 and t.stride(2) != 1):
                raise _capi.NativeLibraryError("lobpcg_rotate: stacks must be (Bt, rows, ld) of one dtype, unit stride "
                                               "along the vector")
            if t.shape[1] < q + w or t.shape[1] < k:
                raise _capi.NativeLibraryError("lobpcg_rotate: a stack has %d rows, k = %d and q + w = %d are needed"
                                               % (t.shape[1], k, q + w))
        if C.dtype != S.dtype or C.dim() != 3 or C.shape[0] != S.shape[0] or C.shape[1] < k or C.shape[2] < q:
            raise _capi.NativeLibraryError("lobpcg_rotate: C must be (Bt, >= k, >= q) in the stacks' dtype")
        if lam.dtype != torch.float64 or lam.dim() != 2 or lam.shape[1] < w or (lam.shape[1] > 1 and lam.stride(1) != 1):
            raise _capi.NativeLibraryError("lobpcg_rotate: lam must be (Bt, >= w) float64, unit stride along its last dim")
    _require_resolved("lobpcg_rotate", S, AS, MS, C)
    require_device(C, "coefficients")
    require_device(lam, "Ritz values")
    Bt = S.shape[0]
    if N is None:
        N = min(t.shape[2] for t in stacks)
    nblk = max(1, lobpcg_blocks(max(int(N), 1), S.dtype))
    if Pnorm is None:
        Pnorm = torch.empty((Bt, max(int(w), 1), nblk), dtype=torch.float64, device=S.device)
    if Pmax is None:
        Pmax = torch.empty((Bt, nblk), dtype=torch.float64, device=S.device)
    args = []
    for t in (S, AS, MS):
        args += [ptr(t), 0, 0] if t is None else [ptr(t), t.stride(1), t.stride(0)]
    rc = call("xk_lobpcg_rotate", S.dtype, *args, ptr(C), C.stride(0), C.stride(1), C.stride(2), ptr(lam),
              lam.stride(0), ptr(Pnorm), ptr(Pmax), Bt, int(N), int(k), int(q), int(w), raw=raw)
    return rc if raw else (Pnorm, Pmax)


# --------------------------------------------------------------------------- complex operators (real embedding)
def _as_real_matrix(A):
    """zero-copy real view (.., M, 2N) of a complex matrix (.., M, N): row i = (Re A_i0, Im A_i0, Re A_i1, ...)"""
    Ar = torch.view_as_real(A)
    return Ar.reshape(*A.shape[:-1], 2 * A.shape[-1])


def dense_mm_complex(A, X, adjoint=False, conj_io=False, out=None):
    """Complex operator-panel product on the REAL kernels (K1): the interleaved storage of A (B, M, N) complex is
    a real (B, M, 2N) matrix, and

        A x       : Re y = A~ . real(conj x),   Im y = A~ . real(i conj x)      -> xk_dense_mm(trans=0), 2P columns
        A^H x     : Z = A~^T [Re x; Im x];  Re y_j = Z[re, 2j] + Z[im, 2j+1],  Im y_j = Z[im, 2j] - Z[re, 2j+1]
                                                                                 -> xk_dense_mm(trans=1), 2P columns

    so the operator is streamed ONCE per product, exactly like the real case, and never copied or split.
    conj_io conjugates input and output (serves A^T x = conj(A^H conj x) and conj(A) x = conj(A conj x), i.e.
    transposed / conjugated *views* of the stored matrix).  X: (B, P, n_in) complex panel-major; returns
    (B, P, n_out) complex.  Replaces torch.matmul(mat, x) of MatrixLinearOperator for complex dtypes
    (xitorch/_core/linop.py:692-702; reference tests: _tests/test_linop_fcns.py:474-524)."""
    require_device(A, "operator matrix")
    require_device(X, "panel")
    if A.is_conj() or X.is_conj():
        raise _capi.NativeLibraryError("dense_mm_complex takes resolved tensors (conjugate views are expressed "
                                       "through adjoint/conj_io)")
    B, P = X.shape[0], X.shape[1]
    Ar = _as_real_matrix(A)
    M, N = A.shape[-2], A.shape[-1]
    rdtype = Ar.dtype
    if conj_io:
        X = X.conj().resolve_conj()
    if not adjoint:
        xc = X.conj().resolve_conj()
        U = torch.empty((B, 2 * P, 2 * N), dtype=rdtype, device=X.device)
        Uv = U.view(B, 2 * P, N, 2)
        Uv[:, :P, :, 0] = xc.real
        Uv[:, :P, :, 1] = xc.imag          # real(conj x)   = (xr, -xi)
        Uv[:, P:, :, 0] = X.imag
        Uv[:, P:, :, 1] = X.real           # real(i conj x) = (xi,  xr)
        Y = dense_mm(Ar, U, trans=False)                                  # (B, 2P, M)
        res = torch.complex(Y[:, :P], Y[:, P:])
    else:
        U = torch.cat([X.real, X.imag], dim=1).contiguous()                # (B, 2P, M)
        Z = dense_mm(Ar, U, trans=True).view(B, 2 * P, N, 2)               # (B, 2P, 2N)
        res = torch.complex(Z[:, :P, :, 0] + Z[:, P:, :, 1], Z[:, P:, :, 0] - Z[:, :P, :, 1])
    if conj_io:
        res = res.conj().resolve_conj()
    if out is not None:
        out.copy_(res)
        return out
    return res


def dense_outer_complex(U, W):
    """G[b,i,j] = sum_c U[b,c,i] conj(W[b,c,j])  (complex panels) through the real streaming kernel xk_dense_outer:
    in the interleaved storage G~[i, 2j] = sum Ur Wr + Ui Wi, G~[i, 2j+1] = sum Ui Wr - Ur Wi — a real outer product
    with 2C columns.  The operator gradient gy x^H of the complex dense apply."""
    B, C, M = U.shape
    N = W.shape[2]
    Ur = torch.cat([U.real, U.imag], dim=1).contiguous()                   # (B, 2C, M)
    Wr = torch.empty((B, 2 * C, 2 * N), dtype=Ur.dtype, device=U.device)
    Wv = Wr.view(B, 2 * C, N, 2)
    Wv[:, :C, :, 0] = W.real
    Wv[:, :C, :, 1] = -W.imag            # rows paired with Re U:  (Wr, -Wi)
    Wv[:, C:, :, 0] = W.imag
    Wv[:, C:, :, 1] = W.real             # rows paired with Im U:  (Wi,  Wr)
    G = dense_outer(Ur, Wr)                                                # (B, M, 2N) real
    return torch.view_as_complex(G.view(B, M, N, 2))


# --------------------------------------------------------------------------- Hermitian Davidson chain (complex)
HERM_EIGH_MAX_K = 128        # order of the Rayleigh-Ritz matrix xk_herm_eigh serves (both complex types)
HERM_EIGH_MAX_P = 16         # wanted pairs per call
HERM_CHOLQR_MAX_Q = 32       # block width of xk_herm_cholqr


def _real_view(t):
    """the interleaved (re, im) storage of a complex tensor as a real tensor (zero-copy)"""
    if t.is_conj():
        raise _capi.NativeLibraryError("Hermitian Davidson kernels take resolved tensors, got a conjugate view")
    return torch.view_as_real(t)


def _ld(t):
    """pitch between the vectors of a (B, q, N) panel (a one-vector panel may carry any stride there)"""
    return t.stride(1) if t.shape[1] > 1 else t.shape[2]


def herm_eigh_ok(k, p):
    return 1 <= p <= min(k, HERM_EIGH_MAX_P) and k <= HERM_EIGH_MAX_K


def herm_eigh(T, k, p, uppest=False):
    """Lowest / uppermost `p` eigenpairs of the Hermitian (B, k, k) complex matrices T[:, :k, :k] (lower triangle
    read): lam (B, p) real ascending, Y (B, p, k) complex with Y[b, c] the c-th eigenvector, flags (B,) int32
    (nonzero: the self-check failed, redo that member on the library).  The complex counterpart of `small_eigh(...,
    method="tri")`; replaces torch.linalg.eigh + _take_eigpairs (symeig.py:174-175) for complex bases."""
    require_device(T, "projected matrix")
    if not herm_eigh_ok(k, p):
        raise _capi.NativeLibraryError("herm_eigh serves k <= %d, p <= min(k, %d); got k = %d, p = %d"
                                       % (HERM_EIGH_MAX_K, HERM_EIGH_MAX_P, k, p))
    B = T.shape[0]
    if T.dim() != 3 or T.stride(2) != 1 or T.shape[1] < k or T.shape[2] < k:
        raise _capi.NativeLibraryError("T must be (B, >=k, >=k) with unit stride along its last dim")
    rdt = torch.float64 if T.dtype == torch.complex128 else torch.float32
    lam = torch.empty((B, p), dtype=rdt, device=T.device)
    Y = torch.empty((B, p, k), dtype=T.dtype, device=T.device)
    info = torch.empty((B,), dtype=torch.int32, device=T.device)
    nws = fn("xk_herm_eigh_workspace_elems")(B, k, p)
    ws = _workspace(max(nws, 1), rdt, T.device)
    call("xk_herm_eigh", T.dtype, ptr(_real_view(T)), ptr(lam), ptr(_real_view(Y)), ptr(info), ptr(ws), nws, B, k, p,
         1 if uppest else 0, T.stride(1), T.stride(0))
    return lam, Y, info


def herm_ritz(V, AV, Y, lam, X, Tn, status, k, p, MV=None):
    """Fused Ritz step of the complex driver (xk_herm_ritz): X[:, :p] = Y^T V[:, :k], Tn[:, :p] = -(Y^T AV - lam Y^T MV),
    status (B + 1 float64) = {max over the batch, max per member} of |R| (complex modulus).  V, AV, MV: (B, >=k, ld)
    panels; Y (B, >=k, >=p) complex (any strides), lam (B, >=p) real, unit stride along p (symeig.py:178-188)."""
    require_device(V, "basis")
    B, N = V.shape[0], V.shape[2]
    if Y.dim() != 3 or Y.shape[0] != B or Y.shape[1] < k or Y.shape[2] < p or lam.shape[0] != B or lam.shape[-1] < p:
        raise _capi.NativeLibraryError("herm_ritz: Y must be (B, >=k, >=p) and lam (B, >=p)")
    if lam.stride(-1) != 1 and p > 1:
        raise _capi.NativeLibraryError("lam must have unit stride along its last dim")
    for t, rows in ((V, k), (AV, k), (MV, k), (X, p), (Tn, p)):
        if t is not None and (t.dim() != 3 or t.shape[0] != B or t.shape[1] < rows or t.shape[2] != N or
                              t.stride(2) != 1 or t.dtype != V.dtype):
            raise _capi.NativeLibraryError("herm_ritz: panels must be (B, rows, N) of one dtype, unit stride along N")
    if status.numel() < B + 1 or status.dtype != torch.float64:
        raise _capi.NativeLibraryError("herm_ritz: status needs B + 1 float64 elements")
    M_ = MV if MV is not None else V
    call("xk_herm_ritz", V.dtype, ptr(_real_view(V)), ptr(_real_view(AV)),
         ptr(_real_view(MV)) if MV is not None else None, ptr(_real_view(Y)), ptr(lam), ptr(_real_view(X)),
         ptr(_real_view(Tn)), ptr(status), B, k, N, p, _ld(V), V.stride(0), _ld(AV), AV.stride(0), _ld(M_),
         M_.stride(0), Y.stride(0), Y.stride(1), Y.stride(2), lam.stride(0), _ld(X), X.stride(0), _ld(Tn), Tn.stride(0))


def herm_cholqr(W, info, MW=None, shift_rel=0.0):
    """CholeskyQR of the complex block W (B, q, N) in place, in the M-inner product when MW = M W is given (then MW is
    transformed alike): G = W^H MW, G + shift_rel trace(G) I = R^H R, W <- W R^-1.  info (B,) int32, sticky: index + 1
    of the first non-positive pivot.  tallqr of the new block (_utils/tensor.py:8-19)."""
    require_device(W, "block")
    B, q, N = W.shape
    if q > HERM_CHOLQR_MAX_Q:
        raise _capi.NativeLibraryError("herm_cholqr serves blocks of up to %d vectors, got %d" % (HERM_CHOLQR_MAX_Q, q))
    for t in (W, MW):
        if t is not None and (t.shape != W.shape or t.stride(2) != 1 or t.dtype != W.dtype):
            raise _capi.NativeLibraryError("herm_cholqr: blocks must be (B, q, N) of one dtype, unit stride along N")
    Rinv = torch.empty((B, q, q), dtype=W.dtype, device=W.device)
    call("xk_herm_cholqr", W.dtype, ptr(_real_view(W)), ptr(_real_view(MW)) if MW is not None else None,
         ptr(_real_view(Rinv)), ptr(info), B, q, N, _ld(W), W.stride(0), _ld(MW) if MW is not None else 0,
         MW.stride(0) if MW is not None else 0, float(shift_rel))
    return Rinv


# --------------------------------------------------------------------------- measurement utility
def stream_read(t):
    """Enqueue one read-only pass over the storage of the contiguous HIP tensor `t` (rows = its last dimension; the
    panel kernels' tile walk, 16 B/lane non-temporal loads, no arithmetic) on the current stream.  Timed by the
    caller: what this very buffer streams at when nothing is computed (bench.py ``roofline.stream_read``)."""
    if not t.is_cuda or not t.is_contiguous() or t.dim() < 1:
        raise _capi.NativeLibraryError("stream_read needs a contiguous HIP tensor")
    pitch = t.shape[-1] * t.element_size()
    if pitch % 16:
        raise _capi.NativeLibraryError("stream_read: the row length must be a multiple of 16 bytes")
    nbytes = t.numel() * t.element_size()
    call("xk_stream_read", None, ptr(t), nbytes, pitch, None)
    return nbytes


# --------------------------------------------------------------------------- CU-masked stream
_MASKED_STREAMS = {}
# which bits of the linear CU mask a masked stream gives up (include/xitorch_amd.h): 0 (shipped) = the last `reserve` bits,
# 1 = every (units / reserve)-th bit.  The driver deals the linear mask out over the 8 XCDs bit by bit (measured with
# xk_probe_xcc, profiles/r05_cu_mask_probe.jsonl): the tail pattern takes reserve / 8 units from EVERY XCD (32 reserved: 28
# of 32 left on each); the strided pattern would take them all from one XCD — and a mask that empties an XCD is not
# honoured at all (every unit stays usable: "strided 32 / 64" in profiles/r05_cu_mask_pattern.jsonl are runs WITHOUT a
# reservation: 208.0 ms per configs[1] call against 209.7 with the tail pattern, but 33.8 vs 30.8 ms at 8 operators,
# 59.4 vs 55.9 at 16, and 109.4 vs 105.6 for the configs[4] shard)
CU_MASK_PATTERN = int(os.environ.get("XITORCH_AMD_CU_MASK_PATTERN", "0"))


def masked_stream(device, reserve_cus=64, slot=0, only_reserved=False):
    """A process-lifetime HIP stream on `device` that leaves `reserve_cus` compute units unused
    (hipExtStreamCreateWithCUMask), wrapped as a torch stream.  The HBM-bound panel product runs at full
    speed on 192-224 CUs; the CUs it leaves free serve the latency-bound kernels of the other batch half.
    A stream with a CU mask owns its hardware queue, so `reserve_cus=0` streams (distinct `slot`s) are also how
    the two batch groups get queues that never share a barrier packet — torch's pooled streams are multiplexed
    onto a few hardware queues, and a group whose stream lands behind the other group's "wait for the panel
    product" barrier is serialised with it."""
    import ctypes
    device = torch.device(device)
    # only_reserved (r06): the complement — a stream that may use ONLY the `reserve_cus` units a plain masked stream leaves
    key = (device.index if device.index is not None else torch.cuda.current_device(), int(reserve_cus), int(slot),
           2 if only_reserved else int(CU_MASK_PATTERN))
    if key not in _MASKED_STREAMS:
        out = ctypes.c_void_p()
        rc = fn("xk_stream_create_cu_masked_pattern")(key[0], key[1], key[3], ctypes.byref(out))
        check(rc, "xk_stream_create_cu_masked")
        if not _MASKED_STREAMS:
            import atexit
            atexit.register(_destroy_masked_streams)
        _MASKED_STREAMS[key] = torch.cuda.ExternalStream(out.value, device=torch.device("cuda", key[0]))
        total = torch.cuda.get_device_properties(key[0]).multi_processor_count
        _STREAM_CUS[(key[0], out.value)] = max(1, key[1] if key[3] == 2 else total - key[1])
    return _MASKED_STREAMS[key]


_STREAM_CUS = {}             # (device index, stream handle) -> compute units the stream's mask leaves it


def stream_cus(stream):
    """compute units a stream may use: what its CU mask leaves (streams made by `masked_stream`), else all of them"""
    dev = stream.device.index if stream.device.index is not None else torch.cuda.current_device()
    n = _STREAM_CUS.get((dev, stream.cuda_stream))
    return n if n is not None else torch.cuda.get_device_properties(dev).multi_processor_count


def _destroy_masked_streams():
    """The streams live as long as the process; hand them back before the HIP runtime (and any profiler layered
    on it) tears down — rocprofv3 otherwise crashes at exit on streams it still tracks."""
    for key, st in list(_MASKED_STREAMS.items()):
        try:
            st.synchronize()
            fn("xk_stream_destroy")(c_void_p_(st.cuda_stream))
        except Exception:
            pass
    _MASKED_STREAMS.clear()


# --------------------------------------------------------------------------- K1s symmetric storage
K1S_OPTS = None       # None = the shipped choice per launch (`k1s_auto_opts`); an int = low 16 bits of the `opts` of the K1s
                      # entry points handed to every call (measurement scripts, tests; include/xitorch_amd.h)
K1S_PERSIST = 16      # opts bit 4: resident workgroups taking runs from a queue (two per compute unit of the stream)
K1S_WIDE8 = 32        # opts bit 5 (fp64): 8-wave workgroups on 2048 x 2048 tiles, one per compute unit


def k1s_auto_opts(B, N, dtype, cus, pipelined=False, lda=None):
    """The form of one K1s launch over B operators of order N on `cus` compute units (r05, profiles/r05_k1s_*):
      * resident launch (workgroups take runs from a queue) from two rounds of workgroups on — below that the launch is
        one wave of workgroups either way; inside the eigensolver's two-group pipeline this is what lets the other
        group's launch, on its own stream, move into the slots the tail frees (217.6 -> 211.9 ms per configs[1] call);
      * fp64: 8-wave workgroups on 2048 x 2048 tiles (half the partial-sum bytes written and folded) once the launch has
        enough of them: a tile is 32 MB, so alone on the GPU it needs ~8 per compute unit to beat the 4-wave form
        (64 x 16384^2: 10.91 vs 11.31 ms; 32 x 16384^2: 5.55 vs 5.45), inside the pipeline — tails overlapped — about 2
        (32 operators per launch: 216.7 -> 209.9 ms per call).  The 8-wave form addresses 2048 rows through one buffer
        descriptor: `lda` (elements; N when not given) must keep 2048 * lda * 8 bytes below 2 GiB (xk_symm.hip's
        launch check) — a wider operator keeps the 4-wave form, whose descriptor spans 1024 rows."""
    if B <= 0 or N <= 0:
        return 0
    f64 = dtype == torch.float64
    slab = 1024 if f64 else 2048
    ns = (N + slab - 1) // slab
    runs4 = B * sum(ns - (i * 1024) // slab for i in range((N + 1023) // 1024))
    # (inside the pipeline a launch of 8 operators of order 16384 — 1088 runs, 1.4 ms — is shorter than the other group's
    #  chain: nothing to overlap, the resident form costs 0.5 %; 16 operators: 112.0 -> 108.9 ms per call)
    o = K1S_PERSIST if runs4 >= (8 if pipelined else 4) * cus else 0
    if f64 and (o & K1S_PERSIST):
        n8 = (N + 2047) // 2048
        # (pipelined, 16 operators per launch = 576 tiles on 192-224 units: 108.8 -> 107.6 ms per call)
        fits = 2048 * int(N if lda is None else lda) * 8 <= 0x7fffffe0
        if fits and B * n8 * (n8 + 1) // 2 >= (2 if pipelined else 8) * cus:
            o |= K1S_WIDE8
    return o


def _k1s_opts(stream, opts=None, shape=None, pipelined=False, lda=None):
    """`opts` of one K1s launch on `stream`: the forced flag bits (argument or module) or the shipped choice for the
    launch's `shape` = (B, N, dtype), plus — for the resident form — the workgroup count (bits 16..27) that fills the
    compute units `stream` may use, two workgroups each."""
    o = K1S_OPTS if opts is None else int(opts)
    if o is None:
        o = k1s_auto_opts(shape[0], shape[1], shape[2], stream_cus(stream), pipelined, lda) if shape is not None else 0
    if (o & K1S_PERSIST) and not (o >> 16):
        o |= min(0xfff, 2 * stream_cus(stream)) << 16
    return o


def dense_symm(A, X, out=None, opts=None):
    """Y[b,c,:] = A_b X[b,c,:] for EXACTLY symmetric A (B or 1, N, N): only the upper triangle is read.
    The caller guarantees A == A^T bit for bit.  X, Y panel-major (B, P, N)."""
    require_device(A, "operator matrix")
    require_device(X, "panel")
    B, P, N = X.shape
    lda, sA = _op_strides(A)
    if A.shape[-1] != N or A.shape[-2] != N or (N > 1 and A.stride(-1) != 1):
        raise _capi.NativeLibraryError("symmetric operator must be (.., %d, %d) with unit stride" % (N, N))
    ldx, sX = _panel_strides(X)
    if out is None:
        out = torch.empty((B, P, N), dtype=X.dtype, device=X.device)
    ldy, sY = _panel_strides(out)
    nws = fn("xk_dense_symm_workspace_elems")(B, N, P, _esize(X.dtype))
    ws = _workspace(nws, X.dtype, X.device)
    call("xk_dense_symm", X.dtype, ptr(A), ptr(X), ptr(out), ptr(ws), nws, B, N, P, lda, sA, ldx, sX, ldy, sY,
         _k1s_opts(torch.cuda.current_stream(), opts, (B, N, X.dtype), lda=lda))
    return out


# --------------------------------------------------------------------------- K1sw symmetric storage, wide panels (MFMA)
SYMM_WIDE_MIN_P, SYMM_WIDE_MAX_P = 9, 16
SYMM_WIDE_MIN_N = 1024        # below this the tiles are too few to fill the chip: K1w / K1s serve
K1SW_OPTS = 9                 # bit 0: workgroup-cooperative forms; + bit 3 (shipped, r06): column part from the load registers, ring of
                              # four blocks, 2 waves per SIMD; + bit 1 (r05, 3 waves per SIMD): s_setprio around the MFMA block; 0: one wave
                              # per tile (include/xitorch_amd.h)
K1SW_PERSIST = 4              # bit 2 (with bit 0): resident workgroups taking super-tiles from a queue, three per compute unit
K1SW_RESIDENT = False         # False (shipped): one workgroup per super-tile.  True / "auto" (inside the two-group pipeline, from
                              # 4 rounds of workgroups): resident launches + one panel stream per group — measured on the
                              # configs[4] shard (profiles/r05_k1sw_pipeline_ab.jsonl): the resident kernel is 3.7 % slower
                              # per launch (4.32 vs 4.17 ms on one stream: issue-bound, 672 workgroups starting in lock step),
                              # two streams win that back (4.20) and the call stays 106.6 -> 109.6 ms: not shipped


def _k1sw_opts(stream, B, N, pipelined=False):
    o = int(K1SW_OPTS)
    if not (o & 1) or (o & 8):
        return o
    cus = stream_cus(stream)
    tr = 1024 if N >= 8192 else (512 if N >= 2048 else 256)
    tiles = B * (N // 512 + 1) * (N // 512 + 2) // 2 * 512 // tr
    want = K1SW_RESIDENT
    if want == "auto":
        want = pipelined and tiles >= 4 * 3 * cus
    if want:
        o |= K1SW_PERSIST | (min(0xfff, 3 * cus) << 16)
    return o


def symm_wide_ok(A, X):
    """does K1sw (upper triangle streamed once, both products on the matrix cores) serve this operator / panel?"""
    N, P = X.shape[2], X.shape[1]
    if A.dtype != torch.float32 or X.dtype != torch.float32 or not (SYMM_WIDE_MIN_P <= P <= SYMM_WIDE_MAX_P):
        return False
    lda = A.stride(-2)
    sA = A.stride(0) if (A.dim() == 3 and A.shape[0] != 1) else 0
    return (N >= SYMM_WIDE_MIN_N and N % 64 == 0 and lda % 4 == 0 and sA % 4 == 0 and A.data_ptr() % 16 == 0
            and X.stride(1) % 2 == 0 and X.stride(0) % 2 == 0 and X.data_ptr() % 8 == 0 and 64 * lda * 4 < 2 ** 31 - 32)


def _symm_wide_args(A, X, out):
    B, P, N = X.shape
    if A.dtype != torch.float32 or X.dtype != torch.float32 or out.dtype != torch.float32:
        raise _capi.NativeLibraryError("K1sw serves float32 operators and panels only, got %s / %s / %s"
                                       % (A.dtype, X.dtype, out.dtype))
    lda, sA = _op_strides(A)
    if A.shape[-1] != N or A.shape[-2] != N or (N > 1 and A.stride(-1) != 1):
        raise _capi.NativeLibraryError("symmetric operator must be (.., %d, %d) with unit stride" % (N, N))
    ldx, sX = _panel_strides(X)
    ldy, sY = _panel_strides(out)
    nws = fn("xk_dense_symm_wide_workspace_elems")(B, N)
    return B, P, N, lda, sA, ldx, sX, ldy, sY, nws


def dense_symm_wide(A, X, out=None):
    """Y[b,c,:] = A_b X[b,c,:] for EXACTLY symmetric fp32 A (B or 1, N, N) and 9 .. 16 panel columns: the upper triangle
    is streamed once, both y_I += A_IJ x_J and y_J += A_IJ^T x_I run on the matrix cores (K1sw).  The caller guarantees
    A == A^T bit for bit.  X, Y panel-major (B, P, N)."""
    require_device(A, "operator matrix")
    require_device(X, "panel")
    if out is None:
        out = torch.empty_like(X)
    B, P, N, lda, sA, ldx, sX, ldy, sY, nws = _symm_wide_args(A, X, out)
    ws = _workspace(nws, X.dtype, X.device)
    call("xk_dense_symm_wide", torch.float32, ptr(A), ptr(X), ptr(out), ptr(ws), nws, B, N, P, lda, sA, ldx, sX, ldy,
         sY, _k1sw_opts(torch.cuda.current_stream(), B, N))
    return out


def dense_symm_wide_split(A, X, out, tiles_stream, timed=False):
    """K1sw with its two launches on two streams, like `dense_symm_split`: the tile kernel on `tiles_stream`, the fold
    back on the current stream.  Returns the timing events around the tile kernel when `timed`."""
    require_device(A, "operator matrix")
    require_device(X, "panel")
    B, P, N, lda, sA, ldx, sX, ldy, sY, nws = _symm_wide_args(A, X, out)
    cur = torch.cuda.current_stream()
    ws = _workspace(nws, X.dtype, X.device)                 # keyed by the CURRENT (group) stream
    ready, done = sync_events(cur)
    ready.record(cur)
    e0 = e1 = None
    wopts = _k1sw_opts(tiles_stream, B, N, pipelined=True)
    with torch.cuda.stream(tiles_stream):
        tiles_stream.wait_event(ready)
        if timed:
            e0, e1 = timing_event_pair()
            e0.record(tiles_stream)
        call("xk_dense_symm_wide_tiles", torch.float32, ptr(A), ptr(X), ptr(ws), nws, B, N, P, lda, sA, ldx, sX, wopts)
        if timed:
            e1.record(tiles_stream)
        done.record(tiles_stream)
    cur.wait_event(done)
    call("xk_dense_symm_wide_fold", torch.float32, ptr(out), ptr(ws), nws, B, N, P, ldy, sY, wopts)
    return e0, e1


# --------------------------------------------------------------------------- events without per-launch creation
# Creating a HIP event costs host time (and every few hundred of them the runtime grows a pool: a ~30 ms stall seen
# once per process in the benchmark's timed region).  Cross-stream ordering therefore re-records two cached events per
# issuing stream, and timing events come from a pool that measurement code can pre-fill.
_SYNC_EVENTS = {}
_TIMING_POOL = {}            # device index -> pre-created timing events (events belong to the device they were made on)


def sync_events(stream):
    """(ready, done): two cached non-timing events owned by `stream` (the stream that issues the work).  A wait
    captures the record that precedes it, so re-recording them launch after launch is safe."""
    key = (stream.device.index, stream.cuda_stream)
    ev = _SYNC_EVENTS.get(key)
    if ev is None:
        ev = _SYNC_EVENTS[key] = (torch.cuda.Event(), torch.cuda.Event())
    return ev


def timing_event_pair():
    pool = _TIMING_POOL.get(torch.cuda.current_device())
    if pool is not None and len(pool) >= 2:
        return pool.pop(), pool.pop()
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def prefill_timing_events(n):
    """Create (and record once, which is what instantiates them) `n` timing events ahead of a timed region."""
    st = torch.cuda.current_stream()
    fresh = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
    for e in fresh:
        e.record(st)
    st.synchronize()
    _TIMING_POOL.setdefault(torch.cuda.current_device(), []).extend(fresh)


def dense_symm_split(A, X, out, tiles_stream, timed=False):
    """K1s with its two launches on two streams (P <= 6): the tile kernel on `tiles_stream` (after everything
    queued so far on the current stream), the fold back on the current stream once the tiles are done.  The
    partial-sum workspace belongs to the current stream, so callers on different streams never share one.
    Returns the (start, end) timing events recorded around the tile kernel when `timed`, else (None, None)."""
    require_device(A, "operator matrix")
    require_device(X, "panel")
    B, P, N = X.shape
    if P > 6:
        raise _capi.NativeLibraryError("dense_symm_split serves panels of at most 6 columns")
    lda, sA = _op_strides(A)
    ldx, sX = _panel_strides(X)
    ldy, sY = _panel_strides(out)
    nws = fn("xk_dense_symm_workspace_elems")(B, N, P, _esize(X.dtype))
    cur = torch.cuda.current_stream()
    ws = _workspace(nws, X.dtype, X.device)                 # keyed by the CURRENT (group) stream
    ready, done = sync_events(cur)                          # re-recorded on every launch: no event is created here
    ready.record(cur)
    kopts = _k1s_opts(tiles_stream, None, (B, N, X.dtype), pipelined=True, lda=lda)
    e0 = e1 = None
    with torch.cuda.stream(tiles_stream):
        tiles_stream.wait_event(ready)
        if timed:
            e0, e1 = timing_event_pair()
            e0.record(tiles_stream)
        call("xk_dense_symm_tiles", X.dtype, ptr(A), ptr(X), ptr(ws), nws, B, N, P, lda, sA, ldx, sX, kopts)
        if timed:
            e1.record(tiles_stream)
        done.record(tiles_stream)
    cur.wait_event(done)
    call("xk_dense_symm_fold", X.dtype, ptr(out), ptr(ws), nws, B, N, P, ldy, sY, kopts)
    return e0, e1


# --------------------------------------------------------------------------- K1w wide panels (MFMA)
WIDE_MIN_P = 12


def _rows_wide_ok(A, X, N, lda, sA, ldx, sX):
    vn = 2 if A.dtype == torch.float64 else 4
    return N % vn == 0 and lda % vn == 0 and sA % vn == 0 and ldx % vn == 0 and sX % vn == 0 and \
        A.data_ptr() % 16 == 0 and X.data_ptr() % 16 == 0


def dense_rows_wide(A, X, out=None):
    """Y[b,c,:] = A_b X[b,c,:] (row orientation) for any number of panel columns, 32 per pass over A (K1wr: LDS
    tile transpose, lane <-> row, scalar panel loads; no transposed copy of the operator).
    A (B or 1, M, N); X panel-major (B, P, N); returns panel-major (B, P, M)."""
    require_device(A, "operator matrix")
    require_device(X, "panel")
    B, P, N = X.shape
    M = A.shape[-2]
    lda, sA = _op_strides(A)
    if A.shape[-1] != N:
        raise _capi.NativeLibraryError("panel length %d != operator columns %d" % (N, A.shape[-1]))
    ldx, sX = _panel_strides(X)
    if out is None:
        out = torch.empty((B, P, M), dtype=X.dtype, device=X.device)
    ldy, sY = _panel_strides(out)
    nws = fn("xk_dense_rows_wide_workspace_elems")(B, M, N, P, _esize(X.dtype))
    ws = _workspace(nws, X.dtype, X.device) if nws > 0 else None
    call("xk_dense_rows_wide", X.dtype, ptr(A), ptr(X), ptr(out), ptr(ws), nws, B, M, N, P, lda, sA, ldx, sX, ldy, sY)
    return out


def _wide_ok(A, N, lda, sA):
    vn = 2 if A.dtype == torch.float64 else 4
    wcols = 32 if A.dtype == torch.float64 else 128
    return N % wcols == 0 and lda % vn == 0 and sA % vn == 0 and A.data_ptr() % 16 == 0


def dense_wide(A, X, out=None):
    """Y[b,c,:] = A_b^T X[b,c,:] for up to 32 panel columns in ONE pass over A (MFMA).
    A (B or 1, M, N); X panel-major (B, P, M); returns panel-major (B, P, N)."""
    require_device(A, "operator matrix")
    require_device(X, "panel")
    B, P, M = X.shape
    N = A.shape[-1]
    lda, sA = _op_strides(A)
    if A.shape[-2] != M:
        raise _capi.NativeLibraryError("panel length %d != operator rows %d" % (M, A.shape[-2]))
    esize = _esize(X.dtype)
    PP = fn("xk_dense_wide_padded_width")(P, esize)
    Xrm = torch.zeros((B, M, PP), dtype=X.dtype, device=X.device)      # row-major, zero-padded to whole tiles
    Xrm[:, :, :P].copy_(X.transpose(1, 2))
    if out is None:
        out = torch.empty((B, P, N), dtype=X.dtype, device=X.device)
    ldy, sY = _panel_strides(out)
    nws = fn("xk_dense_wide_workspace_elems")(B, M, N, P, esize)
    ws = _workspace(nws, X.dtype, X.device)
    call("xk_dense_wide", X.dtype, ptr(A), ptr(Xrm), ptr(out), ptr(ws), nws, B, M, N, P, lda, sA, Xrm.stride(1),
         Xrm.stride(0), ldy, sY)
    return out


# --------------------------------------------------------------------------- Golub-Kahan-Lanczos kernels (xk_gkl.hip)
GKL_MAX_ROWS = 64            # basis rows one xk_gkl_sweep reads (= the largest ncv)
GKL_BSVD_MAX = 64            # order of the projected matrix xk_gkl_bsvd serves


def gkl_chunks(N, dtype):
    """number of chunks xk_gkl_sweep_* cuts a length-N vector of `dtype` into (one partial sum per chunk)"""
    ce = fn("xk_gkl_chunk_elems")(torch.empty((), dtype=dtype).element_size())
    return (N + ce - 1) // ce


def gkl_nval(j, dtype):
    """partial sums per member and chunk of a sweep over j rows: the j dots (complex: re, im) and the sum of squares"""
    return (2 * j if dtype.is_complex else j) + 1


def gkl_sweep(Q, j, w, dst, coef, scale, part, N, raw=False):
    """dst[b,:N] = scale[b] * (w[b,:N] - sum_{i<j} coef[b,i] Q[b,i,:N]) and the partials of Q[b,:j]^H dst[b], |dst[b]|^2
    (xk_gkl_sweep_*).  Q: (Bt, cap, ld) basis panel (rows are vectors; may be None when j == 0); w, dst: (Bt, L) views
    with unit stride along the vector (dst may be w); coef: float64 rows of unit stride, (Bt, >= j) for real panels and
    for complex panels the interleaved (re, im) pairs as (Bt, >= 2j) -- what gkl_finish writes and the driver passes --
    or the same memory viewed (Bt, >= j, 2); None: no update; scale: (Bt,) float64 or None; part: 1-D float64 of at
    least Bt * gkl_nval(j) * gkl_chunks(N)."""
    require_device(w, "vector")
    Bt = w.shape[0]
    for t in (w, dst):
        if t.dim() != 2 or t.shape[0] != Bt or t.dtype != w.dtype or (t.shape[1] > 1 and t.stride(1) != 1):
            raise _capi.NativeLibraryError("gkl_sweep: w and dst must be (Bt, L) of one dtype, unit stride along the vector")
    if j > 0:
        if Q.dim() != 3 or Q.dtype != w.dtype or Q.shape[0] != Bt or (Q.shape[2] > 1 and Q.stride(2) != 1):
            raise _capi.NativeLibraryError("gkl_sweep: the basis must be a (Bt, cap, ld) panel of the vector's dtype")
        if Q.shape[1] < j or Q.shape[2] < N:
            raise _capi.NativeLibraryError("gkl_sweep: the basis panel has fewer than j rows or rows shorter than N")
    if w.is_complex():
        _require_resolved("gkl_sweep", Q, w, dst)
    if (w.shape[1] < N or dst.shape[1] < N) and N > 0:
        raise _capi.NativeLibraryError("gkl_sweep: a vector is shorter than N = %d" % N)
    if coef is not None and (coef.dtype != torch.float64 or coef.shape[0] != Bt or coef.stride(-1) != 1 or
                             (coef.dim() == 3 and coef.stride(1) != 2)):
        raise _capi.NativeLibraryError("gkl_sweep: coef must be float64 (Bt, j) (complex: (Bt, 2j) or (Bt, j, 2)), contiguous rows")
    if part.dtype != torch.float64 or not part.is_contiguous():
        raise _capi.NativeLibraryError("gkl_sweep: part must be a contiguous float64 tensor")
    one = Bt == 1
    rc = call("xk_gkl_sweep", w.dtype,
              ptr(Q if j > 0 else None), Q.stride(1) if j > 0 else 0, 0 if (one or j == 0) else Q.stride(0),
              ptr(w), 0 if one else w.stride(0), ptr(dst), 0 if one else dst.stride(0),
              ptr(coef), 0 if (coef is None or one) else coef.stride(0), ptr(scale), ptr(part), part.numel(),
              Bt, int(j), int(N), raw=raw)
    return rc if raw else dst


def gkl_finish(part, Bt, nval, nchunk, coef, nrm, rnrm, dst=None, smax=None, u=0.0, brk=None, code=0, raw=False):
    """fixed-order sums of a sweep's partials (xk_gkl_finish): coef[b, :nval-1] (may be None), nrm[b] = norm, rnrm[b] = 1 / norm,
    dst[b] = norm for a (Bt,) float64 VIEW dst (e.g. Bm[:, j, j]; None: not stored), smax[b] = max(smax[b], norm);
    breakdown (norm <= u * smax[b] or not finite): norm = 1 / norm = 0 and brk[b] = code where brk[b] < 0."""
    require_device(part, "partials")
    sdst = 0
    if dst is not None:
        if dst.dtype != torch.float64 or dst.dim() != 1 or dst.shape[0] != Bt:
            raise _capi.NativeLibraryError("gkl_finish: dst must be a (Bt,) float64 view")
        sdst = dst.stride(0) if Bt > 1 else 0
    return call("xk_gkl_finish", None, ptr(part), Bt, int(nval), int(nchunk), ptr(coef),
                0 if (coef is None or Bt == 1) else coef.stride(0), ptr(nrm), ptr(rnrm), ptr(dst), sdst, ptr(smax),
                float(u), ptr(brk), int(code), raw=raw)


def gkl_bsvd(Bm, beta=None, smax=None, brk=None, k=0, keep=0, descending=True, tol=0.0, Bnext=None, out=None,
             raw=False):
    """SVD of the (Bt, n, n) float64 projected matrices by one-sided Jacobi in LDS (xk_gkl_bsvd), n <= 64.  Returns
    (sigma (Bt, n) in the asked order, P, Q (Bt, n, n) vectors as columns, res (Bt, n) = |beta P[n-1, :]|,
    status (Bt, 4) int32 = converged among the first k / sweeps / sweep-limit flag / breakdown code).  Bnext: receives
    the projected matrix of the restarted basis (keep < n).  out: a tuple of the five outputs to reuse."""
    require_device(Bm, "projected matrix")
    if Bm.dtype != torch.float64 or Bm.dim() != 3 or Bm.shape[1] != Bm.shape[2] or not Bm.is_contiguous():
        raise _capi.NativeLibraryError("gkl_bsvd: Bm must be a contiguous (Bt, n, n) float64 tensor")
    Bt, n = Bm.shape[0], Bm.shape[1]
    if out is None:
        mk = lambda *s: torch.empty(s, dtype=torch.float64, device=Bm.device)
        out = (mk(Bt, n), mk(Bt, n, n), mk(Bt, n, n), mk(Bt, n), torch.zeros((Bt, 4), dtype=torch.int32, device=Bm.device))
    sigma, P, Q, res, status = out
    rc = call("xk_gkl_bsvd", None, ptr(Bm), ptr(beta), ptr(smax), ptr(brk), Bt, n, int(k), int(keep),
              1 if descending else 0, float(tol), ptr(sigma), ptr(P), ptr(Q), ptr(res), ptr(status), ptr(Bnext), raw=raw)
    return rc if raw else out


# --------------------------------------------------------------------------- Krylov-Schur Arnoldi kernels (xk_arn.hip)
ARN_WHICH = {"LM": 0, "LR": 1, "SR": 2, "LI": 3, "SI": 4}
ARN_FLAG_NONFINITE, ARN_FLAG_QR_LIMIT, ARN_FLAG_NOT_CLOSED, ARN_FLAG_KEEP_MOVED = 1, 2, 4, 8


def arn_max_rows():
    """largest order of the projected matrix xk_arn_schur serves (= the largest ncv of eigs)"""
    return int(fn("xk_arn_max_rows")())


def arn_status_words():
    return int(fn("xk_arn_status_words")())


def arn_finish(part, Bt, nval, nchunk, coef, nrm, rnrm, hcol=None, accumulate=False, dst=None, smax=None, u=0.0,
               brk=None, code=0, raw=False):
    """gkl_finish with the dots also stored in (accumulate: added to) a column of the projected matrix (xk_arn_finish).
    hcol: the (Bt, rows) float64 or (Bt, rows) complex128 VIEW H[:, :rows, j] of the (Bt, m + 1, m) Hessenberg matrix
    (None: not stored); dst: the (Bt,) float64 view that receives the norm (H[:, j + 1, j], or its real part)."""
    require_device(part, "partials")
    sdst = sHb = sHr = cplx = 0
    if dst is not None:
        if dst.dtype != torch.float64 or dst.dim() != 1 or dst.shape[0] != Bt:
            raise _capi.NativeLibraryError("arn_finish: dst must be a (Bt,) float64 view")
        sdst = dst.stride(0) if Bt > 1 else 0
    if hcol is not None:
        cplx = 1 if hcol.is_complex() else 0
        if hcol.dtype not in (torch.float64, torch.complex128) or hcol.dim() != 2 or hcol.shape[0] != Bt or \
                hcol.shape[1] * (2 if cplx else 1) != nval - 1:
            raise _capi.NativeLibraryError("arn_finish: hcol must be a (Bt, rows) float64 / complex128 view of nval - 1 "
                                           "doubles per member")
        mul = 2 if cplx else 1
        sHb, sHr = (hcol.stride(0) * mul if Bt > 1 else 0), hcol.stride(1) * mul
    return call("xk_arn_finish", None, ptr(part), Bt, int(nval), int(nchunk), ptr(coef),
                0 if (coef is None or Bt == 1) else coef.stride(0), ptr(nrm), ptr(rnrm), ptr(hcol), sHb, sHr, cplx,
                1 if accumulate else 0, ptr(dst), sdst, ptr(smax), float(u), ptr(brk), int(code), raw=raw)


def arn_schur(H, neig, keep, which="LM", tol=0.0, u=0.0, keep_add=None, brk=None, Hnext=None, out=None, raw=False):
    """Schur form, ranking, reordering, Ritz data and restart coefficients of the (Bt, m + 1, m) float64 / complex128
    projected matrices of an Arnoldi cycle, in LDS (xk_arn_schur), m <= arn_max_rows().  Returns (theta (Bt, m)
    complex128 in rank order, Y (Bt, m, neig) complex128 unit Ritz vectors as columns, res (Bt, neig) = |beta Y[m-1, :]|,
    Q (Bt, m, m) in H's dtype with the restart coefficients in its first keep' columns, status (Bt, 8) int32 =
    converged among the first neig / QR iterations / flags / keep' / breakdown code).  Hnext: receives the projected
    matrix of the restarted basis.  keep_add: (Bt,) int32 added to keep per member.  out: the five outputs to reuse."""
    require_device(H, "projected matrix")
    if H.dtype not in (torch.float64, torch.complex128) or H.dim() != 3 or H.shape[1] != H.shape[2] + 1 or \
            not H.is_contiguous():
        raise _capi.NativeLibraryError("arn_schur: H must be a contiguous (Bt, m + 1, m) float64 / complex128 tensor")
    if which not in ARN_WHICH:
        raise _capi.NativeLibraryError("arn_schur: which must be one of %s" % sorted(ARN_WHICH))
    Bt, m = H.shape[0], H.shape[2]
    if Hnext is None:
        Hnext = torch.empty_like(H)
    if Hnext.shape != H.shape or Hnext.dtype != H.dtype or not Hnext.is_contiguous():
        raise _capi.NativeLibraryError("arn_schur: Hnext must be a contiguous tensor of H's shape and dtype")
    if out is None:
        mk = lambda dt, *s: torch.zeros(s, dtype=dt, device=H.device)
        out = (mk(torch.complex128, Bt, m), mk(torch.complex128, Bt, m, int(neig)), mk(torch.float64, Bt, int(neig)),
               mk(H.dtype, Bt, m, m), mk(torch.int32, Bt, 8))
    theta, Y, res, Q, status = out
    want = ((theta, torch.complex128, (Bt, m)), (Y, torch.complex128, (Bt, m, int(neig))),
            (res, torch.float64, (Bt, int(neig))), (Q, H.dtype, (Bt, m, m)), (status, torch.int32, (Bt, 8)))
    for t, dt, shape in want:
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != H.device:
            raise _capi.NativeLibraryError("arn_schur: an output is not a contiguous %s tensor of shape %s on H's device"
                                           % (dt, shape))
    for t, n in ((keep_add, "keep_add"), (brk, "brk")):
        if t is not None and (t.dtype != torch.int32 or t.numel() < Bt or not t.is_contiguous() or t.device != H.device):
            raise _capi.NativeLibraryError("arn_schur: %s must be a contiguous (Bt,) int32 tensor on H's device" % n)
    rc = call("xk_arn_schur", None, ptr(H), Bt, m, int(neig), int(keep), ptr(keep_add), ARN_WHICH[which],
              1 if H.is_complex() else 0, float(tol), float(u), ptr(brk), ptr(theta), ptr(Y), ptr(res), ptr(Q),
              ptr(Hnext), ptr(status), raw=raw)
    return rc if raw else out


# --------------------------------------------------------------------------- FSAI preconditioner build
def fsai_max_row():
    return int(fn("xk_fsai_max_row")())


def fsai_check_pattern(g_ptr, g_idx, N, cap=None):
    """The contract of xk_fsai_build (and, with cap = xk_fsai_lu_max_row(), of xk_fsai_lu_build) on the pattern of G,
    checked once in torch ops: every row has between 1 and `cap` (default xk_fsai_max_row()) columns, ascending and
    unique, none beyond the row index, the row index itself last."""
    cap = fsai_max_row() if cap is None else cap
    if g_ptr.dtype != torch.int32 or g_idx.dtype != torch.int32 or g_ptr.dim() != 1 or g_idx.dim() != 1 or \
            g_ptr.numel() != N + 1 or not g_ptr.is_contiguous() or not g_idx.is_contiguous():
        raise _capi.NativeLibraryError("fsai: the pattern of G must be contiguous int32 arrays, g_ptr of N + 1 entries")
    p = g_ptr.to(torch.int64)
    lens = p[1:] - p[:-1]
    if int(p[0]) != 0 or int(p[-1]) != g_idx.numel() or int(lens.min()) < 1:
        raise _capi.NativeLibraryError("fsai: g_ptr must run from 0 to the entry count and leave no row empty")
    if int(lens.max()) > cap:
        raise _capi.NativeLibraryError("fsai: a row of G has %d columns, the kernel's cap is %d"
                                       % (int(lens.max()), cap))
    rows = torch.arange(N, dtype=torch.int64, device=g_ptr.device)
    idx = g_idx.to(torch.int64)
    if not bool((idx[p[1:] - 1] == rows).all()):
        raise _capi.NativeLibraryError("fsai: the last column of every row of G must be the row index")
    row_of = torch.repeat_interleave(rows, lens, output_size=idx.numel())
    if int(idx.min()) < 0 or not bool((idx <= row_of).all()):
        raise _capi.NativeLibraryError("fsai: G is lower triangular, a column index lies outside [0, row]")
    if idx.numel() > 1 and not bool(((idx[1:] > idx[:-1]) | (row_of[1:] != row_of[:-1])).all()):
        raise _capi.NativeLibraryError("fsai: the columns of a row of G must be ascending and unique")


def fsai_build(a_ptr, a_idx, a_val, g_ptr, g_idx, N, out=None, nfail=None, check_pattern=True, raw=False):
    """The FSAI values on the pattern (g_ptr, g_idx) of the Hermitian CSR operator (a_ptr, a_idx, a_val) (xk_fsai_build_*):
    a_val (B, nnz) rows of unit stride (B = 1 for values shared by a batch: G is shared then as well); returns
    (g_val (B, g_nnz), nfail (B,) int32 = rows that fell back to the Jacobi row).  fp64 / fp32 / complex128 /
    complex64; complex values must be resolved."""
    require_device(a_val, "values")
    if a_val.is_complex():
        _require_resolved("fsai_build", a_val, out)
    for t in (a_ptr, a_idx, g_ptr, g_idx):
        if t.dtype != torch.int32 or t.device != a_val.device or not t.is_contiguous():
            raise _capi.NativeLibraryError("fsai_build: index arrays must be contiguous int32 on the values' device")
    a_nnz, g_nnz = a_idx.numel(), g_idx.numel()
    if a_ptr.numel() != N + 1 or a_val.dim() != 2 or a_val.shape[1] != a_nnz or (a_nnz > 1 and a_val.stride(1) != 1):
        raise _capi.NativeLibraryError("fsai_build: a_ptr must have N + 1 entries and the values be (B, %d) rows of "
                                       "unit stride, got %s" % (a_nnz, tuple(a_val.shape)))
    if check_pattern:
        fsai_check_pattern(g_ptr, g_idx, N)
    B = a_val.shape[0]
    if out is None:
        out = torch.zeros((B, g_nnz), dtype=a_val.dtype, device=a_val.device)
    if out.shape != (B, g_nnz) or out.dtype != a_val.dtype or not out.is_contiguous():
        raise _capi.NativeLibraryError("fsai_build: the output must be a contiguous (%d, %d) tensor" % (B, g_nnz))
    if nfail is None:
        nfail = torch.zeros((B,), dtype=torch.int32, device=a_val.device)
    rc = call("xk_fsai_build", a_val.dtype, ptr(a_ptr), ptr(a_idx), ptr(a_val), a_val.stride(0) if B > 1 else 0, a_nnz,
              ptr(g_ptr), ptr(g_idx), ptr(out), out.stride(0) if B > 1 else 0, g_nnz, ptr(nfail), int(N), B, raw=raw)
    return rc if raw else (out, nfail)


# --------------------------------------------------------------------------- unsymmetric FSAI build
def fsai_lu_max_row():
    return int(fn("xk_fsai_lu_max_row")())


def fsai_lu_build(a_ptr, a_idx, a_val, g_ptr, g_idx, N, out=None, nfail=None, check_pattern=True, raw=False):
    """The values of G_L and W = G_U^H on the one pattern (g_ptr, g_idx) for the CSR operator (a_ptr, a_idx, a_val)
    (xk_fsai_lu_build_*): a_val (B, nnz) rows of unit stride (B = 1 for values shared by a batch: the factors are shared
    then as well); out = (gl, w), two contiguous (B, g_nnz) tensors; returns (gl, w, nfail (B,) int32 = fallback rows).
    fp64 / fp32 / complex128 / complex64; complex values must be resolved."""
    require_device(a_val, "values")
    if a_val.is_complex():
        _require_resolved("fsai_lu_build", a_val, *(out or ()))
    for t in (a_ptr, a_idx, g_ptr, g_idx):
        if t.dtype != torch.int32 or t.device != a_val.device or not t.is_contiguous():
            raise _capi.NativeLibraryError("fsai_lu_build: index arrays must be contiguous int32 on the values' device")
    a_nnz, g_nnz = a_idx.numel(), g_idx.numel()
    if a_ptr.numel() != N + 1 or a_val.dim() != 2 or a_val.shape[1] != a_nnz or (a_nnz > 1 and a_val.stride(1) != 1):
        raise _capi.NativeLibraryError("fsai_lu_build: a_ptr must have N + 1 entries and the values be (B, %d) rows of "
                                       "unit stride, got %s" % (a_nnz, tuple(a_val.shape)))
    if check_pattern:
        fsai_check_pattern(g_ptr, g_idx, N, cap=fsai_lu_max_row())
    B = a_val.shape[0]
    if out is None:
        out = tuple(torch.zeros((B, g_nnz), dtype=a_val.dtype, device=a_val.device) for _ in range(2))
    gl, w = out
    for t in (gl, w):
        if t.shape != (B, g_nnz) or t.dtype != a_val.dtype or not t.is_contiguous() or t.device != a_val.device:
            raise _capi.NativeLibraryError("fsai_lu_build: the outputs must be contiguous (%d, %d) tensors" % (B, g_nnz))
    if nfail is None:
        nfail = torch.zeros((B,), dtype=torch.int32, device=a_val.device)
    rc = call("xk_fsai_lu_build", a_val.dtype, ptr(a_ptr), ptr(a_idx), ptr(a_val), a_val.stride(0) if B > 1 else 0,
              a_nnz, ptr(g_ptr), ptr(g_idx), ptr(gl), ptr(w), gl.stride(0) if B > 1 else 0, g_nnz, ptr(nfail), int(N),
              B, raw=raw)
    return rc if raw else (gl, w, nfail)
