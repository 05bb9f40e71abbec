"""Native (HIP) block Davidson for complex Hermitian operators on a HIP device.

`native_eig.davidson` hands every complex128 / complex64 device operator to `davidson` below.  The iteration is
host_eig.py's (which is correct for complex Hermitian operators: conjugate transposes throughout) — start block from
the reference's seed, Rayleigh–Ritz on the whole basis, ONE global stopping test `max|A X - M X diag(lam)| < min_eps`
or a square basis, the best block returned, expansion by the negated residual block; only the NEW block is
orthonormalised (two passes of block Gram–Schmidt against the basis, each followed by a CholeskyQR of the block — the
first one shifted) and `T = V^H A V` is extended by its new rows.  The reference's own davidson is real-only (it builds
`T = V^T A V` with an unconjugated transpose, xitorch/_impls/linalg/symeig.py:165-174).

Every step is a HIP kernel (xk_herm_davidson.hip through `kernels`, the operator and the tall products on the real K1
kernels through the interleaved storage, `kernels.dense_mm_complex`); the only library call is `torch.linalg.eigh` of
the small T beyond the native Rayleigh–Ritz range (k > 128 or neig > 16) and for members whose self-check failed.
One stream; the host reads the status once per iteration.
"""
import torch
from xitorch_amd import kernels as K
from xitorch_amd._capi import NativeLibraryError
from xitorch_amd._util import bcast_shape
from xitorch_amd.linalg._panel import PanelOperator, batch_count, real_dtype, require_hip
from xitorch_amd.linalg.native_eig import _initial_block, _shift_rel

__all__ = ["davidson", "herm_partial_eigh"]


def herm_partial_eigh(T, k, p, mode, counts=None):
    """Lowest / uppermost p eigenpairs of the Hermitian (B, >=k, >=k) complex T[:, :k, :k]: lam (B, p) real
    ascending, Y (B, k, p) complex.  Native kernel inside its range, members whose self-check fails redone on
    torch.linalg.eigh, the library beyond the range; `counts` ({"rr_native": .., "rr_library": ..}) counts the calls
    served each way (a call with any redone member counts as a library call)."""
    B = T.shape[0]
    if K.herm_eigh_ok(k, p):
        lam, Yt, flag = K.herm_eigh(T, k, p, uppest=(mode != "lowest"))
        Y = Yt.transpose(1, 2)
        if int(flag.max().item()) == 0:
            if counts is not None:
                counts["rr_native"] += 1
            return lam, Y
        bad = torch.nonzero(flag, as_tuple=False).flatten()
        l2, U2 = _library_eigh(T[bad, :k, :k], p, mode)
        lam, Y = lam.clone(), Y.clone()
        lam[bad], Y[bad] = l2, U2
    else:
        lam, Y = _library_eigh(T[:B, :k, :k], p, mode)
    if counts is not None:
        counts["rr_library"] += 1
    return lam, Y


def _library_eigh(T, p, mode):
    lam, U = torch.linalg.eigh(T)                     # (lower triangle, like the kernel)
    if mode == "lowest":
        return lam[..., :p].contiguous(), U[..., :p]
    return lam[..., -p:].contiguous(), U[..., -p:]


def _gram(Vk, W):
    """C[b, i, c] = sum_n conj(Vk[b, i, n]) W[b, c, n]  (B, k, q): V^H W on K1 with the basis as the matrix"""
    return K.dense_mm_complex(Vk, W, conj_io=True).transpose(1, 2)


def _combine(Vk, C):
    """out[b, c, :] = sum_i C[b, i, c] Vk[b, i, :]  (B, q, N): the projection V C on K1"""
    return K.dense_mm_complex(Vk, C.transpose(1, 2).contiguous(), adjoint=True, conj_io=True)


class _Basis:
    """V, A V (and M V) in (B, cap, N) panel-major device buffers, T in (B, cap, cap); capacity doubled on demand."""

    def __init__(self, B, N, cap, dtype, device, with_m):
        self.B, self.N, self.dtype, self.device, self.with_m = B, N, dtype, device, with_m
        self.k = 0
        self.cap = 0
        self.V = self.AV = self.MV = self.T = None
        self.grow(cap)

    def grow(self, cap):
        cap = min(max(cap, 1), self.N)
        if cap <= self.cap:
            return
        B, N, k = self.B, self.N, self.k
        new = lambda *s: torch.zeros(s, dtype=self.dtype, device=self.device)
        V, AV, T = new(B, cap, N), new(B, cap, N), new(B, cap, cap)
        MV = new(B, cap, N) if self.with_m else None
        if k > 0:
            V[:, :k].copy_(self.V[:, :k])
            AV[:, :k].copy_(self.AV[:, :k])
            T[:, :k, :k].copy_(self.T[:, :k, :k])
            if MV is not None:
                MV[:, :k].copy_(self.MV[:, :k])
        self.V, self.AV, self.MV, self.T, self.cap = V, AV, MV, T, cap

    def mv(self, hi):
        return self.MV[:, :hi] if self.with_m else self.V[:, :hi]


def davidson(A, neig, mode, M=None, max_niter=1000, nguess=None, v_init="randn", max_addition=None, min_eps=1e-6,
             verbose=False, V0=None, process_group=None, trace=None, rng_device="cpu", precond=None, restart=None,
             **unused):
    """Block Davidson for a complex Hermitian operator on a HIP device; options as `native_eig.davidson`.  The
    scheduling options of the real pipeline are accepted and ignored; `precond=`, `restart=` and batch sharding over
    several ranks are not available for complex operators."""
    dtype, device = A.dtype, torch.device(A.device)
    require_hip(A, "davidson")
    if not dtype.is_complex:
        raise NativeLibraryError("native_eig_herm serves complex128 / complex64 operators, got %s" % dtype)
    if precond is not None or restart is not None:
        raise NativeLibraryError("precond= / restart= are not available for complex Hermitian operators: the native "
                                 "extension (xk_herm_davidson) has no preconditioned or restarted form")
    if process_group is not None and torch.distributed.get_world_size(process_group) > 1:
        raise NativeLibraryError("batch sharding over several ranks is not available for complex Hermitian operators: "
                                 "the native extension (xk_herm_davidson) runs one device")
    N = A.shape[-1]
    p = neig
    if nguess is None:
        nguess = neig
    if M is not None and (nguess > 32 or p > 32):
        raise NativeLibraryError("neig / nguess > 32 with an overlap operator M is not supported by the native "
                                 "davidson")
    if nguess > K.HERM_CHOLQR_MAX_Q or p > K.HERM_CHOLQR_MAX_Q:
        raise NativeLibraryError("neig / nguess > %d is not supported by the native complex davidson (block width of "
                                 "xk_herm_cholqr)" % K.HERM_CHOLQR_MAX_Q)
    bdims = list(A.shape[:-2]) if M is None else list(bcast_shape(A.shape[:-2], M.shape[:-2]))
    B = batch_count(bdims)
    rdtype = real_dtype(dtype)
    opA = PanelOperator(A, bdims, B, N)
    opM = PanelOperator(M, bdims, B, N) if M is not None else None
    counts = {"rr_native": 0, "rr_library": 0}
    info = torch.zeros((B,), dtype=torch.int32, device=device)

    def apply(op, X):
        out = torch.empty_like(X)
        op.apply(X, out)
        return out

    def orthonormalise(W, bas, k):
        """W (B, q, N) -> (W, M W): (M-)orthonormal, (M-)orthogonal to the first k basis vectors"""
        q = W.shape[1]
        MW = None
        for rnd in range(2):
            if k > 0:
                C = _gram(bas.mv(k), W)                       # (MV)^H W
                W = W - _combine(bas.V[:, :k], C)
            MW = apply(opM, W) if opM is not None else None
            K.herm_cholqr(W, info, MW=MW, shift_rel=_shift_rel(N, q, rdtype) if (rnd == 0 and k > 0) else 0.0)
        return W, MW

    V0p = _initial_block(v_init, V0, bdims, B, N, nguess, dtype, device, rng_device)      # (B, nguess, N)
    bas = _Basis(B, N, nguess + 8 * p, dtype, device, M is not None)
    W, MW = orthonormalise(V0p.contiguous(), bas, 0)
    if int(info.max().item()) != 0:
        raise RuntimeError("davidson: the start block is rank deficient (linearly dependent start vectors)")
    k = nguess
    bas.V[:, :k].copy_(W)
    if MW is not None:
        bas.MV[:, :k].copy_(MW)
    bas.AV[:, :k].copy_(apply(opA, W))
    bas.T[:, :k, :k].copy_(_gram(bas.V[:, :k], bas.AV[:, :k]))
    bas.k = k

    Xs = [torch.empty((B, p, N), dtype=dtype, device=device) for _ in range(2)]
    Tn = torch.empty((B, p, N), dtype=dtype, device=device)
    status = torch.zeros((B + 1,), dtype=torch.float64, device=device)
    slot, best_slot, best_lam = 0, -1, None
    best_resid = float("inf")
    history = []
    niter = 0
    stop_reason = "max_niter"
    for it in range(max_niter):
        niter = it + 1
        lam, Y = herm_partial_eigh(bas.T, k, p, mode, counts)
        if slot == best_slot:
            slot = 1 - slot
        K.herm_ritz(bas.V, bas.AV, Y, lam, Xs[slot], Tn, status, k, p, MV=bas.MV if M is not None else None)
        max_resid, flag = torch.stack((status[0], info.max().to(torch.float64))).tolist()
        if max_resid != max_resid:
            max_resid = float("inf")
        if flag != 0:
            # the block appended last lost its rank: this basis is not orthonormal, its Ritz pairs do not count
            stop_reason = "breakdown"
            break
        history.append(max_resid)
        if verbose:
            print("Iter %3d (guess size: %d): resid: %.3e" % (it + 1, k, max_resid))
        if max_resid < best_resid:
            best_resid, best_slot, best_lam = max_resid, slot, lam
        if max_resid < min_eps:
            stop_reason = "converged"
            break
        if k == N:
            stop_reason = "full_basis"
            break
        nadd = min(p, N - k)
        W, MW = orthonormalise(Tn[:, :nadd].clone(), bas, k)
        AW = apply(opA, W)
        bas.grow(max(2 * bas.cap, k + nadd) if k + nadd > bas.cap else bas.cap)
        bas.V[:, k:k + nadd].copy_(W)
        bas.AV[:, k:k + nadd].copy_(AW)
        if MW is not None:
            bas.MV[:, k:k + nadd].copy_(MW)
        Tcol = _gram(bas.V[:, :k], AW)                       # (B, k, nadd) = V^H A W
        bas.T[:, :k, k:k + nadd].copy_(Tcol)
        bas.T[:, k:k + nadd, :k].copy_(Tcol.transpose(1, 2).conj())
        bas.T[:, k:k + nadd, k:k + nadd].copy_(_gram(W, AW))
        k += nadd
        bas.k = k
    if best_slot < 0:
        raise RuntimeError("xitorch_amd davidson: no finite residual was produced")
    if trace is not None:
        trace.update(niter=niter, napply=opA.napply, resid_history=history, basis_size=k, best_resid=best_resid,
                     stop_reason=stop_reason, groups=1,
                     panel_kernel="K1 (complex, interleaved)" if opA.kind == "dense" else opA.kind,
                     rr_native=counts["rr_native"], rr_library=counts["rr_library"])
    evals = best_lam.reshape(*bdims, p)
    evecs = Xs[best_slot].transpose(-2, -1).reshape(*bdims, N, p)
    return evals, evecs
