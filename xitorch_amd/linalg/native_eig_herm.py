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
from xitorch_amd.linalg._panel import PanelOperator, batch_count, require_hip
# (herm_partial_eigh and _shift_rel: re-exported under the names the tests and scripts know)
from xitorch_amd.linalg._block import ComplexBlockOps, herm_partial_eigh, _initial_block, _shift_rel

__all__ = ["davidson", "herm_partial_eigh"]


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
    opA = PanelOperator(A, bdims, B, N)
    opM = PanelOperator(M, bdims, B, N) if M is not None else None
    ops = ComplexBlockOps(B, N, p, dtype, device)
    counts, info = ops.counts, ops.info

    def apply(op, X):
        out = torch.empty_like(X)
        op.apply(X, out)
        return out

    def orthonormalise(W, bas, k):
        """W (B, q, N), a fresh block -> (W, M W): (M-)orthonormal, (M-)orthogonal to the first k basis vectors: two
        passes, M W recomputed after each projection, the first pass shifted when there is a basis to project against"""
        MW = torch.empty_like(W) if opM is not None else None
        ops.orth_block(W, bas.V[:, :k] if k > 0 else None, 2, info, k > 0, MW=MW,
                       MV=bas.MV[:, :k] if opM is not None and k > 0 else None, opM=opM)
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
    bas.T[:, :k, :k].copy_(ops.gram(bas.V[:, :k], bas.AV[:, :k]))
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
        Tcol = ops.gram(bas.V[:, :k], AW)                       # (B, k, nadd) = V^H A W
        bas.T[:, :k, k:k + nadd].copy_(Tcol)
        bas.T[:, k:k + nadd, :k].copy_(Tcol.transpose(1, 2).conj())
        bas.T[:, k:k + nadd, k:k + nadd].copy_(ops.gram(W, AW))
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
