"""LOBPCG on the HIP kernels: `symeig(..., method="lobpcg")`.

An extension (the reference leaves it as a TODO, xitorch/linalg/symeig.py:123): Knyazev's locally optimal block
preconditioned conjugate gradient method (SIAM J. Sci. Comput. 23 (2001) 517) in the basis-orthonormal form of Duersch,
Shao, Yang and Gu (SIAM J. Sci. Comput. 40 (2018) C655).  Block Davidson keeps every vector it ever added; Chebyshev-
filtered subspace iteration has a fixed block but takes neither an overlap operator nor a preconditioner.  Here the
storage is three stacks S = [X | P | W], A S and — with an overlap operator — M S of 3 w rows each, w = neig + nguard,
and nothing else grows with N.  One iteration is

  1. W = T R on the residual rows the previous rotation left in the stack (T: `precond` in davidson's grammar — None,
     "diag" / "jacobi" or a diagonal tensor d: T = |d|^-1 by `xk_diag_precond` (positive definite, as LOBPCG needs it;
     not davidson's indefinite (diag A - lam diag M)^-1), or a Hermitian positive definite LinearOperator such as
     `fsai(A)` through the panel kernels), columns scaled to unit norm (no preconditioner: from the rotation kernel's
     partial sums), columns without a direction replaced by random ones;
  2. W made M-orthonormal against [X, P] and within itself: two passes of projection + CholeskyQR, the first shifted
     (`xk_davidson_orth`; with M: K1 Gram blocks, `xk_lincomb`, `xk_panel_chol`, `xk_panel_transform`; complex:
     K1 projections + `xk_herm_cholqr`), M applied to W once and M W transformed alongside;
  3. A W: the one operator product, on the wide panel kernels (`PanelOperator.apply`);
  4. T_S = sign * S^H A S recomputed from the stacks (K1 Gram block), its w lowest pairs from the native dense solvers
     (`native_partial_eigh` / the Jacobi kernel; complex: `herm_partial_eigh` up to 16 vectors, the library beyond),
     C_p from C_x by a handful of torch ops on (Bt, k, w) device tensors (`host_eig.lob_cp`);
  5. the rotation in place, `xk_lobpcg_rotate`: X' = S C_x, P' = S C_p, the same of A S and M S, the new residual into
     the dead W rows with its partial sums — 6 w N to 9 w N elements read (w <= 8; wider blocks read back w N more,
     see xk_lobpcg.hip), no second copy of the stacks;
  6. the guard max|X'^H M X' - I| (`xk_ritz_guard`), `xk_group_status` and ONE host read of {max|resid|, Cholesky
     flag, guard} by the driver itself.  The dense eigensolvers add one read of their own per call: the self-check
     flag inside `native_partial_eigh` (real) and inside `herm_partial_eigh` (complex).  max|resid| is taken over the
     wanted columns: with guard vectors that is one more read of neig N residual elements (the kernel's per-member
     maximum covers the whole block).

Library calls on the device, all on small (Bt, k, w) or (Bt, k, k) tensors: `torch.linalg.qr` twice per iteration in
`lob_cp`, and `torch.linalg.eigh` for complex blocks wider than 16 vectors or where a self-check flag is set.

`host_eig.lobpcg` is the same algorithm in torch ops for operators in host memory.  Not built: locking / deflation of
converged columns, batch sharding, an MFMA form of the rotation.
"""
import warnings
import torch
from xitorch_amd import kernels as K
from xitorch_amd._util import ConvergenceWarning
from xitorch_amd.linalg._panel import PanelOperator, real_dtype, require_hip
from xitorch_amd.linalg._block import block_ops, GUARD_BAD, GUARD_MAX_REDO, _preconditioner
from xitorch_amd.linalg import host_eig
from xitorch_amd.linalg.host_eig import lob_cp, lob_dependent_columns

__all__ = ["lobpcg"]


class _Stacks:
    """the three stacks S = [X | P | W], A S and M S on the block layer, and the rotation kernel's partial sums"""

    def __init__(self, ops, neig, with_m):
        self.ops, self.w, self.neig = ops, ops.w, neig
        self.nalloc = 0                                   # panel buffers allocated, in units of (Bt, w, ld)
        self.S = self.panels(3)
        self.AS = self.panels(3)
        self.MS = self.panels(3) if with_m else None
        nblk = K.lobpcg_blocks(ops.N, ops.dtype)
        self.Pnorm = torch.zeros((ops.Bt, self.w, nblk), dtype=torch.float64, device=ops.device)
        self.Pmax = torch.zeros((ops.Bt, nblk), dtype=torch.float64, device=ops.device)

    def panels(self, n):
        self.nalloc += n
        return self.ops.panel(n * self.w)

    def rotate(self, C, lam, k, q):
        """the stacks' rows [0, q) <- their combinations by C (Bt, k, q); residual -> S rows [q, q + w)"""
        K.lobpcg_rotate(self.S, self.AS, self.MS, C, lam.to(torch.float64).contiguous(), k, q, self.w, N=self.ops.N,
                        Pnorm=self.Pnorm, Pmax=self.Pmax)

    def resid_max(self, q):
        """(Bt,) float64: largest residual entry over the WANTED columns.  The kernel's Pmax covers all w columns of
        the block, so it serves only a block without guard vectors; otherwise one more read of the neig wanted
        residual rows (a max-norm reduction, no temporary panel)."""
        if self.neig == self.w:
            return self.Pmax.amax(dim=1)
        R = self.S[:, q:q + self.neig, :self.ops.N]
        return torch.linalg.vector_norm(R, ord=float("inf"), dim=(1, 2)).to(torch.float64)

    def orth(self, k0, passes, opM):
        """rows [k0, k0 + w) of S M-orthonormal and M-orthogonal to rows [0, k0); with M the rows of MS follow (M is
        applied once).  The Cholesky flags land in ops.info (sticky)."""
        self.ops.orth(self.S, k0, self.w, passes, self.ops.info, MS=self.MS, opM=opM)

    def status_read(self, q):
        """[max|resid| over the wanted columns, Cholesky flag, guard] of X = rows [0, w): the one host read"""
        return self.ops.status(self.S, self.w, self.resid_max(q), self.ops.info, MX=self.MS)


def lobpcg(A, neig, mode, M=None, max_niter=200, min_eps=1e-6, nguard=None, precond=None, V0=None, v_init="randn",
           rng_device="cpu", verbose=False, trace=None, process_group=None, **unused):
    """
    LOBPCG for the ``neig`` lowest / uppermost eigenpairs of a large Hermitian operator, also of the generalised problem
    ``A x = lam M x`` (dense, banded, CSR or a user ``_mv``; float64, float32, complex128, complex64; any batch shape),
    in constant storage on the HIP kernels: three stacks of ``3 (neig + nguard)`` vectors whatever the iteration count.

    Keyword arguments
    -----------------
    max_niter: int
        Maximum number of iterations (each: one operator product and one preconditioner product on the block)
    min_eps: float
        Stop when the largest residual element ``max|A X - M X diag(lam)|`` over the wanted columns of all operators is
        below this (davidson's rule); otherwise the best block seen is returned with a ``ConvergenceWarning``
    nguard: int or None
        Guard vectors: the block has ``w = neig + nguard`` columns.  Default ``max(2, ceil(neig / 4))``
    precond: None, str, tensor or LinearOperator
        The preconditioner ``T`` of ``W = T R`` in ``davidson``'s grammar: ``"diag"`` / ``"jacobi"`` (``|diag A|^-1``),
        a diagonal ``d`` of shape ``(*batch, N)`` (``|d|^-1``), or a Hermitian positive definite operator such as
        ``fsai(A)``.  ``T`` must be positive definite: the diagonal forms are Jacobi's, not davidson's shifted one
    V0: tensor or None
        Start block ``(*batch, na, k)``; completed by random columns when ``k < neig + nguard``
    v_init, rng_device: str
        The start block, as for ``davidson`` (seed 12421)
    trace: dict or None
        Receives ``niter``, ``napply``, ``w``, ``resid_history`` (entry i: after i iterations), ``best_resid``,
        ``restarts``, ``redraws``, ``small_eigh`` (``"native"`` / ``"library"``), ``panel_kernel``

    ``process_group`` raises ``NotImplementedError``, and so does a block with ``3 w`` beyond the rows of the rotation
    kernel (``xk_lobpcg_max_rows()``: use ``chebfsi`` or ``davidson``).  ``mode="uppest"`` works on ``-A``.  A problem of
    order ``N <= max(5 w, 16)`` is handed to ``exacteig``.  A block that fails the a-posteriori guard
    ``max|X^H M X - I| > GUARD_BAD`` is never returned or kept: X is orthonormalised again, P is dropped (the next
    Rayleigh-Ritz problem has order ``2 w``) and the run goes on; more than ``GUARD_MAX_REDO`` such restarts raise.  A
    residual column without a direction (norm zero or not finite) is replaced by a random one, never divided by.  A
    Cholesky flag of the new directions reaches the host with the iteration's one status read, after the rotation:
    the iterate is discarded like a failed guard and the run restarts from the best block (the host twin, which sees
    the flag at once, redraws W with three passes instead); dependent START vectors are found on the small Gram
    matrix, drawn afresh and orthonormalised with three passes, and a second failure raises.

    Not built: locking / deflation of converged columns, batch sharding, an MFMA form of the rotation.
    """
    from xitorch_amd.linalg.native_eig import exacteig
    host_eig.refuse_nearest("lobpcg", mode)
    device = torch.device(A.device)
    if device.type == "cpu":
        # device dispatch (see native_eig.davidson): an operator in HOST memory is served by host_eig.py
        return host_eig.lobpcg(A, neig, mode, M, max_niter=max_niter, min_eps=min_eps, nguard=nguard, precond=precond,
                               V0=V0, v_init=v_init, rng_device=rng_device, verbose=verbose, trace=trace,
                               process_group=process_group)
    N, bdims, Bt, w, hand_over = host_eig._lob_setup(A, neig, M, nguard, V0, process_group)
    host_eig._lob_check_precond(precond)
    require_hip(A, "lobpcg")
    dtype = A.dtype
    if hand_over:
        if trace is not None:
            trace.update(niter=0, napply=0, w=w, handed_to="exacteig")
        return exacteig(A, neig, mode, M)
    if 3 * w > K.lobpcg_max_rows():
        raise NotImplementedError("lobpcg: a block of %d vectors is beyond the %d rows of the rotation kernel; use "
                                  "method='chebfsi' or method='davidson'" % (w, K.lobpcg_max_rows()))
    sign = 1.0 if mode == "lowest" else -1.0
    rdt = real_dtype(dtype)
    gbad = GUARD_BAD[rdt]
    op = PanelOperator(A, bdims, Bt, N)
    opM = PanelOperator(M, bdims, Bt, N) if M is not None else None
    if trace is not None and trace.get("k1_events") is not None:
        op.events = trace["k1_events"]
    pc = _preconditioner(precond, op, M, bdims, Bt, N, dtype, device)
    ops = block_ops(Bt, N, w, dtype, device, kmax=2 * w)
    blk = _Stacks(ops, neig, M is not None)
    S, AS, MS = blk.S, blk.AS, blk.MS
    best_X = blk.panels(1)
    spare = blk.panels(1)                  # random directions, drawn once: what replaces a column without a direction
    scratch = blk.panels(1) if pc is not None and pc[0] == "op" else None          # the preconditioner's output
    ndraw, redraws, restarts, nfail = 0, 0, 0, 0
    bad_cols = torch.zeros((), dtype=torch.int64, device=device)

    def random_into(dst):
        nonlocal ndraw
        ndraw += 1
        R = host_eig._lob_random(bdims, Bt, N, w, dtype, device, rng_device, ndraw)
        dst[:, :, :N].copy_(R)

    def chol_flag():
        return int(ops.info.max().item())

    def ritz_on_x():
        """Rayleigh-Ritz on X alone (rows [0, w)); the residual lands in rows [w, 2w)"""
        mu, Y = ops.eigh_lowest(ops.rr_matrix(S[:, :w], AS[:, :w], sign), w, w)
        lam = mu * sign
        blk.rotate(Y, lam, w, w)
        return lam

    # ---- start: M-orthonormal block, Rayleigh-Ritz on it alone
    random_into(spare)
    V0p = host_eig._cheb_start_block(v_init, V0, bdims, Bt, N, w, dtype, device, rng_device)
    ops.load(S[:, :w], V0p)
    ops.info.zero_()
    blk.orth(0, 2, opM)
    _, flag, guard = blk.status_read(w)
    if flag != 0 or not guard <= gbad:
        # dependent start vectors (the shifted first pass hides them from the Cholesky flag; the guard sees them): the
        # columns a Cholesky factorisation of the small Gram matrix (on the host) finds dependent are drawn afresh and
        # the block gets three passes; a second failure raises
        ops.load(S[:, :w], V0p)
        X0 = S[:, :w]
        if opM is not None:
            opM.apply(X0, MS[:, :w])
        G = ops.gram(X0, MS[:, :w] if opM is not None else X0)
        bad = lob_dependent_columns(G, rdt).to(device)
        redraws += int(bad.sum())
        X0.copy_(torch.where(bad[:, :, None], spare, X0))
        ops.info.zero_()
        blk.orth(0, 3, opM)
        if chol_flag() != 0:
            raise RuntimeError("lobpcg: the start block is rank deficient (linearly dependent start vectors)")
    del V0p
    op.apply(S[:, :w], AS[:, :w])
    lam = ritz_on_x()
    q = w                                   # rows of [X | P] in the stacks; the residual sits in rows [q, q + w)
    max_resid, flag, guard = blk.status_read(q)
    if not guard <= gbad:
        raise RuntimeError("lobpcg: the start block is not orthonormal (max|X^H M X - I| = %.2e)" % guard)

    best_resid, best_lam = float("inf"), None
    history = []
    niter = 0
    while True:
        if max_resid != max_resid:
            max_resid = float("inf")
        history.append(max_resid)
        if verbose:
            print("Iter %3d (block of %d): resid: %.3e" % (niter, w, max_resid))
        if max_resid < best_resid:
            best_resid, best_lam = max_resid, lam[:, :neig].clone()
            best_X.copy_(S[:, :w])
        if max_resid < min_eps or niter >= max_niter:
            break
        niter += 1
        R = S[:, q:q + w]
        # W = T R in place, columns scaled to unit norm; a column without a direction is replaced, never divided by
        if pc is None:
            nrm = torch.sqrt(blk.Pnorm.sum(dim=-1))
        else:
            if pc[0] == "diag":
                ops.precond_diag(R, pc[1])
            else:
                pc[1].apply(R, scratch)
                R.copy_(scratch)
            nrm = torch.linalg.vector_norm(R[:, :, :N], dim=-1).to(torch.float64)
        bad = ~(torch.isfinite(nrm) & (nrm > 0))
        bad_cols += bad.sum()
        inv = torch.where(bad, torch.ones_like(nrm), 1.0 / torch.where(bad, torch.ones_like(nrm), nrm)).to(rdt)
        R.mul_(inv[:, :, None])
        torch.where(bad[:, :, None], spare, R, out=R)
        ops.info.zero_()
        blk.orth(q, 2, opM)
        k = q + w
        op.apply(S[:, q:k], AS[:, q:k])
        mu, Cx = ops.eigh_lowest(ops.rr_matrix(S[:, :k], AS[:, :k], sign), k, w)   # T_S recomputed from the stacks
        lam = mu * sign
        C = torch.cat((Cx, lob_cp(Cx, w)), dim=-1)
        blk.rotate(C, lam, k, 2 * w)
        q = 2 * w
        max_resid, flag, guard = blk.status_read(q)
        if flag != 0:
            # W could not be orthonormalised: what the rotation made of it is discarded like a failed guard
            guard = float("inf")
        if not guard <= gbad:
            # never returned or kept: X is orthonormalised again, P dropped (the next problem has order 2 w)
            restarts += 1
            nfail += 1
            if nfail > GUARD_MAX_REDO:
                raise RuntimeError("xitorch_amd lobpcg: the block lost its orthonormality %d times (max|X^H M X - I| = "
                                   "%.2e, Cholesky flag %d, at iteration %d)" % (nfail, guard, int(flag), niter))
            ops.info.zero_()
            if flag != 0:
                # (the stacks hold combinations of a W that was not orthonormal: start again from the best block)
                S[:, :w].copy_(best_X)
            blk.orth(0, 3, opM)
            op.apply(S[:, :w], AS[:, :w])
            lam = ritz_on_x()
            q = w
            max_resid, flag, guard = blk.status_read(q)
            if flag != 0 or not guard <= gbad:
                raise RuntimeError("xitorch_amd lobpcg: the block could not be orthonormalised again (max|X^H M X - I| "
                                   "= %.2e, Cholesky flag %d, at iteration %d)" % (guard, int(flag), niter))
    if best_lam is None:
        raise RuntimeError("xitorch_amd lobpcg: no finite residual was produced")
    if not best_resid < min_eps:
        warnings.warn(ConvergenceWarning("lobpcg: convergence is not achieved after %d iterations (max |resid| = %.3e "
                                         ">= min_eps = %.3e); the best block is returned" % (niter, best_resid, min_eps)))
    if trace is not None:
        kernel = op.last_kernel if op.kind != "generic" else "generic"
        if dtype.is_complex and op.kind == "dense":
            kernel = "K1"
        trace.update(niter=niter, napply=op.napply, w=w, resid_history=history, best_resid=best_resid,
                     restarts=restarts, redraws=redraws + int(bad_cols.item()), small_eigh=ops.small_eigh,
                     panel_kernel=kernel, panel_buffers=blk.nalloc, torch_applies=op.torch_applies)
    evals = best_lam.to(rdt).reshape(*bdims, neig)
    evecs = ops.result(best_X, neig, bdims)
    if mode != "lowest":
        evals, evecs = evals.flip(-1), evecs.flip(-1)
    return evals, evecs
