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
from xitorch_amd.linalg._panel import PanelOperator, pad_len, real_dtype, require_hip
from xitorch_amd.linalg import host_eig
from xitorch_amd.linalg.host_eig import lob_cp, lob_dependent_columns

__all__ = ["lobpcg"]


class _Block:
    """the three stacks and what the iteration does to them; the subclasses supply the kernels of their dtype"""

    def __init__(self, Bt, N, w, neig, dtype, device, with_m):
        self.Bt, self.N, self.w, self.neig, self.dtype, self.device = Bt, N, w, neig, dtype, device
        self.rdtype = real_dtype(dtype)
        self.nalloc = 0                                   # panel buffers allocated, in units of (Bt, w, ld)
        self.S = self.stack()
        self.AS = self.stack()
        self.MS = self.stack() if with_m else None
        self.info = torch.zeros((Bt,), dtype=torch.int32, device=device)
        nblk = K.lobpcg_blocks(N, dtype)
        self.Pnorm = torch.zeros((Bt, w, nblk), dtype=torch.float64, device=device)
        self.Pmax = torch.zeros((Bt, nblk), dtype=torch.float64, device=device)
        self.small_eigh = "native"
        self.zero_lam = self.dabs = None                  # the Jacobi preconditioner's tables, made on first use

    def stack(self):
        self.nalloc += 3
        return torch.zeros((self.Bt, 3 * self.w, self.ld), dtype=self.dtype, device=self.device)

    def panel(self):
        self.nalloc += 1
        return torch.zeros((self.Bt, self.w, self.ld), dtype=self.dtype, device=self.device)

    def rows(self, stack, k0):
        return stack[:, k0:k0 + self.w]

    def rotate(self, C, lam, k, q):
        """the stacks' rows [0, q) <- their combinations by C (Bt, k, q); residual -> S rows [q, q + w)"""
        K.lobpcg_rotate(self.S, self.AS, self.MS, C, lam.to(torch.float64).contiguous(), k, q, self.w, N=self.N,
                        Pnorm=self.Pnorm, Pmax=self.Pmax)

    def resid_max(self, q):
        """(Bt,) float64: largest residual entry over the WANTED columns.  The kernel's Pmax covers all w columns of
        the block, so it serves only a block without guard vectors; otherwise one more read of the neig wanted
        residual rows (a max-norm reduction, no temporary panel)."""
        if self.neig == self.w:
            return self.Pmax.amax(dim=1)
        R = self.S[:, q:q + self.neig, :self.N]
        return torch.linalg.vector_norm(R, ord=float("inf"), dim=(1, 2)).to(torch.float64)

    def orth(self, k0, passes, opM):
        """rows [k0, k0 + w) of S M-orthonormal and M-orthogonal to rows [0, k0); with M the rows of MS follow (M is
        applied once).  The Cholesky flags land in self.info (sticky)."""
        raise NotImplementedError


class _RealBlock(_Block):
    """fp64 / fp32: zero-padded (Bt, 3w, pad_len(N)) stacks on the Davidson chain kernels"""

    def __init__(self, Bt, N, w, neig, dtype, device, with_m):
        self.ld = pad_len(N)
        super().__init__(Bt, N, w, neig, dtype, device, with_m)
        self.Cs = torch.empty((Bt * max(w, 32) * max(2 * w, 32),), dtype=dtype, device=device)
        self.Wq = torch.empty((Bt * 32 * 32,), dtype=dtype, device=device)
        self.rmax = torch.zeros((Bt,), dtype=dtype, device=device)
        self.orth_g = torch.zeros((Bt,), dtype=dtype, device=device)
        self.status = torch.zeros((5,), dtype=torch.float64, device=device)

    def load(self, V0p):
        self.S[:, :self.w, :self.N].copy_(V0p)

    def gram(self, Pa, Pb):
        """G[b, i, c] = <Pa_i, Pb_c>"""
        return K.dense_mm(Pa[:, :, :self.N], Pb[:, :, :self.N]).transpose(1, 2)

    def orth(self, k0, passes, opM):
        N, w = self.N, self.w
        if self.MS is None:
            K.davidson_orth(self.S, N, k0, w, self.Cs, self.Wq, self.info, passes=passes)
            return
        from xitorch_amd.linalg.native_eig import _shift_rel
        W, MW = self.rows(self.S, k0), self.rows(self.MS, k0)
        opM.apply(W, MW)
        Wq = self.Wq[:self.Bt * w * w].view(self.Bt, w, w)
        for r in range(passes):
            if k0 > 0:
                C = K.dense_mm(self.MS[:, :k0, :N], W[:, :, :N])             # C[b, c, a] = <M S_a, W_c>
                K.lincomb(self.S, C, W, k0, w, coef_layout="ca", alpha=-1.0, beta=1.0)
                K.lincomb(self.MS, C, MW, k0, w, coef_layout="ca", alpha=-1.0, beta=1.0)
            G = K.dense_mm(W[:, :, :N], MW[:, :, :N])
            if r == 0 and passes > 1:
                tr = torch.diagonal(G, dim1=-2, dim2=-1).sum(-1)
                G = G + (_shift_rel(N, w, self.dtype) * tr)[:, None, None] * torch.eye(w, dtype=G.dtype,
                                                                                         device=G.device)
            K.panel_chol(G, Wq, self.info, w)
            K.panel_transform(W, Wq, w)
            K.panel_transform(MW, Wq, w)

    def eigh(self, T, n, p):
        """(mu (Bt, p) ascending, Y (Bt, n, p)) of the symmetric (Bt, n, n) T on the native dense solvers"""
        from xitorch_amd.linalg.native_eig import native_partial_eigh
        if n >= 8:
            return native_partial_eigh(T, p, "lowest")
        mu, Yt, _ = K.small_eigh(T, n, p)                                    # LDS Jacobi kernel (tiny blocks)
        return mu, Yt.transpose(1, 2)

    def precond_diag(self, R, d):
        """R <- R / |d| (Jacobi; xk_diag_precond with a zero shift table)"""
        if self.zero_lam is None:
            self.zero_lam = torch.zeros((self.Bt, self.w), dtype=self.dtype, device=self.device)
            self.dabs = d.abs().contiguous()
        K.diag_precond(R, self.dabs, self.zero_lam, self.w)

    def status_read(self, q):
        """[max|resid| over the wanted columns, Cholesky flag, guard] of X = rows [0, w): the one host read"""
        self.rmax.copy_(self.resid_max(q))
        K.ritz_guard(self.S, self.orth_g, self.w, self.ld, MX=self.MS)
        K.group_status(self.rmax, self.info, None, self.status, orth=self.orth_g)
        st = self.status.tolist()
        return st[0], st[1], st[4]

    def result(self, X, bdims):
        return X[:, :self.neig, :self.N].transpose(-2, -1).reshape(*bdims, self.N, self.neig)


class _ComplexBlock(_Block):
    """complex128 / complex64: (Bt, 3w, N) stacks on the Hermitian Davidson kernels (xk_herm_*)"""

    def __init__(self, Bt, N, w, neig, dtype, device, with_m):
        self.ld = N
        super().__init__(Bt, N, w, neig, dtype, device, with_m)
        self.counts = {"rr_native": 0, "rr_library": 0}
        self.eye = torch.eye(w, dtype=dtype, device=device)

    def load(self, V0p):
        self.S[:, :self.w].copy_(V0p)

    def gram(self, Pa, Pb):
        from xitorch_amd.linalg.native_eig_herm import _gram
        return _gram(Pa, Pb)

    def orth(self, k0, passes, opM):
        from xitorch_amd.linalg.native_eig_herm import _shift_rel, _gram, _combine
        w = self.w
        W = self.rows(self.S, k0)
        MW = None
        if self.MS is not None:
            MW = self.rows(self.MS, k0)
            opM.apply(W, MW)
        for r in range(passes):
            if k0 > 0:
                C = _gram((self.MS if self.MS is not None else self.S)[:, :k0], W).contiguous()
                W.sub_(_combine(self.S[:, :k0], C))
                if MW is not None:
                    MW.sub_(_combine(self.MS[:, :k0], C))
            K.herm_cholqr(W, self.info, MW=MW,
                          shift_rel=_shift_rel(self.N, w, self.rdtype) if (r == 0 and passes > 1) else 0.0)

    def eigh(self, T, n, p):
        from xitorch_amd.linalg.native_eig_herm import herm_partial_eigh
        mu, Y = herm_partial_eigh(T, n, p, "lowest", self.counts)           # the library where chebfsi uses it: p > 16
        if self.counts["rr_library"]:
            self.small_eigh = "library"
        return mu, Y

    def precond_diag(self, R, d):
        """R <- R / |d| (Jacobi): the real kernel xk_diag_precond on the interleaved storage, every diagonal entry
        taken twice, with a zero shift table"""
        if self.zero_lam is None:
            self.zero_lam = torch.zeros((self.Bt, self.w), dtype=self.rdtype, device=self.device)
            self.dabs = d.abs().to(self.rdtype).repeat_interleave(2, dim=-1).contiguous()
        Rr = torch.view_as_real(R).reshape(R.shape[0], R.shape[1], 2 * R.shape[2])
        K.diag_precond(Rr, self.dabs, self.zero_lam, self.w)

    def status_read(self, q):
        X = self.S[:, :self.w]
        MX = self.MS[:, :self.w] if self.MS is not None else X
        guard = (self.gram(X, MX) - self.eye).abs().max().to(torch.float64)
        st = torch.stack((self.resid_max(q).max(), self.info.max().to(torch.float64), guard)).tolist()
        return st[0], st[1], st[2]

    def result(self, X, bdims):
        return X[:, :self.neig].transpose(-2, -1).reshape(*bdims, self.N, self.neig)


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
    from xitorch_amd.linalg.native_eig import exacteig, GUARD_BAD, GUARD_MAX_REDO, _preconditioner
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
    blk = (_ComplexBlock if dtype.is_complex else _RealBlock)(Bt, N, w, neig, dtype, device, M is not None)
    S, AS, MS = blk.S, blk.AS, blk.MS
    best_X = blk.panel()
    spare = blk.panel()                    # random directions, drawn once: what replaces a column without a direction
    scratch = blk.panel() if pc is not None and pc[0] == "op" else None            # the preconditioner's output
    ndraw, redraws, restarts, nfail = 0, 0, 0, 0
    bad_cols = torch.zeros((), dtype=torch.int64, device=device)

    def random_into(dst):
        nonlocal ndraw
        ndraw += 1
        R = host_eig._lob_random(bdims, Bt, N, w, dtype, device, rng_device, ndraw)
        dst[:, :, :N].copy_(R)

    def chol_flag():
        return int(blk.info.max().item())

    def ritz_on_x():
        """Rayleigh-Ritz on X alone (rows [0, w)); the residual lands in rows [w, 2w)"""
        T = blk.gram(S[:, :w], AS[:, :w])
        T = ((T + T.transpose(1, 2).conj()) * (0.5 * sign)).contiguous()
        mu, Y = blk.eigh(T, w, w)
        lam = mu * sign
        blk.rotate(Y, lam, w, w)
        return lam

    # ---- start: M-orthonormal block, Rayleigh-Ritz on it alone
    random_into(spare)
    V0p = host_eig._cheb_start_block(v_init, V0, bdims, Bt, N, w, dtype, device, rng_device)
    blk.load(V0p)
    blk.info.zero_()
    blk.orth(0, 2, opM)
    _, flag, guard = blk.status_read(w)
    if flag != 0 or not guard <= gbad:
        # dependent start vectors (the shifted first pass hides them from the Cholesky flag; the guard sees them): the
        # columns a Cholesky factorisation of the small Gram matrix (on the host) finds dependent are drawn afresh and
        # the block gets three passes; a second failure raises
        blk.load(V0p)
        X0 = S[:, :w]
        if opM is not None:
            opM.apply(X0, MS[:, :w])
        G = blk.gram(X0, MS[:, :w] if opM is not None else X0)
        bad = lob_dependent_columns(G, rdt).to(device)
        redraws += int(bad.sum())
        X0.copy_(torch.where(bad[:, :, None], spare, X0))
        blk.info.zero_()
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
                blk.precond_diag(R, pc[1])
            else:
                pc[1].apply(R, scratch)
                R.copy_(scratch)
            nrm = torch.linalg.vector_norm(R[:, :, :N], dim=-1).to(torch.float64)
        bad = ~(torch.isfinite(nrm) & (nrm > 0))
        bad_cols += bad.sum()
        inv = torch.where(bad, torch.ones_like(nrm), 1.0 / torch.where(bad, torch.ones_like(nrm), nrm)).to(rdt)
        R.mul_(inv[:, :, None])
        torch.where(bad[:, :, None], spare, R, out=R)
        blk.info.zero_()
        blk.orth(q, 2, opM)
        k = q + w
        op.apply(S[:, q:k], AS[:, q:k])
        T = blk.gram(S[:, :k], AS[:, :k])                 # recomputed from the stacks every iteration
        T = ((T + T.transpose(1, 2).conj()) * (0.5 * sign)).contiguous()
        mu, Cx = blk.eigh(T, k, w)
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
            blk.info.zero_()
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
                     restarts=restarts, redraws=redraws + int(bad_cols.item()), small_eigh=blk.small_eigh,
                     panel_kernel=kernel, panel_buffers=blk.nalloc, torch_applies=op.torch_applies)
    evals = best_lam.to(rdt).reshape(*bdims, neig)
    evecs = blk.result(best_X, bdims)
    if mode != "lowest":
        evals, evecs = evals.flip(-1), evecs.flip(-1)
    return evals, evecs
