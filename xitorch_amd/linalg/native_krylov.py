"""Linear solvers: dense `exactsolve` and the native (HIP) Krylov methods cg / bicgstab / gmres / minres.

Drop-in for the method functions of the reference (xitorch/_impls/linalg/solve.py): same names,
signatures ``f(A, B, E, M, **options) -> X``, options, stopping rule
(``all(|r_col| < max(rtol |b_col|, atol))``), best-iterate return (quirk Q10), true-residual
refresh every ``resid_calc_every`` iterations, ``_safedenom`` patching (Q9), normal-equation
fallback for ``posdef=False`` and ``ConvergenceWarning`` on non-convergence.

Every (batch member, column) pair is one *system*; all S = Bt*ncols systems advance in lock step.
Vectors live in padded (Bt, ncols, ld) panels (== (S, ld) arrays); per-system scalars never leave
the device; an iteration is a fixed sequence of fused kernels of libxitorch_amd.so
(xk_bicg_*, xk_cg_*, xk_kry_*) around the operator applies (xk_dense_mm / xk_banded_mm for the
native operators, the operator's own ``.mm`` otherwise) and ONE host sync (the stopping test).
With per-column shifts ``E`` the reference moves the columns to a leading axis (solve.py:575-604,
Q11); here the shift is simply a per-system scalar.
"""
import warnings
import torch
from xitorch_amd import kernels as K
from xitorch_amd._capi import NativeLibraryError, ptr, call
from xitorch_amd._util import pad_shapes, ConvergenceWarning
from xitorch_amd.linalg import host_krylov
from xitorch_amd.linalg.host_krylov import get_batchdims, zero_solution
from xitorch_amd.linalg._panel import PanelOperator, pad_len, batch_count, real_dtype, kry_blocks, require_hip, \
    to_panel, from_panel
from xitorch_amd.dist import allreduce_max_, all_ranks_agree_true

__all__ = ["exactsolve", "custom_exactsolve", "cg", "bicgstab", "gmres", "minres", "scipy_gmres", "broyden1_solve", "get_batchdims"]


def _in_host_memory(A):
    """Device dispatch (the reference runs a method on whatever device the operator lives on): operators in HOST memory
    are served by host_krylov.py; everything else — any device tensor — by the HIP kernels below and by nothing else:
    `_Problem` raises for a device it has no kernels for, `_capi.lib()` raises when the library is missing."""
    return torch.device(A.device).type == "cpu"


# ------------------------------------------------------------------------------- dense
def exactsolve(A, B, E, M):
    """Solve by building the full matrices (reference: exactsolve, solve.py:481-512)."""
    if E is None:
        return torch.linalg.solve(A.fullmatrix(), B)
    if M is None:
        return _solve_ABE(A.fullmatrix(), B, E)
    L = torch.linalg.cholesky(M.fullmatrix())
    Linv = torch.inverse(L)
    LinvH = Linv.transpose(-2, -1).conj()
    A2 = torch.matmul(Linv, A.mm(LinvH))
    X2 = _solve_ABE(A2, torch.matmul(Linv, B), E)
    return torch.matmul(LinvH, X2)


def _solve_ABE(A, B, E):
    """Column c solves (A - E_c I) x_c = b_c; columns become a leading batch axis
    (reference: _solve_ABE, solve.py:514-537, including the one jittered retry)."""
    na = A.shape[-1]
    BA, BB, BE = pad_shapes(A.shape[:-2], B.shape[:-2], E.shape[:-1])
    Ec = E.reshape(1, *BE, E.shape[-1]).transpose(0, -1)                 # (ncols, *BE, 1)
    Bc = B.reshape(1, *BB, *B.shape[-2:]).transpose(0, -1)               # (ncols, *BB, na, 1)
    AE = A - torch.diag_embed(Ec.repeat_interleave(repeats=na, dim=-1), dim1=-2, dim2=-1)
    try:
        r = torch.linalg.solve(AE, Bc)
    except torch._C._LinAlgError:
        eps = torch.finfo(A.dtype).eps
        jitter = 10 * eps * torch.max(AE.reshape(*AE.shape[:-2], -1), dim=-1)[0][..., None, None]
        AE = AE + torch.eye(na, dtype=A.dtype, device=A.device) * jitter
        r = torch.linalg.solve(AE, Bc)
    return r.transpose(0, -1).squeeze(0)


def custom_exactsolve(A, B, E=None, M=None, **options):
    return exactsolve(A, B, E, M)


# ------------------------------------------------------------------------------- problem set-up
class _Problem:
    """The linear problem in panel layout: apply(X) = A X - E * (M X), optionally the normal
    equations (reference: _setup_linear_problem, solve.py:560-643)."""

    def __init__(self, A, B, E, M, bdims, posdef, need_hermit):
        require_hip(A, "native solvers")
        self.dtype, self.device = A.dtype, torch.device(A.device)
        self.cplx = A.dtype.is_complex
        self.rdtype = real_dtype(A.dtype)         # element type of the kernels' scalars / partials
        self.bdims = list(bdims)
        self.N = A.shape[-1]
        self.nc = B.shape[-1]
        self.Bt = batch_count(self.bdims)
        self.ld = pad_len(self.N)
        self.S = self.Bt * self.nc
        self.opA = PanelOperator(A, self.bdims, self.Bt, self.N)
        self.opM = PanelOperator(M, self.bdims, self.Bt, self.N) if (M is not None and E is not None) else None
        self.E = None
        if E is not None:
            self.E = E.to(self.dtype).expand(*self.bdims, self.nc).reshape(self.Bt, self.nc).resolve_conj().contiguous()
        self._tmp = None
        self._tmp2 = None
        self._scratchP = None
        self.kr = _Kry(self)
        rhs = to_panel(B.to(self.dtype), self.bdims, self.Bt, self.N)

        hermit = A.is_hermitian and (M is None or M.is_hermitian)
        if need_hermit and not hermit:
            posdef = False                                            # solve.py:607-612
        if posdef is None:
            posdef = self._posdef_heuristic()
        self.normal = not posdef
        if self.normal:                                               # A -> A^H A, B -> A^H B (solve.py:637-643)
            rhs2 = self.new()
            self._apply1(rhs, rhs2, trans=True)
            rhs = rhs2
        self.rhs = rhs

    def new(self, n=None):
        return torch.zeros((self.Bt, self.nc if n is None else n, self.ld), dtype=self.dtype, device=self.device)

    def _shift_operand(self, X, trans):
        """Z of the shift term  - E * Z:  M X (or M^H X), or X itself when there is no M."""
        if self.opM is None:
            return X
        if self._tmp2 is None or self._tmp2.shape != X.shape:
            self._tmp2 = torch.zeros_like(X)
        self.opM.apply(X, self._tmp2, trans=trans)
        return self._tmp2

    def nblk(self):
        return kry_blocks(self.N, self.dtype)

    def _shift_now(self, out, Z):
        """out -= E * Z in place through xk_kry_dots' shift stage (its dot product goes to a scratch partial)."""
        if self._scratchP is None:
            self._scratchP = self.kr.partial()
        self.kr.dots(out, out, self._scratchP, shift=Z)

    def _apply1(self, X, out, trans=False, defer=False):
        """out = A X - E * (M X)  (solve.py:590-604).  defer=True leaves the shift to the caller's next
        xk_kry_dots launch, which applies it while it streams `out` anyway: returns the operand Z (or None)."""
        self.opA.apply(X, out, trans=trans)
        if self.E is None:
            return None
        Z = self._shift_operand(X, trans)
        if defer:
            return Z
        self._shift_now(out, Z)
        return None

    def apply(self, X, out, defer=False):
        """out = (A - E M) X, or the normal-equation operator.  With defer=True the return value, when not None,
        is the pending shift operand: pass it as `shift=` to the `_Kry.dots` call that follows."""
        if not self.normal:
            return self._apply1(X, out, defer=defer)
        if self._tmp is None or self._tmp.shape != X.shape:
            self._tmp = torch.zeros_like(X)
        self._apply1(X, self._tmp)
        self._apply1(self._tmp, out, trans=True)
        return None

    @property
    def napply(self):
        return self.opA.napply

    def _posdef_heuristic(self):
        # reference solve.py:617-634 + _get_largest_eival (:645-663): power iterations from an
        # (unseeded) random start; `largest` is a NORM, so this is "posdef unless the operator is 0" (Q8)
        x0 = torch.randn((self.Bt, self.nc, self.ld), dtype=self.dtype, device=self.device)
        x0[:, :, self.N:] = 0
        x0 = x0 / x0.norm(dim=-1, keepdim=True)

        def largest(fcn, x):
            prev = None
            for i in range(10):
                y = self.new()
                x = fcn(x, y)
                xn = x.norm(dim=-1, keepdim=True)
                if i > 0 and bool(torch.all(torch.abs(prev - xn) <= 1e-3 * xn + 1e-6)):
                    break
                prev = xn
                if i < 9:
                    x = x / xn
            return xn
        def op(x, y):
            self._apply1(x, y)
            return y
        big = largest(op, x0)
        neg = big <= 0
        if bool(torch.all(neg)):
            return False
        offset = torch.clamp(big, min=0.0)
        mostneg = largest(lambda x, y: op(x, y).sub_(offset * x), x0)
        return bool(torch.all(torch.logical_or(-mostneg <= offset, neg)).item())

    def solution(self, Xp):
        return from_panel(Xp, self.bdims, self.N)


class _Kry:
    """ctypes plumbing of the fused Krylov kernels on (S, ld) arrays (real or interleaved complex): S systems of
    length N and pitch ld, as any object with `S, N, ld, dtype, device` (and `E`, the per-system shifts, when `dots`
    is to fold them in) describes them.  `nblk` is the block count the kernels are launched with: `geom.nblk()` where
    the object has its own (a `_Problem`), else `kry_blocks(N, dtype)`."""

    def __init__(self, geom):
        self.S, self.N, self.ld = geom.S, geom.N, geom.ld
        self.dtype, self.device = geom.dtype, geom.device
        self.cplx, self.rdtype = geom.dtype.is_complex, real_dtype(geom.dtype)
        self.nblk = geom.nblk() if hasattr(geom, "nblk") else kry_blocks(geom.N, geom.dtype)
        self.E = getattr(geom, "E", None)
        self.status = torch.zeros((2,), dtype=torch.float64, device=self.device)
        self.rnorm = torch.zeros((self.S,), dtype=self.rdtype, device=self.device)

    def partial(self):
        """block partials of an inner product: (S, 64) real, or (S, 64, 2) for complex products"""
        shape = (self.S, 64, 2) if self.cplx else (self.S, 64)
        return torch.zeros(shape, dtype=self.rdtype, device=self.device)

    def partial_real(self):
        """block partials of |r|^2 (always real, consumed by xk_kry_status)"""
        return torch.zeros((self.S, 64), dtype=self.rdtype, device=self.device)

    def scalar(self, val=0.0):
        if not self.cplx:
            return torch.full((self.S,), val, dtype=self.dtype, device=self.device)
        t = torch.zeros((self.S, 2), dtype=self.rdtype, device=self.device)
        t[:, 0] = val
        return t

    def dots(self, x1, y1, P1, x2=None, y2=None, P2=None, shift=None, conj1=False):
        """partials of <x1,y1> (and <x2,y2>), <x,y> = sum conj(x) y; shift = Z: first y1 -= E * Z in the same pass
        (the `- M X E` term of the operator, solve.py:590-595, folded into the reduction that follows every apply);
        conj1 (complex only): P1 <- <y1,x1> instead."""
        extra = ((1 if conj1 else 0),) if self.cplx else ()
        call("xk_kry_dots", self.dtype, ptr(x1), ptr(y1), ptr(x2), ptr(y2), ptr(shift),
             ptr(self.E if shift is not None else None), ptr(P1), ptr(P2), self.S, self.N, self.ld, self.nblk, *extra)

    def bicg_p(self, r, p, v, Prho, rho_old, alpha, omega, rho_store, eps, first):
        call("xk_bicg_p", self.dtype, ptr(r), ptr(p), ptr(v), ptr(Prho), ptr(rho_old), ptr(alpha), ptr(omega),
             ptr(rho_store), self.S, self.N, self.ld, self.nblk, float(eps), 1 if first else 0)

    def bicg_s(self, r, v, s, rho, Pr0v, alpha, eps):
        call("xk_bicg_s", self.dtype, ptr(r), ptr(v), ptr(s), ptr(rho), ptr(Pr0v), ptr(alpha), self.S, self.N, self.ld,
             self.nblk, float(eps))

    def bicg_final(self, x, xout, yd, zd, s, t, r, r0, alpha, Pts, Ptt, omega, Prr, Prho, eps, skip_r):
        call("xk_bicg_final", self.dtype, ptr(x), ptr(xout), ptr(yd), ptr(zd), ptr(s), ptr(t), ptr(r), ptr(r0),
             ptr(alpha), ptr(Pts), ptr(Ptt), ptr(omega), ptr(Prr), ptr(Prho), self.S, self.N, self.ld, self.nblk,
             float(eps), 1 if skip_r else 0)

    def resid(self, b, y, r, r0, Prr, Prho, init=False):
        """r = b - y with partials |r|^2 -> Prr (real) and <r0, r> -> Prho; init=True: only the partials of the
        vector `b` itself (y is taken as zero: the kernel is run with y = a zero panel and a scratch r)."""
        if init:
            if getattr(self, "_zero", None) is None or self._zero.shape != b.shape:
                self._zero = torch.zeros_like(b)
            y, r = self._zero, torch.empty_like(b)
        call("xk_kry_resid", self.dtype, ptr(b), ptr(y), ptr(r), ptr(r0), ptr(Prr), ptr(Prho), self.S, self.N, self.ld,
             self.nblk)

    def cg_update(self, x, xout, p, Ap, r, Prz, PpAp, Prr, eps, skip_r):
        call("xk_cg_update", self.dtype, ptr(x), ptr(xout), ptr(p), ptr(Ap), ptr(r), ptr(Prz), ptr(PpAp), ptr(Prr),
             self.S, self.N, self.ld, self.nblk, float(eps), 1 if skip_r else 0)

    def cg_p(self, z, p, Prz_new, Prz_old, eps):
        call("xk_cg_p", self.dtype, ptr(z), ptr(p), ptr(Prz_new), ptr(Prz_old), self.S, self.N, self.ld, self.nblk,
             float(eps))

    def check_status(self, Prr, stop, process_group=None, nblk=None):
        """-> (max residual norm over all systems, number of unconverged systems): the one host sync.
        nblk: partials per system held by Prr (default: the block count of the vector kernels)."""
        call("xk_kry_status", self.rdtype, ptr(Prr), ptr(stop), ptr(self.rnorm), ptr(self.status), self.S,
             self.nblk if nblk is None else nblk)
        # MAX over the ranks of both entries: max residual, and "someone is unconverged" (count > 0)
        allreduce_max_(self.status, process_group)
        mx, nbad = self.status.tolist()
        return mx, nbad


class _Run:
    """What cg / bicgstab / gmres / minres share around their loops.  Before: device dispatch (an operator in host
    memory goes to the method of the same name in host_krylov.py), the `max_niter` default, the zero right-hand side
    shortcut, the problem in panel layout with its kernels and the stopping vector.  After: the trace, the warning and
    the solution in the caller's layout.  `X` is the result when there is nothing (left) to iterate on, else None."""

    def __init__(self, method, A, B, E, M, opt, posdef, need_hermit, niter_factor=1.5):
        self.X = self.prob = None
        if _in_host_memory(A):
            self.X = getattr(host_krylov, method)(A, B, E, M, **opt)
            return
        self.trace, self.process_group = opt["trace"], opt["process_group"]
        self.max_niter = int(niter_factor * A.shape[-1]) if opt["max_niter"] is None else opt["max_niter"]
        bdims = get_batchdims(A, B, E, M)
        # (sharded runs: every rank takes this shortcut or none does — the loops contain collectives)
        if all_ranks_agree_true(torch.allclose(B, B * 0, rtol=opt["rtol"], atol=opt["atol"]), B.device,
                                self.process_group):
            self.X = zero_solution(A, B, bdims)
            return
        self.prob = _Problem(A, B, E, M, bdims, posdef, need_hermit)
        if self.trace is not None and self.trace.get("k1_events") is not None:
            self.prob.opA.events = self.trace["k1_events"]      # measurement: HIP events around every operator apply
        self.kr = self.prob.kr
        bnorm = self.prob.rhs.norm(dim=-1).reshape(-1)
        self.stop = torch.max(opt["rtol"] * bnorm, opt["atol"] * torch.ones_like(bnorm)).contiguous()

    def finish(self, Xp, converged, best, niter, said_niter, resid="resid", **more):
        """Xp: the panel of the iterate to return"""
        if self.trace is not None:
            self.trace.update(niter=niter, napply=self.prob.napply, converged=converged, best_resid=best, **more)
        if not converged:
            warnings.warn(ConvergenceWarning("Convergence is not achieved after %d iterations. "
                                             "Max norm of %s: %.3e" % (said_niter, resid, best)))
        return self.prob.solution(Xp)


def _precond(P, prob):
    if P is None:
        return None
    from xitorch_amd.linop import LinearOperator
    if not isinstance(P, LinearOperator):
        raise TypeError("precond can only be LinearOperator or None")
    return PanelOperator(P, prob.bdims, prob.Bt, prob.N)


class _XRing:
    """Three rotating solution buffers: current, next, and whichever holds the best iterate —
    best-iterate tracking (solve.py:157-160, 300-303) without copying."""

    def __init__(self, prob):
        self.bufs = [prob.new() for _ in range(3)]
        self.cur, self.best = 0, 0

    def next_index(self):
        for i in range(3):
            if i != self.cur and i != self.best:
                return i
        raise AssertionError


# ------------------------------------------------------------------------------- BiCGStab
def bicgstab(A, B, E=None, M=None, posdef=None, precond_l=None, precond_r=None, max_niter=None,
             rtol=1e-6, atol=1e-8, eps=1e-12, verbose=False, resid_calc_every=10, process_group=None,
             trace=None, **unused):
    r"""
    Solve the linear equations using the stabilized Biconjugate-Gradient method on HIP kernels.

    Keyword arguments
    -----------------
    posdef: bool or None
        Whether :math:`\mathbf{AX-MXE}` is positive definite for all columns and batches; ``None``
        runs the reference's power-iteration heuristic; ``False`` solves the normal equations
    precond_l, precond_r: LinearOperator or None
        Left / right preconditioners
    max_niter: int or None
        Maximum number of iterations (default ``int(1.5 * A.shape[-1])``)
    rtol, atol: float
        Relative / absolute tolerance of the stopping condition w.r.t. the norm of B
    eps: float
        Replacement of exact zeros in denominators
    resid_calc_every: int
        Recompute the true residual with this period (0: never)
    verbose: bool
        Print the progress
    process_group: torch.distributed group or None
        (extension) batch-sharded multi-GPU run: the stopping test is all-reduced over the group
    """
    run = _Run("bicgstab", A, B, E, M, dict(
        posdef=posdef, precond_l=precond_l, precond_r=precond_r, max_niter=max_niter, rtol=rtol, atol=atol, eps=eps,
        verbose=verbose, resid_calc_every=resid_calc_every, process_group=process_group, trace=trace), posdef, False)
    if run.X is not None:
        return run.X
    prob, kr, stop, max_niter = run.prob, run.kr, run.stop, run.max_niter
    pl, pr = _precond(precond_l, prob), _precond(precond_r, prob)

    r = prob.rhs.clone()                      # x0 = 0  ->  r = B - A 0 = B (solve.py:262)
    r0 = r.clone()
    p, v, s, t = prob.new(), prob.new(), prob.new(), prob.new()
    y = prob.new() if pr is not None else p
    z = prob.new() if pr is not None else s
    Kt = prob.new() if pl is not None else t
    Ks = prob.new() if pl is not None else s
    tmp = prob.new()
    ring = _XRing(prob)
    Prho, Pr0v, Pts, Ptt = (kr.partial() for _ in range(4))
    Prr = kr.partial_real()
    rho = [kr.scalar(), kr.scalar()]
    alpha, omega = kr.scalar(1.0), kr.scalar(1.0)

    kr.resid(r, None, None, r0, Prr, Prho, init=True)              # |r|^2 and <r0, r> of the initial residual
    best, _ = kr.check_status(Prr, stop, process_group)
    converged = False
    niter = 0
    for k in range(1, max_niter + 1):
        niter = k
        kr.bicg_p(r, p, v, Prho, rho[(k + 1) % 2], alpha, omega, rho[k % 2], eps, first=(k == 1))
        if pr is not None:
            pr.apply(p, y)
        sh = prob.apply(y, v, defer=True)
        kr.dots(r0, v, Pr0v, shift=sh)
        kr.bicg_s(r, v, s, rho[k % 2], Pr0v, alpha, eps)
        if pr is not None:
            pr.apply(s, z)
        sh = prob.apply(z, t, defer=(pl is None))
        if pl is not None:
            pl.apply(t, Kt)
            pl.apply(s, Ks)
        kr.dots(Ks, Kt, Pts, Kt, Kt, Ptt, shift=sh, conj1=True)    # <t, s> (solve.py:286) and <t, t>
        refresh = resid_calc_every != 0 and k % resid_calc_every == 0
        nxt = ring.next_index()
        kr.bicg_final(ring.bufs[ring.cur], ring.bufs[nxt], y, z, s, t, r, r0, alpha, Pts, Ptt, omega, Prr, Prho,
                      eps, skip_r=refresh)
        ring.cur = nxt
        if refresh:                                                # solve.py:290-291
            prob.apply(ring.bufs[nxt], tmp)
            kr.resid(prob.rhs, tmp, r, r0, Prr, Prho)
        mx, nbad = kr.check_status(Prr, stop, process_group)
        if mx < best:
            best, ring.best = mx, nxt
        if verbose and (k < 10 or k % 10 == 0):
            print("%4d: |dy|=%.3e" % (k, mx))
        if nbad == 0:
            converged = True
            break
    return run.finish(ring.bufs[ring.best], converged, best, niter, max_niter)


# ------------------------------------------------------------------------------- CG
def cg(A, B, E=None, M=None, posdef=None, precond=None, max_niter=None, rtol=1e-6, atol=1e-8, eps=1e-12,
       resid_calc_every=10, verbose=False, process_group=None, trace=None, **unused):
    r"""
    Solve the linear equations using the Conjugate-Gradient (CG) method on HIP kernels.

    Keyword arguments
    -----------------
    posdef: bool or None
        Whether :math:`\mathbf{AX-MXE}` is positive definite for all columns and batches; ``None``
        runs the reference's power-iteration heuristic; ``False`` (forced for non-Hermitian
        operators) solves the normal equations
    precond: LinearOperator or None
        Preconditioner
    max_niter: int or None
        Maximum number of iterations (default ``int(1.5 * A.shape[-1])``)
    rtol, atol: float
        Relative / absolute tolerance of the stopping condition w.r.t. the norm of B
    eps: float
        Replacement of exact zeros in denominators
    resid_calc_every: int
        Recompute the true residual with this period (0: never)
    verbose: bool
        Print the progress
    process_group: torch.distributed group or None
        (extension) batch-sharded multi-GPU run: the stopping test is all-reduced over the group
    """
    run = _Run("cg", A, B, E, M, dict(
        posdef=posdef, precond=precond, max_niter=max_niter, rtol=rtol, atol=atol, eps=eps,
        resid_calc_every=resid_calc_every, verbose=verbose, process_group=process_group, trace=trace), posdef, True)
    if run.X is not None:
        return run.X
    prob, kr, stop, max_niter = run.prob, run.kr, run.stop, run.max_niter
    pre = _precond(precond, prob)

    r = prob.rhs.clone()
    z = prob.new() if pre is not None else r
    if pre is not None:
        pre.apply(r, z)
    p = z.clone()
    Ap, tmp = prob.new(), prob.new()
    ring = _XRing(prob)
    Prz = [kr.partial(), kr.partial()]
    PpAp, Prr = kr.partial(), kr.partial_real()
    kr.resid(r, None, None, None, Prr, None, init=True)            # |r|^2 of the initial residual
    kr.dots(r, z, Prz[0])
    best, _ = kr.check_status(Prr, stop, process_group)
    converged = False
    cur = 0
    niter = 0
    for k in range(1, max_niter + 1):
        niter = k
        sh = prob.apply(p, Ap, defer=True)
        kr.dots(p, Ap, PpAp, shift=sh)
        refresh = resid_calc_every != 0 and k % resid_calc_every == 0
        nxt = ring.next_index()
        kr.cg_update(ring.bufs[ring.cur], ring.bufs[nxt], p, Ap, r, Prz[cur], PpAp, Prr, eps, skip_r=refresh)
        ring.cur = nxt
        if refresh:                                                # solve.py:148-149
            prob.apply(ring.bufs[nxt], tmp)
            kr.resid(prob.rhs, tmp, r, None, Prr, None)
        mx, nbad = kr.check_status(Prr, stop, process_group)
        if mx < best:
            best, ring.best = mx, nxt
        if verbose and (k < 10 or k % 10 == 0):
            print("%4d: |dy|=%.3e" % (k, mx))
        if nbad == 0:
            converged = True
            break
        if pre is not None:
            pre.apply(r, z)
        kr.dots(r, z, Prz[1 - cur])
        kr.cg_p(z, p, Prz[1 - cur], Prz[cur], eps)
        cur = 1 - cur
    return run.finish(ring.bufs[ring.best], converged, best, niter, max_niter, resid="best resid")


# ------------------------------------------------------------------------------- GMRES
class _GmresState:
    """Everything of GMRES that grows with the Krylov basis, on the device: the basis Q (S, cap, ld) and the coefficient
    row `ycoef` of the iterate in the vector dtype; the per-system Hessenberg / Givens state R, cs, sn, g for cap - 1
    columns (float64 whatever the vector dtype; complex: R, sn, g are complex128, interleaved pairs for
    xk_gmres_*_c*, cs stays real); complex only, the coefficient rows c1, c2n of the two Gram passes and the scratch of
    xk_gmres_gram_c*' fixed-shape reduction, one double pair per (system, tile, row).  (The reference preallocates
    max_niter vectors and a (max_niter+1) x max_niter Hessenberg, solve.py:384-386, Q12.)"""

    def __init__(self, S, N, ld, dtype, device, cap):
        self.S, self.ld, self.dtype, self.device = S, ld, dtype, device
        self.gtiles = K.gmres_gram_tiles(N, dtype) if dtype.is_complex else 0
        self.cap = 0
        self.grow(cap)

    def grow(self, cap):
        """storage for `cap` basis vectors, the first `self.cap` kept"""
        S, old, hc, ho = self.S, self.cap, cap - 1, self.cap - 1
        zdtype = torch.complex128 if self.dtype.is_complex else torch.float64
        z = lambda dt, *shape: torch.zeros(shape, dtype=dt, device=self.device)
        Q = z(self.dtype, S, cap, self.ld)
        R, cs, sn, g = z(zdtype, S, hc + 1, hc), z(torch.float64, S, hc), z(zdtype, S, hc), z(zdtype, S, hc + 1)
        if old:
            Q[:, :old].copy_(self.Q)
            R[:, :ho + 1, :ho] = self.R
            cs[:, :ho], sn[:, :ho], g[:, :ho + 1] = self.cs, self.sn, self.g
        self.Q, self.R, self.cs, self.sn, self.g, self.cap, self.hcap = Q, R, cs, sn, g, cap, hc
        self.ycoef = z(self.dtype, S, 1, cap)
        if self.dtype.is_complex:
            self.c1, self.c2n = z(self.dtype, S, cap + 1), z(self.dtype, S, cap + 1)
            self.gscr = z(torch.float64, S * self.gtiles * (cap + 1) * 2)


def gmres(A, B, E=None, M=None, posdef=None, max_niter=None, rtol=1e-6, atol=1e-8, eps=1e-12,
          resid_calc_every=1, restart=None, process_group=None, trace=None, precond_r=None, **unused):
    r"""
    Solve the linear equations using the Generalised minimal residual method on HIP kernels
    (reference: gmres, xitorch/_impls/linalg/solve.py:326-433).  Real and complex operators (extension: the reference's
    gmres is real-only); for complex dtypes inner products are ``<x, y> = sum conj(x) y``, the Hessenberg matrix and
    the Givens sines are complex, and the basis work runs on ``xk_gmres_gram_c*`` / ``xk_lincomb_c*`` /
    ``xk_gmres_*_c*`` in place of the real kernels named below.

    Same iterates, same stopping rule and same return value as the reference: un-restarted GMRES from ``x0 = 0``;
    after ``k`` Arnoldi steps the iterate ``x_k`` minimises the residual over the ``k``-dimensional Krylov space; the
    TRUE residual ``B - (A x_k - M x_k E)`` decides convergence (``all(|r_col| < max(rtol |b_col|, atol))``) and
    which iterate is the best one (smallest maximum residual norm over all batches and columns, solve.py:414-425);
    the best iterate is returned, with a ``ConvergenceWarning`` when the tolerance was not reached.  Like the
    reference's loop (``for k in range(min(nr, max_niter))`` solving with the first ``k`` columns, :389,403-410) at most
    ``min(nr, max_niter) - 1`` Krylov vectors contribute.

    How it runs here: the Krylov basis of every system is kept panel-major on the device and grows by one vector per
    iteration; the new direction is orthogonalised by classical Gram-Schmidt applied twice (two Gram products on
    the K1 kernel, ``xk_lincomb`` / ``xk_gmres_finish`` — the reference's modified Gram-Schmidt, :391-393, is a
    sequential chain of k dot / axpy pairs); the Hessenberg column, its Givens rotations and the rotated right-hand
    side live on the device (``xk_gmres_step``), so the least-squares problem the reference hands to
    ``torch.linalg.lstsq`` every iteration (:403) is one back substitution (``xk_gmres_solve``); its residual
    ``|g[k+1]|`` equals the true residual norm in exact arithmetic.  One host read per iteration.

    Keyword arguments
    -----------------
    posdef: bool or None
        As for :func:`bicgstab`
    max_niter: int or None
        Maximum number of iterations (default ``A.shape[-1]``)
    rtol, atol: float
        Relative / absolute tolerance of the stopping condition w.r.t. the norm of B
    eps: float
        Replacement of exact zeros in denominators
    resid_calc_every: int
        (extension) ``1`` (default): the iterate and its true residual are formed every iteration, exactly like the
        reference.  ``n > 1``: only every n-th iteration, on the last one, and whenever the least-squares estimate
        says that every system has converged (one more operator apply and one pass over the basis saved per skipped
        iteration; stopping decisions are still taken on true residuals only, best-iterate tracking sees the
        checked iterates).
    restart: int or None
        (extension) ``None`` (default): un-restarted, like the reference, whose Krylov basis grows until ``max_niter``
        (solve.py:384-389: it preallocates ``max_niter`` vectors).  An integer ``m``: GMRES(m) — after ``m`` Arnoldi steps
        the iterate and its true residual are formed, the basis is dropped and the next cycle starts from that residual
        (memory ``m + 1`` vectors per system instead of ``max_niter``; lets systems that need more steps than fit
        reach a tight ``rtol``).  Stopping rule and best-iterate rule are unchanged and run across the cycles; ``max_niter``
        bounds the total number of steps.
    process_group: torch.distributed group or None
        (extension) batch-sharded multi-GPU run: the stopping test is all-reduced over the group
    precond_r: LinearOperator or None
        (extension) right preconditioner ``P``: the Krylov space is that of ``A P`` (one more panel apply per Arnoldi
        step, ``w = A (P q_j)``) and the iterate is ``x_base + P (Q y)``; the residual of the right-preconditioned
        system is the true residual of the original one, so the stopping rule, the best-iterate rule and every other
        option are untouched.  Refused (``ValueError``) when the problem resolves to the normal equations: a
        preconditioner of ``A`` is not one of ``A^H A``.  ``linalg.fsai_lu(A)`` makes one for a sparse ``A``.

    With ``E`` the reference returns its column-swapped work layout ``(ncols, *batch, nr, 1)`` without undoing the
    swap (:432, and fails for more than one column); this function returns ``(*batch, nr, ncols)`` like every other
    method.
    """
    run = _Run("gmres", A, B, E, M, dict(
        posdef=posdef, max_niter=max_niter, rtol=rtol, atol=atol, eps=eps, resid_calc_every=resid_calc_every,
        restart=restart, process_group=process_group, trace=trace, precond_r=precond_r), posdef, False, niter_factor=1)
    if run.X is not None:
        return run.X
    prob, kr, stop, max_niter = run.prob, run.kr, run.stop, run.max_niter
    pr = _precond(precond_r, prob)
    if pr is not None and prob.normal:
        raise ValueError("gmres: precond_r cannot be used when the normal equations are solved (posdef=False): a "
                         "preconditioner of A is not one of A^H A")
    nr = A.shape[-1]
    S, N, ld = prob.S, prob.N, prob.ld
    dtype, dev = prob.dtype, prob.device
    every = max(1, int(resid_calc_every))
    msteps = min(nr, max_niter) - 1           # Arnoldi steps whose column enters an iterate (solve.py:389,403)
    if restart is not None:
        restart = int(restart)
        if restart < 1:
            raise ValueError("gmres: restart must be a positive number of Arnoldi steps, got %d" % restart)
        msteps = max_niter - 1 if max_niter > 1 else 0      # (restarted: the total is not bounded by the order)
    mcyc = msteps if restart is None else min(restart, max(msteps, 1))     # Arnoldi steps per cycle
    lazy_limit = None
    kd_max = 4096 if prob.cplx else 8192      # 64 KiB of LDS / (16 B | 8 B) per entry of y
    if mcyc > kd_max:
        # xk_gmres_solve keeps the least-squares solution of a system in LDS: at most 8192 (complex: 4096) basis vectors
        # per cycle (the dense Hessenberg of such a run is 8 S k^2 bytes long before that).  An explicit restart length
        # beyond it is refused here; the un-restarted default (max_niter = None -> the operator's order, solve.py:389) only fails if
        # a run really gets that far — almost every run converges in a few dozen steps whatever the order
        if restart is not None:
            raise NativeLibraryError("xitorch_amd gmres: restart=%d exceeds the supported cycle length (%d basis "
                                     "vectors per system)" % (restart, kd_max))
        lazy_limit, mcyc = kd_max, kd_max
    rhs = prob.rhs.reshape(S, ld)
    beta = rhs.norm(dim=-1)                                                      # (S,)
    best = float(allreduce_max_(beta.max().double().reshape(1), process_group).item())      # solve.py:380-381
    xbufs = [torch.zeros((S, 1, ld), dtype=dtype, device=dev) for _ in range(2)]
    best_i, cur_i = 0, 1                      # xbufs[0] = x0 = 0 is the best iterate so far (:382)
    converged = False
    nsteps, nsync, ncycles = 0, 1, 0
    if msteps > 0:
        x_base = None                         # restarted cycles: the iterate the current cycle corrects
        st = _GmresState(S, N, ld, dtype, dev, min(mcyc + 1, 32))
        st.Q[:, 0] = rhs / torch.where(beta == 0, torch.full_like(beta, eps), beta).unsqueeze(-1)   # :385, _safedenom
        st.g[:, 0] = beta.double()
        inv_hn = torch.zeros((S,), dtype=prob.rdtype, device=dev)
        Pest, Ptrue = kr.partial_real(), kr.partial_real()
        status4 = torch.zeros((4,), dtype=torch.float64, device=dev)
        tmp = prob.new()
        rtrue = prob.new()
        pq = prob.new() if pr is not None else None                  # P q_j, and Q y before P is applied to it

        def status_of(Prr, nblk, slot):
            call("xk_kry_status", kr.rdtype, ptr(Prr), ptr(stop), ptr(kr.rnorm), ptr(status4[2 * slot:]), S, nblk)

        def true_residual(kd):
            """x = Q y with R y = g (the reference's lstsq solution, :403-410), r = B - A x (:414): partials -> Ptrue"""
            call("xk_gmres_solve", dtype, ptr(st.R), ptr(st.g), ptr(st.ycoef), st.ycoef.stride(0), S, kd, st.hcap)
            x = xbufs[cur_i]
            qy = x if pr is None else pq.reshape(S, 1, ld)
            if prob.cplx:
                K.lincomb_c(st.Q, st.ycoef, qy, kd, 1, alpha=1.0, beta=0.0, N=N)
            else:
                K.lincomb(st.Q, st.ycoef, qy, kd, 1, coef_layout="ca", alpha=1.0, beta=0.0)
            if pr is not None:
                pr.apply(pq, x.reshape(prob.Bt, prob.nc, ld))                  # x = P (Q y)
            if x_base is not None:
                x.add_(x_base)
            prob.apply(x.reshape(prob.Bt, prob.nc, ld), tmp)
            kr.resid(prob.rhs, tmp, rtrue, None, Ptrue, None)
            status_of(Ptrue, kr.nblk, 1)

        cyc0 = 0                              # global index of the current cycle's first Arnoldi step
        for k in range(msteps):
            j = k - cyc0                                              # step index inside the cycle
            if lazy_limit is not None and j >= lazy_limit:
                raise NativeLibraryError("xitorch_amd gmres: the un-restarted Krylov basis reached %d vectors per system "
                                         "without converging (best residual %.3e); pass restart=m (GMRES(m)) or a "
                                         "max_niter <= %d" % (lazy_limit, best, lazy_limit + 1))
            nsteps = k + 1
            if j + 2 > st.cap:
                st.grow(min(mcyc + 1, 2 * st.cap))
            Q = st.Q
            # w = A q_j (solve.py:390) straight into basis row j+1; with a shift E the fused shift kernel wants
            # contiguous (S, ld) arrays, so q_j / w pass through two contiguous buffers (O(N) copies)
            if pr is not None:
                # right preconditioning: w = A (P q_j), through the contiguous scratch panel
                pr.apply(Q[:, j].reshape(prob.Bt, prob.nc, ld), pq)
                if prob.E is None:
                    prob.apply(pq, Q[:, j + 1].reshape(prob.Bt, prob.nc, ld))
                else:
                    prob.apply(pq, tmp)
                    Q[:, j + 1].copy_(tmp.reshape(S, ld))
            elif prob.E is None:
                prob.apply(Q[:, j].reshape(prob.Bt, prob.nc, ld), Q[:, j + 1].reshape(prob.Bt, prob.nc, ld))
            else:
                rtrue.reshape(S, ld).copy_(Q[:, j])
                prob.apply(rtrue, tmp)
                Q[:, j + 1].copy_(tmp.reshape(S, ld))
            wrow = Q[:, j + 1:j + 2]
            if prob.cplx:
                c1, c2n = st.c1, st.c2n
                K.gmres_gram_c(Q, Q[:, j + 1], c1, st.gscr, j + 1, N)              # c1[s, i] = <q_i, w>, i <= j
                K.lincomb_c(Q, c1.unsqueeze(1), wrow, j + 1, 1, alpha=-1.0, beta=1.0, N=N)
                K.gmres_gram_c(Q, Q[:, j + 1], c2n, st.gscr, j + 1, N)             # second pass; entry j+1 = |w1|^2
            else:
                c1 = K.dense_mm(Q[:, :j + 1, :N], wrow[:, :, :N])                  # (S, 1, j+1): <q_i, w>
                K.lincomb(Q, c1, wrow, j + 1, 1, coef_layout="ca", alpha=-1.0, beta=1.0)
                c2n = K.dense_mm(Q[:, :j + 2, :N], wrow[:, :, :N])                 # second pass; last entry |w1|^2
            call("xk_gmres_step", dtype, ptr(c1), c1.stride(0), ptr(c2n), c2n.stride(0), j, st.hcap, ptr(st.R),
                 ptr(st.cs), ptr(st.sn), ptr(st.g), ptr(inv_hn), ptr(Pest), S)
            call("xk_gmres_finish", dtype, ptr(Q), ptr(c2n), c2n.stride(0), ptr(inv_hn), S, N, j, Q.stride(1),
                 Q.stride(0))
            status_of(Pest, 1, 0)
            cycle_end = restart is not None and j + 1 == mcyc
            checked = (k + 1) % every == 0 or k == msteps - 1 or cycle_end
            if checked:
                true_residual(j + 1)
            allreduce_max_(status4, process_group)
            est_mx, est_bad, tr_mx, tr_bad = status4.tolist()                      # the iteration's host read
            nsync += 1
            if not checked and est_bad == 0:
                # the least-squares residual says every system is done: decide on the true residual, like the
                # reference does every iteration; from here on every iterate is checked
                true_residual(j + 1)
                allreduce_max_(status4, process_group)
                est_mx, est_bad, tr_mx, tr_bad = status4.tolist()
                nsync += 1
                checked, every = True, 1
            just = cur_i                                                            # buffer of the iterate just formed
            if checked:
                if tr_mx < best:                                                    # solve.py:417-421
                    best = tr_mx
                    best_i, cur_i = cur_i, best_i
                if tr_bad == 0:                                                     # :423-425
                    converged = True
                    break
            if cycle_end and k < msteps - 1:
                # GMRES(m): the next cycle corrects the iterate just formed, starting from its TRUE residual
                if x_base is None:
                    x_base = torch.zeros((S, 1, ld), dtype=dtype, device=dev)
                x_base.copy_(xbufs[just])
                rcur = rtrue.reshape(S, ld)
                beta = rcur.norm(dim=-1)
                st.Q[:, 0] = rcur / torch.where(beta == 0, torch.full_like(beta, eps), beta).unsqueeze(-1)
                for t in (st.R, st.cs, st.sn, st.g):
                    t.zero_()
                st.g[:, 0] = beta.double()
                cyc0 = k + 1
                ncycles += 1
    # niter counts like the reference's loop: the pass that tests x_k is pass k + 1
    return run.finish(xbufs[best_i].reshape(prob.Bt, prob.nc, ld), converged, best, nsteps + 1, max_niter,
                      arnoldi_steps=nsteps, host_syncs=nsync, restarts=ncycles)


# ------------------------------------------------------------------------------- MINRES
def minres(A, B, E=None, M=None, precond=None, max_niter=None, rtol=1e-6, atol=1e-8, max_restart=2, verbose=False,
           process_group=None, trace=None, **unused):
    r"""
    Solve the linear equations with the minimal residual method MINRES (Paige & Saunders 1975) on HIP kernels
    (extension: the reference has no MINRES).

    For Hermitian operators :math:`\mathbf{A} - e_c \mathbf{M}` that may be indefinite, or singular with a
    consistent right-hand side (the shifted systems of the ``symeig`` backward): one operator apply per iteration, a
    three-term recurrence (constant storage), a residual norm that never grows, and, from ``x0 = 0``, the minimum-norm
    solution of a consistent singular system.  An exactly vanishing Lanczos norm freezes its system (exact
    convergence); no denominator is ever replaced by an ``eps``.

    Stopping rule, per system: :math:`|r| \le \max(\mathrm{rtol}\,|b|, \mathrm{atol})`, evaluated on the recurrence
    value :math:`\bar\phi` (equal to :math:`|b - A x_k|` in exact arithmetic) with one host read per iteration.  When
    every system passes, the true residual is computed once; a system that misses the rule is restarted from the
    current iterate with that residual as right-hand side, at most ``max_restart`` times (with a preconditioner
    :math:`\bar\phi` is the :math:`P`-norm of the residual: a restart therefore asks the recurrence for the reduction
    the true norm still lacks).  The returned iterate is
    always one whose true residual was computed; a ``ConvergenceWarning`` carries its norm when the rule is not met.

    Keyword arguments
    -----------------
    precond: LinearOperator or None
        Hermitian POSITIVE DEFINITE preconditioner (not checked, except that :math:`\langle r, P r\rangle < 0` raises)
    max_niter: int or None
        Maximum number of iterations over all restarts (default ``int(1.5 * A.shape[-1])``)
    rtol, atol: float
        Relative / absolute tolerance of the stopping condition w.r.t. the norm of B
    max_restart: int
        Maximum number of restarts after a failed true-residual confirmation
    verbose: bool
        Print the progress
    process_group: torch.distributed group or None
        batch-sharded multi-GPU run: the stopping test is all-reduced over the group
    trace: dict or None
        receives ``niter``, ``napply``, ``converged``, ``best_resid`` (true), ``nrestart``, ``resid_history``

    ``A`` and ``M`` must be Hermitian and ``E`` real (``RuntimeError`` otherwise: use ``bicgstab`` or ``gmres``);
    ``posdef`` is accepted and ignored.
    """
    if not _in_host_memory(A):                                       # (the host driver checks its own)
        E = host_krylov.check_minres_inputs(A, M, E)
    run = _Run("minres", A, B, E, M, dict(
        precond=precond, max_niter=max_niter, rtol=rtol, atol=atol, max_restart=max_restart, verbose=verbose,
        process_group=process_group, trace=trace), True, True)            # Hermitian: never the normal equations
    if run.X is not None:
        return run.X
    prob, kr, stop, max_niter = run.prob, run.kr, run.stop, run.max_niter
    pre = _precond(precond, prob)
    S, N, ld, nblk = prob.S, prob.N, prob.ld, kr.nblk

    x, v, Av, tmp, rtrue = (prob.new() for _ in range(5))
    r1, r2 = prob.new(), prob.rhs.clone()                            # x0 = 0: the first right-hand side is B
    w1, w2 = prob.new(), prob.new()
    ybuf = prob.new() if pre is not None else None
    state = K.minres_state(S, prob.device)
    Palpha, Pdot = kr.partial(), (kr.partial() if pre is not None else None)
    Pbeta, Pphi, Prr = kr.partial_real(), kr.partial_real(), kr.partial_real()
    flagged = torch.zeros((1,), dtype=torch.float64, device=prob.device)

    stop_rec = stop

    def status(k):
        """the iteration's one host read; a non-finite maximum is looked into: the preconditioner flag raises"""
        mx, nbad = kr.check_status(Pphi, stop_rec, process_group, nblk=1)
        if mx != mx or mx == float("inf"):
            flagged[0] = (state[k & 1, :, 7] == 2).any().double()
            allreduce_max_(flagged, process_group)
            if flagged.item() != 0:
                raise RuntimeError("minres: <r, P r> < 0: the preconditioner is not positive definite")
        return mx, nbad

    k, nrestart, hist = 0, 0, []
    converged, best = False, float("inf")
    while True:
        y = r2
        if pre is not None:
            pre.apply(r2, ybuf)
            y = ybuf
        kr.dots(r2, y, Palpha)                                       # <b, P b>
        K.minres_init(y, v, Palpha, state, Pphi, S, N, ld, nblk, k)
        if nrestart > 0:
            # restart: the recurrence has to fall by the factor the TRUE norm still has to fall by (with a
            # preconditioner phibar is the P-norm of the residual, not its 2-norm), and by 2 for safety
            rt = rtrue_norm.double()
            scaled = 0.5 * state[k & 1, :, 6] * stop.double() / torch.where(rt == 0, torch.ones_like(rt), rt)
            stop_rec = torch.minimum(stop_rec, scaled.to(stop.dtype)).contiguous()
        mx, nbad = status(k)
        rec_ok = nbad == 0
        while not rec_ok and k < max_niter:
            sh = prob.apply(v, Av, defer=True)
            kr.dots(v, Av, Palpha, shift=sh)                         # alpha = <v, A v>, shift folded in
            K.minres_lanczos(Av, r2, r1, Palpha, state, Pbeta if pre is None else None, S, N, ld, nblk, k)
            r1, r2 = r2, r1
            y = r2
            if pre is not None:
                pre.apply(r2, ybuf)
                kr.dots(r2, ybuf, Pdot)                              # beta^2 = <r2, P r2>
                y = ybuf
            K.minres_update(v, y, w1, w2, x, Palpha, Pbeta if pre is None else Pdot, pre is not None, state, Pphi,
                            S, N, ld, nblk, k)
            w1, w2 = w2, w1
            k += 1
            mx, nbad = status(k)
            hist.append(mx)
            if verbose and (k < 10 or k % 10 == 0):
                print("%4d: |dy|=%.3e" % (k, mx))
            if nbad == 0:
                rec_ok = True
            elif mx != mx or mx == float("inf"):
                break
        prob.apply(x, tmp)                                           # confirmation on the true residual
        kr.resid(prob.rhs, tmp, rtrue, None, Prr, None)
        best, nbad = kr.check_status(Prr, stop, process_group)
        if nbad == 0:
            converged = True
            break
        if not rec_ok or nrestart >= max_restart or k >= max_niter:
            break
        nrestart += 1                                                # restart from x with the true residual
        rtrue_norm = kr.rnorm.clone()
        r2.copy_(rtrue)
        w1.zero_()
        w2.zero_()
    return run.finish(x, converged, best, k, k, nrestart=nrestart, resid_history=hist)


def scipy_gmres(A, B, E=None, M=None, min_eps=1e-9, max_niter=None, **unused):
    """The reference's `method="scipy_gmres"` (wrap_gmres, solve.py:14-66): SciPy's GMRES on the host, one system at a
    time, with the operator applied wherever it lives (the reference copies every iterate between the host and the
    operator's device as well)."""
    return host_krylov.scipy_gmres(A, B, E, M, min_eps=min_eps, max_niter=max_niter)


# ------------------------------------------------------------------------------- root-finder based
def broyden1_solve(A, B, E=None, M=None, **options):
    """Solve ``A X - M X E = B`` as a root-finding problem with Broyden's first method
    (reference: broyden1_solve/_rootfinder_solve, solve.py:447-478)."""
    from xitorch_amd.optimize.native_root import broyden1
    nr = A.shape[-1]
    ncols = B.shape[-1]

    def residual(xi):
        x = xi.reshape(*xi.shape[:-1], nr, ncols)
        y = A.mm(x) - B
        if E is not None:
            MX = M.mm(x) if M is not None else x
            y = y - MX * E.unsqueeze(-2)
        return y.reshape(*xi.shape[:-1], -1)

    bdims = get_batchdims(A, B, E, M)
    x0 = torch.zeros((*bdims, nr * ncols), dtype=A.dtype, device=A.device)
    x = broyden1(residual, x0, **options)
    return x.reshape(*x.shape[:-1], nr, ncols)
